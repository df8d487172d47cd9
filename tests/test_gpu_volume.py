"""GPU: baked radiance volumes (csrc/volume.hip) through ops.bake_volume / ops.render_volume, GeneratorNerfINR.bake and
evaluation.render_volume.

  bake       channels are the inputs' bits; the brick occupancy equals torch's amax over the node ranges of the header, bit for
             bit (a maximum has no rounding).
  render     against the fp64 yardstick tests/volume_oracle.py on the cases tests/test_volume_oracle_cpu.py holds to itself:
             |err| <= bar on every pixel that is not `near` a box face, the bar derived there from fp32 eps alone.
  exactness  skip on / off, two calls, one volume for three cameras against three copies: equal bits.  A volume with sigma <= 0
             everywhere renders exactly nothing.
  end to end on the small seeded generator at N = 17.

MEASURED on an MI355X, the largest error over its bar (`pytest -s` prints every figure; profiles/volume_render.txt keeps the
maxima): rgb 0.038 (outside_16_s2_relu_white, inside_16_s12_relu_last_smooth), 0.026 (inside_5x7_s2_softplus), 0.005 - 0.019 on
the other cases that see the volume; depth 0.017 and opacity 0.034 (inside_16_s12_relu_last_smooth), at most 0.015 elsewhere; no
case has a `near` pixel.  The bar adds magnitudes of worst cases, so a correct kernel sits far inside it;
tests/test_volume_oracle_cpu.py shows that wrong rules do not."""
from types import SimpleNamespace

import pytest
import torch

import volume_oracle as vo
from conftest import seeded_generator

pytestmark = pytest.mark.gpu
CASES = vo.cases()


def dev():
    return torch.device("cuda")


def _bake(case):
    from cips3d_amd import ops
    return ops.bake_volume(case.sigma.to(dev()), case.rgb.to(dev()))


def _render(case, packed, occ, **over):
    from cips3d_amd import ops
    a = dict(clamp_mode=case.clamp_mode, last_back=case.last_back, white_back=case.white_back, skip=case.clamp_mode == 'relu',
             cam2world=case.cam2world)
    a.update(over)
    cams = a.pop("cam2world").to(dev())
    return ops.render_volume(packed, occ, case.lo, case.hi, cams, case.zc, case.H, case.W, zg=case.zg.to(dev()), **a)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ bake

def _occ_by_torch(sigma):
    Bv, nx, ny, nz = sigma.shape
    nb = [-(-(n - 1) // 8) for n in (nx, ny, nz)]
    out = torch.empty(Bv, *nb)
    for I in range(nb[0]):
        for J in range(nb[1]):
            for K in range(nb[2]):
                out[:, I, J, K] = sigma[:, 8 * I:min(8 * I + 8, nx - 1) + 1, 8 * J:min(8 * J + 8, ny - 1) + 1,
                                        8 * K:min(8 * K + 8, nz - 1) + 1].amax((1, 2, 3))
    return out


@pytest.mark.parametrize("Bv", [1, 3])
@pytest.mark.parametrize("shape", [(2, 2, 2), (5, 6, 7), (9, 17, 10), (18, 9, 9)], ids=lambda s: "x".join(map(str, s)))
def test_bake_copies_bits_and_takes_exact_brick_maxima(shape, Bv):
    from cips3d_amd import ops
    sigma, rgb = vo.random_volume(100 + Bv, Bv, *shape)
    packed, occ = ops.bake_volume(sigma.to(dev()), rgb.to(dev()))
    assert packed.shape == (Bv, *shape, 4) and packed.dtype == torch.float32 and packed.data_ptr() % 16 == 0
    assert torch.equal(packed[..., :3].cpu(), rgb) and torch.equal(packed[..., 3].cpu(), sigma)
    want = _occ_by_torch(sigma)
    assert occ.shape == want.shape and torch.equal(occ.cpu(), want)
    # a brick maximum that sits ONLY on the shared upper face is seen by both neighbours
    if shape[0] > 9:
        sigma2 = -sigma.abs() - 1
        sigma2[:, 8, 3, 3] = 5.0
        _, occ2 = ops.bake_volume(sigma2.to(dev()), rgb.to(dev()))
        assert torch.equal(occ2.cpu(), _occ_by_torch(sigma2)) and bool((occ2[:, 0, 0, 0] == 5).all()) and bool((occ2[:, 1, 0, 0] == 5).all())


# ------------------------------------------------------------------ render against the oracle

@pytest.mark.parametrize("name", list(CASES))
def test_render_against_the_oracle(name):
    case, ref = CASES[name], vo.reference(name)
    packed, occ = _bake(case)
    rgb, depth, opacity = _render(case, packed, occ)
    b = case.cam2world.shape[0]
    assert rgb.shape == (b, 3, case.H, case.W) and depth.shape == opacity.shape == (b, 1, case.H, case.W)
    assert all(bool(torch.isfinite(t).all()) for t in (rgb, depth, opacity))
    q = vo.compare(ref, rgb, depth, opacity)
    print(f"{name}: rgb {q.rgb:.4f}, depth {q.depth:.4f}, opacity {q.opacity:.4f} of the bar; {int(ref.near.sum())} near pixels, "
          f"{int(ref.sees.sum())} of {ref.sees.numel()} see the volume")
    assert q.rgb <= 1 and q.depth <= 1 and q.opacity <= 1
    if case.clamp_mode == 'relu':
        assert _equal((rgb, depth, opacity), _render(case, packed, occ, skip=False))


def test_constant_colour_volume_returns_the_colour_times_opacity():
    """rgb_ref = c opacity_ref exactly, so |rgb - c opacity| <= bar_rgb + |c| bar_opacity for outputs within their bars"""
    base = CASES["turntable_16_s12_relu"]
    colour = torch.tensor([0.25, -0.5, 0.75])
    case = SimpleNamespace(**vars(base))
    case.rgb = colour.expand_as(base.rgb).contiguous()
    ref = vo.render(case, bars=True)
    rgb, depth, opacity = _render(case, *_bake(case))
    q = vo.compare(ref, rgb, depth, opacity)
    assert q.rgb <= 1 and q.depth <= 1 and q.opacity <= 1
    c = colour.view(1, 3, 1, 1).double()
    err = (rgb.cpu().double() - c * opacity.cpu().double()).abs()
    bound = ref.bar_rgb + c.abs() * ref.bar_opacity
    keep = ~ref.near.unsqueeze(1).expand_as(err)
    assert bool((err <= bound)[keep].all()) and float(opacity.max()) > 0.5


# ------------------------------------------------------------------ exactness

BLOBS = (((14, 19), (2, 6), (6, 10)), ((1, 5), (10, 18), (1, 4)))            # per volume, per axis: the node range [from, to)


def _blob_case(all_nonpositive, inside_camera=False):
    """Two volumes of 26 x 19 x 10 nodes: 4 x 3 x 2 bricks, a different count on every axis.  sigma in [-2, -1) except at a few
    exact zeros (both signs), plus — unless all_nonpositive — one positive blob per volume, off the diagonal and elsewhere in
    each: volume 0 across the brick faces at x = 16 and z = 8 (bricks {1, 2} x {0} x {0, 1}), volume 1 across the face at
    y = 16 (bricks {0} x {1, 2} x {0}).  No permutation of the brick indices, no mixed-up stride and no forgotten per-volume
    offset maps these sets onto themselves."""
    g = torch.Generator().manual_seed(77)
    sigma = -1 - torch.rand(2, 26, 19, 10, generator=g)
    sigma[:, 25, 17, 1], sigma[:, 1, 16, 9], sigma[:, 24, 2, 9] = 0.0, -0.0, 0.0          # in bricks no blob touches
    if not all_nonpositive:
        for v, ((x0, x1), (y0, y1), (z0, z1)) in enumerate(BLOBS):
            sigma[v, x0:x1, y0:y1, z0:z1] = 400 * torch.rand(x1 - x0, y1 - y0, z1 - z0, generator=g)
    rgb = torch.rand(2, 26, 19, 10, 3, generator=g) * 2 - 1
    if inside_camera:            # every sample lies within 0.06 of the origin, the box reaches 0.10 and more on every side
        return vo.make_case(sigma, rgb, vo.cameras([0.9, 2.1], [1.25, 1.7], radius=0.05), 50, 16, 16, 0.01, 0.09, 12)
    return vo.make_case(sigma, rgb, vo.cameras([0.8, 2.2], [1.2, 1.9]), 16, 16, 16, 0.8, 1.2, 12)


def _positive_bricks(v):
    want = torch.zeros(4, 3, 2, dtype=torch.bool)
    (x0, x1), (y0, y1), (z0, z1) = BLOBS[v]
    for I in range(4):
        for J in range(3):
            for K in range(2):          # brick (I, J, K) reads nodes 8I .. 8I + 8 (inclusive) per axis
                want[I, J, K] = (x0 <= 8 * I + 8 and x1 > 8 * I) and (y0 <= 8 * J + 8 and y1 > 8 * J) and (z0 <= 8 * K + 8 and z1 > 8 * K)
    return want


@pytest.mark.parametrize("white_back", [False, True])
@pytest.mark.parametrize("last_back", [False, True])
def test_skip_changes_no_bit(last_back, white_back):
    case = _blob_case(False)
    packed, occ = _bake(case)
    assert occ.shape == (2, 4, 3, 2)
    for v, n in ((0, 4), (1, 2)):
        assert torch.equal((occ[v] > 0).cpu(), _positive_bricks(v)) and int((occ[v] > 0).sum()) == n
    kw = dict(last_back=last_back, white_back=white_back)
    on = _render(case, packed, occ, skip=True, **kw)
    off = _render(case, packed, occ, skip=False, **kw)
    no_occ = _render(case, packed, None, skip=False, **kw)
    assert _equal(on, off) and _equal(off, no_occ)
    for v in range(2):                                                        # each blob is seen, and so is empty space
        assert float(on[2][v].max()) > 0.5 and float(on[2][v].min()) == 0
    assert _equal(on, _render(case, packed, occ, skip=True, **kw))            # two calls
    # the volumes the other way round under the same cameras: other pictures, and again the same bits with and without the skip
    swapped = _render(case, packed.flip(0), occ.flip(0), skip=True, **kw)
    assert _equal(swapped, _render(case, packed.flip(0), None, skip=False, **kw)) and not torch.equal(swapped[2], on[2])
    # one volume for both cameras (Bv = 1): volume v alone
    for v in range(2):
        alone = _render(case, packed[v:v + 1], occ[v:v + 1], skip=True, **kw)
        assert _equal(alone, _render(case, packed[v:v + 1], None, skip=False, **kw))
        assert _equal([t[v] for t in alone], [t[v] for t in on])


@pytest.mark.parametrize("inside_camera", [False, True], ids=["outside", "inside"])
def test_a_nonpositive_volume_renders_exactly_nothing(inside_camera):
    case = _blob_case(True, inside_camera)
    packed, occ = _bake(case)
    assert bool((occ <= 0).all())
    zlast = float(case.zg[-1])
    for last_back in (False, True):
        for white_back in (False, True):
            on = _render(case, packed, occ, last_back=last_back, white_back=white_back, skip=True)
            off = _render(case, packed, occ, last_back=last_back, white_back=white_back, skip=False)
            assert _equal(on, off)
            rgb, depth, opacity = on
            assert bool((opacity == 0).all())
            if not last_back:
                assert bool((depth == 0).all()) and bool((rgb == (1.0 if white_back else 0.0)).all())
                continue
            # the top-up 1 - 0 goes to the last sample: its depth exactly, its colour (zero if it lies outside the box)
            assert bool((depth == zlast).all())
            flat = SimpleNamespace(**vars(case))
            flat.last_back, flat.white_back = True, white_back
            ref = vo.render(flat, bars=True)
            q = vo.compare(ref, rgb, depth, opacity)
            assert q.rgb <= 1 and q.depth <= 1 and q.opacity == 0
            if inside_camera:
                assert bool(ref.sees.all()) and float((rgb - (1.0 if white_back else 0.0)).abs().max()) > 0.5
            else:
                assert bool((rgb == (1.0 if white_back else 0.0)).all())      # ray_end lies beyond the box


def test_one_volume_for_three_cameras_equals_three_copies():
    case = CASES["turntable_16_s12_relu"]
    packed, occ = _bake(case)
    one = _render(case, packed, occ)
    three = _render(case, packed.repeat(3, 1, 1, 1, 1), occ.repeat(3, 1, 1, 1))
    assert _equal(one, three)
    assert not torch.equal(one[0][0], one[0][1])                              # the cameras do differ
    for i in range(3):                                                        # and camera i alone gives image i
        assert _equal([t[i:i + 1] for t in one], _render(case, packed, occ, cam2world=case.cam2world[i:i + 1]))


def test_softplus_ignores_no_sample():
    """softplus has no empty space: ops refuses skip=True with it, and skip=False matches the oracle (above); here: a volume
    that is <= 0 everywhere is NOT empty under softplus"""
    case = _blob_case(True)
    packed, occ = _bake(case)
    with pytest.raises(ValueError, match="skip"):
        _render(case, packed, occ, clamp_mode='softplus', skip=True)
    _, _, opacity = _render(case, packed, occ, clamp_mode='softplus', skip=False)
    assert float(opacity.max()) > 0


# ------------------------------------------------------------------ end to end

@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _zs(seed, b):
    g = torch.Generator().manual_seed(seed)
    return {"z_nerf": torch.randn(b, 256, generator=g).to(dev()), "z_inr": torch.randn(b, 512, generator=g).to(dev())}


def test_bake_and_render_on_the_generator(x3, tmp_path):
    from cips3d_amd import evaluation, ops
    from cips3d_amd.generator import _zc
    N, L, FOV = 17, 0.3, 12
    G = seeded_generator(8, device=dev())
    zs = _zs(82, 1)
    vol = G.bake(zs, resolution=N, cube_length=L)
    rgb_grid, sigma_grid = G.color_grid(zs, resolution=N, cube_length=L, return_sigma=True)
    assert vol.rgbs.shape == (1, N, N, N, 4) and vol.occupancy.shape == (1, 2, 2, 2) and vol.resolution == N
    assert torch.equal(vol.rgbs[..., :3], rgb_grid) and torch.equal(vol.rgbs[..., 3], sigma_grid)
    assert torch.equal(vol.rgbs[..., 3], G.density_grid(zs, resolution=N, cube_length=L))
    grids = evaluation.density_lattice(N, L, (0., 0., 0.))
    assert vol.lo == tuple(float(g[0]) for g in grids) and vol.hi == tuple(float(g[-1]) for g in grids)
    cams = evaluation.orbit_cameras([1.2, 1.6, 1.9], [1.45, 1.5, 1.7], device=dev())
    for kw in (dict(), dict(last_back=True), dict(white_back=True, skip=False), dict(clamp_mode='softplus', skip=False)):
        out = evaluation.render_volume(vol, cams, FOV, 16, 0.88, 1.12, 12, **kw)
        assert out.imgs.shape == (3, 3, 16, 16) and out.depth.shape == out.opacity.shape == (3, 1, 16, 16) and out.cam2world is cams
        assert not out.imgs.requires_grad
        parts = ops.render_volume(vol.rgbs, vol.occupancy, vol.lo, vol.hi, cams, _zc(FOV), 16, 16, ray_start=0.88, ray_end=1.12,
                                  num_steps=12, **kw)
        assert _equal((out.imgs, out.depth, out.opacity), parts)
        assert all(bool(torch.isfinite(t).all()) for t in parts)
        if kw.get('clamp_mode', 'relu') == 'relu':                           # skip on and off on the generator's own volume
            flipped = dict(kw, skip=not kw.get('skip', True))
            assert _equal(parts, ops.render_volume(vol.rgbs, vol.occupancy, vol.lo, vol.hi, cams, _zc(FOV), 16, 16, ray_start=0.88,
                                                   ray_end=1.12, num_steps=12, **flipped))
        assert float(out.opacity.min()) >= 0 and float(out.opacity.max()) <= 1 + 1e-5
    out = evaluation.render_volume(vol, cams, FOV, 16, 0.88, 1.12, 12, last_back=True)
    path = tmp_path / "volume.png"
    evaluation.save_image(out.imgs, str(path), nrow=3, normalize=True, value_range=(-1, 1))
    assert path.stat().st_size > 0
    rolled = evaluation.render_volume(vol, cams.roll(1, 0), FOV, 16, 0.88, 1.12, 12, last_back=True)
    warped = evaluation.warp_view(out, rolled, FOV)
    assert warped.imgs.shape == (3, 3, 16, 16) and bool(torch.isfinite(warped.imgs).all()) and warped.mask.shape == (3, 1, 16, 16)
    # b volumes, b cameras
    vol2 = G.bake(_zs(83, 2), resolution=N, cube_length=L)
    out2 = evaluation.render_volume(vol2, cams[:2], FOV, 16, 0.88, 1.12, 12)
    assert out2.imgs.shape == (2, 3, 16, 16) and bool(torch.isfinite(out2.imgs).all())
