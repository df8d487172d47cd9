"""GPU: baked feature volumes (csrc/volume.hip) through ops.bake_feature_volume / ops.render_feature_volume,
GeneratorNerfINR.bake_features and evaluation.render_feature_volume.

  oracle     against the fp64 yardstick tests/feature_volume_oracle.py (tests/volume_oracle.py, eleven times) on the cases
             tests/test_feature_volume_oracle_cpu.py holds to itself: |err| <= bar on every pixel that is not `near` a box face,
             for all 32 channels, depth and opacity.
  rgb        a feature volume whose every group carries a packed (r, g, b, sigma) volume renders ops.render_volume's bits in
             every group: the lerp order, the composite and the top-ups are those of a kernel that passed its own yardstick.
  skips      brick skip on / off / without occ, an opaque volume, an empty one, the top-up fetch: equal bits.
  batching   one volume for three cameras, a volume per camera, the volumes swapped.
  bake       the planes are the features' bits in the documented layout; the generator's volume is NeRFNetwork.evaluate's.
  end to end the image is the generator's own head on the composited features, and it approaches forward()'s as the lattice
             is refined (profiles/feature_volume.txt keeps the measured errors).

MEASURED on an MI355X, the largest error over its bar (`pytest -s` prints every figure): features 0.044
(inside_16_s12_relu_last_smooth), 0.037 (outside_16_s2_relu_white), 0.012 - 0.023 on the other cases that see the volume; depth at
most 0.017, opacity at most 0.034; the opaque volume 0.040; no case has a `near` pixel.  Convergence: 1.0e-4 at N = 24, 2e-5 at
N = 48, ratio 3.98."""
from types import SimpleNamespace

import pytest
import torch

import feature_volume_oracle as fo
import volume_oracle as vo
from conftest import seeded_generator

pytestmark = pytest.mark.gpu
CASES = fo.cases()


def dev():
    return torch.device("cuda")


def _bake(case):
    from cips3d_amd import ops
    sigma = case.sigma.to(dev())
    planes, occ = ops.bake_feature_volume(sigma, case.feat.to(dev()))
    return sigma, planes, occ


def _render(case, sigma, planes, occ, **over):
    from cips3d_amd import ops
    a = dict(clamp_mode=case.clamp_mode, last_back=case.last_back, white_back=case.white_back, skip=case.clamp_mode == 'relu',
             cam2world=case.cam2world)
    a.update(over)
    cams = a.pop("cam2world").to(dev())
    return ops.render_feature_volume(sigma, planes, occ, case.lo, case.hi, cams, case.zc, case.H, case.W, zg=case.zg.to(dev()), **a)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _planes_by_torch(feat):
    """(Bv,nx,ny,nz,32) -> (Bv,8,nx,ny,nz,4): group g holds channels 4g .. 4g+3"""
    Bv, nx, ny, nz, _ = feat.shape
    return feat.view(Bv, nx, ny, nz, 8, 4).permute(0, 4, 1, 2, 3, 5).contiguous()


# ------------------------------------------------------------------ 1. against fp64

@pytest.mark.parametrize("name", fo.NAMES)
def test_render_against_the_oracle(name):
    case, ref = CASES[name], fo.reference(name)
    vol = _bake(case)
    fea, depth, opacity = _render(case, *vol)
    b = case.cam2world.shape[0]
    assert fea.shape == (b, case.H * case.W, 32) and depth.shape == opacity.shape == (b, 1, case.H, case.W)
    assert all(bool(torch.isfinite(t).all()) for t in (fea, depth, opacity)) and not fea.requires_grad and fea.grad_fn is None
    q = fo.compare(ref, fea, depth, opacity)
    print(f"{name}: fea {q.fea:.4f}, depth {q.depth:.4f}, opacity {q.opacity:.4f} of the bar; {int(ref.near.sum())} near pixels, "
          f"{int(ref.sees.sum())} of {ref.sees.numel()} see the volume")
    assert q.fea <= 1 and q.depth <= 1 and q.opacity <= 1 and not bool(q.over.any())
    if case.clamp_mode == 'relu':
        assert _equal((fea, depth, opacity), _render(case, *vol, skip=False))


# ------------------------------------------------------------------ 2. the rgb renderer's bits

@pytest.mark.parametrize("name", ["corner_16_s12_relu_last", "corner_16_s12_softplus_white", "turntable_16_s12_relu"])
def test_every_group_renders_the_rgb_renderers_bits(name):
    from cips3d_amd import ops
    case = vo.cases()[name]
    assert (name.endswith("relu_last") and case.last_back) or (name.endswith("softplus_white") and case.white_back) or "turntable" in name
    sigma = case.sigma.to(dev())
    packed, occ = ops.bake_volume(sigma, case.rgb.to(dev()))
    planes, occ_f = ops.bake_feature_volume(sigma, packed.repeat(1, 1, 1, 1, 8))         # every group: (r, g, b, sigma)
    assert torch.equal(occ_f, occ)
    kw = dict(clamp_mode=case.clamp_mode, last_back=case.last_back, white_back=case.white_back, skip=case.clamp_mode == 'relu',
              zg=case.zg.to(dev()))
    cams = case.cam2world.to(dev())
    rgb, depth, opacity = ops.render_volume(packed, occ, case.lo, case.hi, cams, case.zc, case.H, case.W, **kw)
    fea, depth_f, opacity_f = ops.render_feature_volume(sigma, planes, occ, case.lo, case.hi, cams, case.zc, case.H, case.W, **kw)
    assert torch.equal(depth_f, depth) and torch.equal(opacity_f, opacity)
    want = rgb.reshape(cams.shape[0], 3, case.H * case.W).transpose(1, 2)
    assert float(want.abs().max()) > 0.1
    for g in range(8):
        assert torch.equal(fea[..., 4 * g:4 * g + 3], want), g


# ------------------------------------------------------------------ 3. the skips change no bit

def _half_empty_case(scale=40.0, **flags):
    """17 x 17 x 10 nodes (2 x 2 x 2 bricks): sigma <= 0 on the nodes x <= 8 — the whole bricks I = 0 — and of both signs beyond"""
    g = torch.Generator().manual_seed(31)
    sigma = torch.randn(1, 17, 17, 10, generator=g) * scale
    sigma[:, :9] = -sigma[:, :9].abs()
    sigma[:, 3, 4, 5], sigma[:, 8, 8, 8] = 0.0, -0.0
    base = vo.make_case(sigma, torch.zeros(1, 17, 17, 10, 3), vo.cameras([0.8, 2.2], [1.2, 1.9]), 16, 16, 16, 0.8, 1.2, 12, **flags)
    return fo.with_features(base, fo.random_features(32, 1, 17, 17, 10))


@pytest.mark.parametrize("white_back", [False, True])
@pytest.mark.parametrize("last_back", [False, True])
def test_brick_skip_changes_no_bit(last_back, white_back):
    case = _half_empty_case()
    sigma, planes, occ = _bake(case)
    assert occ.shape == (1, 2, 2, 2) and bool((occ[0, 0] <= 0).all()) and bool((occ[0, 1] > 0).all())
    kw = dict(last_back=last_back, white_back=white_back)
    on = _render(case, sigma, planes, occ, skip=True, **kw)
    off = _render(case, sigma, planes, occ, skip=False, **kw)
    no_occ = _render(case, sigma, planes, None, skip=False, **kw)
    assert _equal(on, off) and _equal(off, no_occ)
    assert float(on[2].max()) > 0.5                                             # the volume is seen
    assert _equal(on, _render(case, sigma, planes, occ, skip=True, **kw))       # two calls


@pytest.mark.parametrize("last_back", [False, True])
def test_an_opaque_volume_ends_its_feature_traffic_and_stays_exact(last_back):
    """sigma in the thousands: alpha = 1 at the first sample inside, T falls by 1e-10 per sample and fp32(T) is exactly 0 five
    samples later, so most samples of a ray have weight zero and fetch no features.  Build-independent check: the fp64 oracle
    with its bars, which the same rule in fp32 torch meets too."""
    g = torch.Generator().manual_seed(41)
    sigma = 2000 + 2000 * torch.rand(1, 9, 17, 10, generator=g)
    base = vo.make_case(sigma, torch.zeros(1, 9, 17, 10, 3), vo.cameras([0.7, 2.0], [1.9, 1.2]), 16, 16, 16, 0.8, 1.2, 12,
                        last_back=last_back)
    case = fo.with_features(base, fo.random_features(42, 1, 9, 17, 10))
    ref = fo.render(case, bars=True)
    t32 = fo.render(case, dtype=torch.float32)
    assert not bool(fo.compare(ref, t32.fea, t32.depth, t32.opacity).over.any())
    vol = _bake(case)
    out = _render(case, *vol)
    q = fo.compare(ref, *out)
    print(f"opaque, last_back={last_back}: fea {q.fea:.4f}, depth {q.depth:.4f}, opacity {q.opacity:.4f} of the bar")
    assert q.fea <= 1 and q.depth <= 1 and q.opacity <= 1
    assert float(ref.opacity.max()) > 0.999 and float(ref.near.double().mean()) <= 0.02
    assert _equal(out, _render(case, *vol)) and _equal(out, _render(case, *vol, skip=False))


@pytest.mark.parametrize("inside_camera", [False, True], ids=["outside", "inside"])
def test_an_empty_volume_renders_exactly_nothing_and_the_top_up_fetches(inside_camera):
    g = torch.Generator().manual_seed(51)
    sigma = -1 - torch.rand(2, 9, 17, 10, generator=g)
    sigma[:, 1, 16, 9], sigma[:, 8, 2, 3] = 0.0, -0.0
    zero = torch.zeros(2, 9, 17, 10, 3)
    if inside_camera:            # every sample lies within 0.06 of the origin, the box reaches 0.10 and more on every side
        base = vo.make_case(sigma, zero, vo.cameras([0.9, 2.1], [1.25, 1.7], radius=0.05), 50, 16, 16, 0.01, 0.09, 12)
    else:
        base = vo.make_case(sigma, zero, vo.cameras([0.8, 2.2], [1.2, 1.9]), 16, 16, 16, 0.8, 1.2, 12)
    case = fo.with_features(base, fo.random_features(52, 2, 9, 17, 10))
    sigma_d, planes, occ = _bake(case)
    assert bool((occ <= 0).all())
    for last_back in (False, True):
        for white_back in (False, True):
            on = _render(case, sigma_d, planes, occ, last_back=last_back, white_back=white_back, skip=True)
            assert _equal(on, _render(case, sigma_d, planes, occ, last_back=last_back, white_back=white_back, skip=False))
            fea, depth, opacity = on
            back = 1.0 if white_back else 0.0
            assert bool((opacity == 0).all())
            if not last_back:
                assert bool((depth == 0).all()) and bool((fea == back).all())
                continue
            # every weight is zero and the top-up is 1 - 0: the last sample's features arrive whole (its fetch is the top-up's)
            assert bool((depth == float(case.zg[-1])).all())
            flat = SimpleNamespace(**{**vars(case), "last_back": True, "white_back": white_back})
            ref = fo.render(flat, bars=True)
            q = fo.compare(ref, fea, depth, opacity)
            assert q.fea <= 1 and q.depth <= 1 and q.opacity == 0
            if inside_camera:
                assert bool(ref.sees.all()) and float((fea - back).abs().amax(-1).min()) > 0.1
                assert float((ref.fea - back).abs().max()) > 0.5
            else:
                assert bool((fea == back).all())                                # ray_end lies beyond the box


# ------------------------------------------------------------------ 4. batching

def test_one_volume_for_three_cameras_equals_three_calls():
    case = CASES["turntable_16_s12_relu"]
    vol = _bake(case)
    one = _render(case, *vol)
    assert not torch.equal(one[0][0], one[0][1])                                # the cameras do differ
    for i in range(3):
        assert _equal([t[i:i + 1] for t in one], _render(case, *vol, cam2world=case.cam2world[i:i + 1]))


def test_a_volume_per_camera_equals_single_calls_and_swaps_with_its_volumes():
    case = CASES["pairs_5x7_s12_softplus_last"]
    sigma, planes, occ = _bake(case)
    both = _render(case, sigma, planes, occ)
    for i in range(2):
        alone = _render(case, sigma[i:i + 1], planes[i:i + 1], occ[i:i + 1], cam2world=case.cam2world[i:i + 1])
        assert _equal([t[i:i + 1] for t in both], alone)
    swapped = _render(case, sigma.flip(0), planes.flip(0), occ.flip(0), cam2world=case.cam2world.flip(0))
    assert _equal([t.flip(0) for t in both], swapped)
    assert not torch.equal(both[0][0], both[0][1])


# ------------------------------------------------------------------ 5. the bake

@pytest.mark.parametrize("Bv", [1, 3])
@pytest.mark.parametrize("shape", [(2, 2, 2), (5, 6, 7), (9, 17, 10)], ids=lambda s: "x".join(map(str, s)))
def test_bake_copies_bits_into_the_documented_layout(shape, Bv):
    from cips3d_amd import ops
    sigma, rgb = vo.random_volume(200 + Bv, Bv, *shape)
    feat = fo.random_features(300 + Bv, Bv, *shape)
    planes, occ = ops.bake_feature_volume(sigma.to(dev()), feat.to(dev()))
    assert planes.shape == (Bv, 8, *shape, 4) and planes.dtype == torch.float32 and planes.data_ptr() % 16 == 0
    assert torch.equal(planes.cpu(), _planes_by_torch(feat))
    rows = ops.bake_feature_volume(sigma.to(dev()), feat.view(Bv, -1, 32).to(dev()))         # the (Bv, P, 32) form
    assert _equal(rows, (planes, occ))
    assert torch.equal(occ, ops.bake_volume(sigma.to(dev()), rgb.to(dev()))[1])


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _zs(seed, b):
    g = torch.Generator().manual_seed(seed)
    return {"z_nerf": torch.randn(b, 256, generator=g).to(dev()), "z_inr": torch.randn(b, 512, generator=g).to(dev())}


def test_bake_features_on_the_generator(x3):
    from cips3d_amd import evaluation, ops
    N, L = 16, 0.3
    G = seeded_generator(8, device=dev())
    zs = _zs(82, 2)
    vol = G.bake_features(zs, resolution=N, cube_length=L)
    assert vol.sigma.shape == (2, N, N, N) and vol.features.shape == (2, 8, N, N, N, 4) and vol.occupancy.shape == (2, 2, 2, 2)
    assert vol.resolution == N and tuple(vol.styles) == G.style_names and all(t.shape[0] == 2 for t in vol.styles.values())
    assert not vol.features.requires_grad and not vol.sigma.requires_grad
    grids = evaluation.density_lattice(N, L, (0., 0., 0.))
    assert vol.lo == tuple(float(g[0]) for g in grids) and vol.hi == tuple(float(g[-1]) for g in grids)
    gx, gy, gz = (g.to(dev()) for g in grids)
    with torch.no_grad():
        feat, sigma = G.siren.evaluate(ops.lattice_points(gx, gy, gz, 2).contiguous(), vol.styles)
    assert torch.equal(vol.sigma, sigma.view(2, N, N, N))
    assert torch.equal(vol.features, _planes_by_torch(feat.view(2, N, N, N, 32)))
    # the density entry points' sigma on the same lattice with the volume's own styles, and (psi = 1) density_grid's
    assert torch.equal(vol.sigma, G.siren.density_lattice(gx, gy, gz, vol.styles))
    assert torch.equal(vol.sigma, G.density_grid(zs, resolution=N, cube_length=L))
    assert torch.equal(vol.occupancy, ops.bake_feature_volume(vol.sigma, feat)[1])
    for slab in (1, 5):                                                          # 5 does not divide 16: a short last slab
        again = G.bake_features(zs, resolution=N, cube_length=L, slab=slab)
        assert _equal((again.sigma, again.features, again.occupancy), (vol.sigma, vol.features, vol.occupancy)), slab


# ------------------------------------------------------------------ 6. end to end

def test_the_image_is_the_generators_own_head_on_the_composited_features(x3, tmp_path):
    from cips3d_amd import evaluation, ops
    from cips3d_amd.generator import _ToRGBFunction, _zc
    N, L, FOV, H = 16, 0.3, 12, 16
    G = seeded_generator(8, device=dev())
    vol = G.bake_features(_zs(82, 1), resolution=N, cube_length=L)
    cams = evaluation.orbit_cameras([1.2, 1.6, 1.9], [1.45, 1.5, 1.7], device=dev())
    for kw in (dict(), dict(last_back=True), dict(white_back=True, skip=False), dict(clamp_mode='softplus', skip=False)):
        out = evaluation.render_feature_volume(G, vol, cams, FOV, H, 0.88, 1.12, 12, return_aux_img=True, **kw)
        assert out.imgs.shape == out.aux.shape == (3, 3, H, H) and out.depth.shape == out.opacity.shape == (3, 1, H, H)
        assert out.features.shape == (3, H * H, 32) and out.cam2world is cams and not out.imgs.requires_grad
        parts = ops.render_feature_volume(vol.sigma, vol.features, vol.occupancy, vol.lo, vol.hi, cams, _zc(FOV), H, H,
                                          ray_start=0.88, ray_end=1.12, num_steps=12, **kw)
        assert _equal((out.features, out.depth, out.opacity), parts)
        with torch.no_grad():
            styles = {k: v.expand(3, -1).contiguous() for k, v in vol.styles.items()}
            rows = G.inr_net(out.features, styles)                               # WITHOUT img_size, as forward() calls it
            want = G.filters(rows.view(3, H, H, 3).permute(0, 3, 1, 2)).contiguous()
            aux = torch.tanh(G.aux_to_rbg[0](out.features)).view(3, H, H, 3).permute(0, 3, 1, 2)
        assert torch.equal(out.imgs, want) and bool(torch.isfinite(out.imgs).all())
        assert torch.allclose(out.aux, aux, rtol=0, atol=1e-5)                   # nn.Linear in place of the ToRGB kernel
        with torch.no_grad():                                                    # and the generator's own layer: the bits
            own = torch.tanh(_ToRGBFunction.apply(out.features, G.aux_to_rbg[0].weight, G.aux_to_rbg[0].bias))
        assert torch.equal(out.aux, own.view(3, H, H, 3).permute(0, 3, 1, 2))
        plain = evaluation.render_feature_volume(G, vol, cams, FOV, H, 0.88, 1.12, 12, **kw)
        assert torch.equal(plain.imgs, out.imgs) and not hasattr(plain, "aux")
    path = tmp_path / "feature_volume.png"
    evaluation.save_image(out.imgs, str(path), nrow=3, normalize=True, value_range=(-1, 1))
    assert path.stat().st_size > 0
    # a volume per camera
    vol2 = G.bake_features(_zs(83, 2), resolution=N, cube_length=L)
    out2 = evaluation.render_feature_volume(G, vol2, cams[:2], FOV, H, 0.88, 1.12, 12)
    assert out2.imgs.shape == (2, 3, H, H) and bool(torch.isfinite(out2.imgs).all())


def test_the_image_approaches_the_networks_as_the_lattice_is_refined(x3):
    """forward()'s picture without noise, jitter or resampling against the baked one from the same styles and camera.  The box
    (half-width 0.25) holds every sample: a sample is at most |z - 1| <= 0.12 from the origin along the view axis and
    1.12 tan(6 deg) sqrt(2) = 0.167 across it, 0.21 in all.  A condition, not a number: the error at N = 48 is smaller than at
    N = 24; profiles/feature_volume.txt keeps the figures."""
    from cips3d_amd import evaluation
    FOV, H, S, L = 12, 16, 12, 0.5
    G = seeded_generator(8, device=dev())
    zs = _zs(84, 1)
    kw = dict(img_size=H, fov=FOV, ray_start=0.88, ray_end=1.12, num_steps=S)
    with torch.no_grad():
        styles = G.styles(zs)
        net = G.render_styles(styles, h_stddev=0., v_stddev=0., h_mean=1.3, v_mean=1.45, hierarchical_sample=False, nerf_noise=0.,
                              sample_dist="gaussian", last_back=True,
                              rand_override={"jitter": torch.full((1, H * H, S, 1), 0.5, device=dev())}, **kw)
    err = {}
    for N in (24, 48):
        vol = G.bake_features(zs, resolution=N, cube_length=L)
        assert all(torch.equal(vol.styles[k], styles[k]) for k in styles)
        out = evaluation.render_feature_volume(G, vol, net.cam2world, FOV, H, 0.88, 1.12, S, last_back=True)
        err[N] = float((out.imgs - net.imgs).abs().mean())
    print(f"mean |image difference| to the network: N=24 {err[24]:.5f}, N=48 {err[48]:.5f}, ratio {err[24] / err[48]:.2f}")
    assert err[48] < err[24]
