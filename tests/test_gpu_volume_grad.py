"""GPU: the gradient of the baked-volume renderer with respect to its nodes (cips_volume_render_bwd through ops.render_volume's
autograd Function), ops.volume_occupancy, evaluation.render_volume(grad=True) and evaluation.fit_volume.

  oracle     against the fp64 yardstick tests/volume_grad_oracle.py (torch autograd through volume_oracle.render) on the eleven
             cases of volume_oracle and one more of 9 x 10 pixels with two cameras: max|g - g64| / max|g64| per channel group
             within the bar, which is 8 x the same measure of fp32 torch autograd on that case (floor 16 * 2^-24) and comes from
             nothing the kernel computes.  tests/test_volume_grad_oracle_cpu.py shows that wrong rules leave it.
  exactness  what is exactly zero is exactly zero: a camera that misses, a volume with sigma <= 0 everywhere (all of it without
             last_back; its sigma channel with), and the same SET of non-zero nodes with the skip on and off.  Values are
             compared within the bar, not bit for bit, wherever two launches are involved: a node's sum is a sequence of fp32
             atomic adds in arrival order, which differs from launch to launch (and with the skip, which changes the timing of
             every ray), so the last bits of a sum can differ although every term is the same bits.
  fit        fit_volume lowers every image's loss, leaves its input alone and returns the occupancy of what it returns.

MEASURED on an MI355X (`pytest -s` prints every figure; profiles/volume_backward.txt keeps those of the twelve cases): the kernel's
error over its bar is 0.06 - 0.21 for sigma and 0.08 - 0.19 for colour on the cases that see the volume (errors 3.5e-7 ... 2.8e-5
against bars 2.1e-6 ... 4.3e-4), at most 0.32 with one output alone (opacity alone, inside_16_s12_relu_last_white), 0.09 - 0.13 on
the two-blob volumes with the skip on, off and without an occupancy, 0.13 on the non-positive volume under last_back; one volume
under three cameras differs from the sum of the cameras alone by 1.5e-7, two calls by 4e-8, the two shapes of the atomic adds give
ratios within 0.01 of each other.  fit_volume: loss last / first 0.020 - 0.026 (synthetic, 30 steps), 0.54 (one view with depth
and matte terms, 5 steps), 0.06 - 0.10 (the seeded generator at N = 17, 30 steps)."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import volume_grad_oracle as go
import volume_oracle as vo
from conftest import seeded_generator

pytestmark = pytest.mark.gpu
CASES = go.all_cases()


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


def _gradient(case, ups, packed=None, occ=None, **over):
    """-> (d sum(up out) / d packed on the CPU, the three outputs): through autograd; a None upstream is an unused output"""
    if packed is None:
        packed, occ = _bake(case)
    leaf = packed.detach().clone().requires_grad_(True)
    out = _render(case, leaf, occ, **over)
    assert all(o.grad_fn is not None for o in out)
    used = [(o, u.to(dev())) for o, u in zip(out, ups) if u is not None]
    g, = torch.autograd.grad([o for o, _ in used], leaf, [u for _, u in used])
    assert g.shape == packed.shape and g.dtype == torch.float32 and torch.equal(leaf.detach(), packed)      # packed untouched
    return g.cpu(), out


def _report(what, m, bar):
    print(f"{what}: sigma {m[0]:.3e} (bar {bar[0]:.3e}, ratio {m[0] / bar[0]:.3f}), colour {m[1]:.3e} (bar {bar[1]:.3e}, "
          f"ratio {m[1] / bar[1]:.3f})")


# ------------------------------------------------------------------ against the oracle

@pytest.mark.parametrize("name", list(CASES))
def test_gradient_against_the_oracle(name):
    """MEASURED on an MI355X, error / bar (sigma, colour): outside_5x7_s12_relu 0.207, 0.194; outside_16_s12_softplus_last 0.062,
    0.106; outside_16_s2_relu_white 0.132, 0.075; inside_16_s12_relu_last_white 0.088, 0.187; inside_5x7_s2_softplus 0.146, 0.163;
    miss_5x7_s12_relu_white 0, 0; corner_16_s12_relu_last 0.114, 0.113; corner_16_s12_softplus_white 0.066, 0.093;
    turntable_16_s12_relu 0.125, 0.116; inside_16_s12_relu_last_smooth 0.166 - 0.207, 0.146 - 0.181 (two runs: the sums are
    atomic); pairs_5x7_s12_softplus_last 0.134, 0.172; pairs_9x10_s12_relu_last 0.104, 0.124."""
    ref = go.reference(name)
    case = ref.case
    packed, occ = _bake(case)
    g, out = _gradient(case, ref.ups, packed, occ)
    assert bool(torch.isfinite(g).all())
    m = go.measure(g, ref.g64)
    _report(name, m, ref.bar)
    assert go.within(m, ref.bar)
    with torch.no_grad():                                   # the forward with autograd on: the bits of the plain launch
        plain = _render(case, packed, occ)
    assert all(p.grad_fn is None and torch.equal(p, o) for p, o in zip(plain, out))
    leaf = packed.clone().requires_grad_(True)
    with torch.no_grad():                                   # ... and no Function under no_grad, whatever the leaf asks for
        assert all(o.grad_fn is None for o in _render(case, leaf, occ))


@pytest.mark.parametrize("which", ["rgb", "depth", "opacity"])
@pytest.mark.parametrize("name", ["inside_16_s12_relu_last_white", "outside_16_s12_softplus_last"])
def test_each_output_alone(name, which):
    """The other two upstreams arrive as None and are passed as NULL: go's sign, the gd z_last term inside s_last.  Under softplus
    opacity is 1 whatever the nodes are (the last alpha is exactly 1), so its gradient is rounding on both sides and the bar, the
    fp32 reference's own error, says so (it is in the hundreds there): that one combination checks the plumbing only."""
    ref = go.reference(name, 1, (which,))
    g, _ = _gradient(ref.case, ref.ups)
    m = go.measure(g, ref.g64)
    _report(f"{name} / {which} alone", m, ref.bar)
    assert bool(torch.isfinite(g).all()) and go.within(m, ref.bar)
    if not (which == "opacity" and ref.case.clamp_mode == 'softplus'):
        assert float(g.abs().max()) > 1e-3
    if which != "rgb":                                      # dc = w G with G = 0: the colours receive exact zeros
        assert bool((g[..., :3] == 0).all())


# ------------------------------------------------------------------ exact zeros

blob_case = go.blob_case


def _own_reference(case, seed=0):
    near = vo.render(case, bars=True).near
    ups = go.upstreams(case, near, seed)
    g64 = go.autograd_gradient(case, ups)
    return SimpleNamespace(case=case, ups=ups, g64=g64, bar=go.bar_of(case, ups, g64), near=near)


def test_a_camera_that_misses_gives_exactly_zero():
    ref = go.reference("miss_5x7_s12_relu_white")
    for skip in (True, False):
        g, _ = _gradient(ref.case, ref.ups, skip=skip)
        assert bool((g == 0).all())


@pytest.mark.parametrize("inside_camera", [False, True], ids=["outside", "inside"])
def test_a_nonpositive_volume_without_last_back_gives_exactly_zero(inside_camera):
    for white_back in (False, True):
        ref = _own_reference(blob_case(True, inside_camera, white_back=white_back))
        for skip in (True, False):
            g, _ = _gradient(ref.case, ref.ups, skip=skip)
            assert bool((ref.g64 == 0).all()) and bool((g == 0).all())


def test_a_nonpositive_volume_with_last_back_moves_only_the_last_colours():
    ref = _own_reference(blob_case(True, True, last_back=True))
    assert int(ref.near.sum()) == 0 and go.last_sample_inside(ref.case, every=True)
    for skip in (True, False):
        g, _ = _gradient(ref.case, ref.ups, skip=skip)
        assert bool((g[..., 3] == 0).all()) and bool((ref.g64[..., 3] == 0).all())          # relu' = 0 at every sample
        m = go.measure(g, ref.g64)
        _report(f"nonpositive, last_back, skip={skip}", m, ref.bar)
        assert go.within(m, ref.bar) and float(g[..., :3].abs().max()) > 1e-3
        # non-zero only around the last samples: within one node of the yardstick's non-zero nodes (a last sample that fp32
        # puts into the neighbouring cell touches that cell's far nodes with a weight of rounding size), and few
        hit = (ref.g64[..., :3] != 0).any(-1).float().unsqueeze(1)
        around = F.max_pool3d(hit, 3, 1, 1)[:, 0] > 0
        got = (g[..., :3] != 0).any(-1)
        assert bool((got & ~around).sum() == 0)
        assert int(got.sum()) <= 8 * 2 * 16 * 16 and int(got.sum()) < got.numel() // 4


# ------------------------------------------------------------------ bricks

@pytest.mark.parametrize("last_back", [False, True])
def test_skip_changes_no_node_of_the_gradient(last_back):
    """4 x 3 x 2 bricks, Bv = 2.  With the skip on and off the same nodes are non-zero, exactly: a sample in an empty brick is
    not live either way (w = 0 and relu' = 0).  Their values agree within the bar and not bit for bit: the sums are fp32 atomic
    adds in arrival order, and skipping changes when every ray arrives."""
    ref = _own_reference(blob_case(False, last_back=last_back, white_back=True))
    packed, occ = _bake(ref.case)
    assert occ.shape == (2, 4, 3, 2) and int((occ > 0).sum()) == 6
    on, _ = _gradient(ref.case, ref.ups, packed, occ, skip=True)
    off, _ = _gradient(ref.case, ref.ups, packed, occ, skip=False)
    no_occ, _ = _gradient(ref.case, ref.ups, packed, None, skip=False)
    for what, g in (("skip on", on), ("skip off", off), ("no occ", no_occ)):
        m = go.measure(g, ref.g64)
        _report(f"bricks, last_back={last_back}, {what}", m, ref.bar)
        assert go.within(m, ref.bar)
    assert torch.equal(on != 0, off != 0) and torch.equal(off != 0, no_occ != 0)
    assert go.within(go.measure(on, off.double()), ref.bar)
    for v in range(2):                                                        # each volume is reached, and most of it is not
        assert float(on[v, ..., 3].abs().max()) > 0 and int((on[v] != 0).any(-1).sum()) < on[v, ..., 0].numel() // 2


# ------------------------------------------------------------------ volumes and cameras

def test_one_volume_under_three_cameras_sums_their_gradients():
    ref = go.reference("turntable_16_s12_relu")
    case = ref.case
    packed, occ = _bake(case)
    total, _ = _gradient(case, ref.ups, packed, occ)
    alone = []
    for i in range(3):
        ups_i = tuple(u[i:i + 1] for u in ref.ups)
        alone.append(_gradient(case, ups_i, packed, occ, cam2world=case.cam2world[i:i + 1])[0])
    m = go.measure(total, sum(a.double() for a in alone))
    _report("one volume, three cameras against the sum of each alone", m, ref.bar)
    assert go.within(m, ref.bar)
    assert all(float((alone[i] - alone[j]).abs().max()) > 1e-3 for i, j in ((0, 1), (1, 2)))       # the cameras do differ
    # three copies: copy i receives camera i's gradient and nothing else
    copies, _ = _gradient(case, ref.ups, packed.repeat(3, 1, 1, 1, 1), occ.repeat(3, 1, 1, 1))
    assert copies.shape[0] == 3
    for i in range(3):
        m = go.measure(copies[i:i + 1], alone[i].double())
        _report(f"copy {i} against camera {i} alone", m, ref.bar)
        assert go.within(m, ref.bar) and torch.equal(copies[i] != 0, alone[i][0] != 0)


def test_two_calls_agree():
    ref = go.reference("corner_16_s12_relu_last")
    packed, occ = _bake(ref.case)
    a, _ = _gradient(ref.case, ref.ups, packed, occ)
    b, _ = _gradient(ref.case, ref.ups, packed, occ)
    m = go.measure(a, b.double())
    _report("two calls", m, ref.bar)
    assert go.within(m, ref.bar) and torch.equal(a != 0, b != 0)


def test_both_shapes_of_the_atomic_adds_give_the_gradient(monkeypatch):
    """the scatter that bench_volume_backward.py measures against the default one: the same terms, another order"""
    from cips3d_amd import ops
    for name in ("pairs_9x10_s12_relu_last", "pairs_5x7_s12_softplus_last"):
        ref = go.reference(name)
        quad, _ = _gradient(ref.case, ref.ups)
        monkeypatch.setattr(ops, "VOLUME_SCATTER_PER_LANE", not ops.VOLUME_SCATTER_PER_LANE)
        other, _ = _gradient(ref.case, ref.ups)
        for what, g in (("default shape", quad), ("other shape", other)):
            m = go.measure(g, ref.g64)
            _report(f"{name}, {what}", m, ref.bar)
            assert go.within(m, ref.bar)
        assert torch.equal(quad != 0, other != 0)


# ------------------------------------------------------------------ occupancy

@pytest.mark.parametrize("Bv", [1, 3])
@pytest.mark.parametrize("shape", [(2, 2, 2), (5, 6, 7), (9, 17, 10), (18, 9, 9)], ids=lambda s: "x".join(map(str, s)))
def test_volume_occupancy_equals_bake(shape, Bv):
    from cips3d_amd import ops
    sigma, rgb = vo.random_volume(100 + Bv, Bv, *shape)
    packed, occ = ops.bake_volume(sigma.to(dev()), rgb.to(dev()))
    again = ops.volume_occupancy(packed)
    assert again.shape == occ.shape and again.dtype == occ.dtype and torch.equal(again, occ)
    assert torch.equal(ops.volume_occupancy(packed.clone().requires_grad_(True)), occ) and not again.requires_grad
    if shape[0] > 9:                                        # a maximum that sits only on a shared brick face
        moved = packed.clone()
        moved[..., 3] = -moved[..., 3].abs() - 1
        moved[:, 8, 3, 3, 3] = 5.0
        _, want = ops.bake_volume(moved[..., 3].contiguous(), moved[..., :3].contiguous())
        got = ops.volume_occupancy(moved)
        assert torch.equal(got, want) and bool((got[:, 0, 0, 0] == 5).all()) and bool((got[:, 1, 0, 0] == 5).all())


# ------------------------------------------------------------------ fitting

def _check_fit(fit, vol, before, steps, b):
    from cips3d_amd import ops
    assert fit.losses.shape == (steps, b) and fit.losses.is_cuda and bool(torch.isfinite(fit.losses).all())
    first, last = fit.losses[0].cpu(), fit.losses[-1].cpu()
    print("fit_volume: loss per image", [f"{float(a):.4e} -> {float(z):.4e} (x {float(z / a):.3f})" for a, z in zip(first, last)])
    assert bool((last < first).all())
    assert fit.rgbs.shape == vol.rgbs.shape and not fit.rgbs.requires_grad and bool(torch.isfinite(fit.rgbs).all())
    assert torch.equal(fit.occupancy, ops.volume_occupancy(fit.rgbs))
    assert fit.lo == vol.lo and fit.hi == vol.hi
    assert torch.equal(vol.rgbs, before) and not torch.equal(fit.rgbs, before)              # the input volume is not modified


def test_fit_volume_recovers_colours_on_a_synthetic_volume():
    from cips3d_amd import evaluation, ops
    case = blob_case(False)
    packed, occ = ops.bake_volume(case.sigma[:1].to(dev()), case.rgb[:1].to(dev()))
    truth = SimpleNamespace(rgbs=packed, occupancy=occ, lo=case.lo, hi=case.hi, resolution=None)
    cams = evaluation.orbit_cameras([0.8, 1.5, 2.2, 2.9], [1.2, 1.6, 1.9, 1.4], device=dev())
    FOV = 16
    targets = evaluation.render_volume(truth, cams, FOV, 16, 0.8, 1.2, 12).imgs
    assert float(targets.abs().max()) > 0.1
    start = packed.clone()
    start[..., :3] = 0
    vol = SimpleNamespace(rgbs=start, occupancy=occ, lo=case.lo, hi=case.hi, resolution=None)
    before = start.clone()
    fit = evaluation.fit_volume(vol, targets, cams, FOV, 0.8, 1.2, 12, steps=30, lr=0.05)
    _check_fit(fit, vol, before, 30, 4)
    assert fit.resolution is None
    # with the depth and the matte as further targets, and one volume per view
    out = evaluation.render_volume(truth, cams[:1], FOV, 16, 0.8, 1.2, 12, last_back=True)
    fit1 = evaluation.fit_volume(vol, out.imgs, cams[:1], FOV, 0.8, 1.2, 12, steps=5, lr=0.05, last_back=True,
                                 target_depth=out.depth, target_opacity=out.opacity, depth_weight=1., opacity_weight=1.,
                                 level_weights=(1., 0.5), kind="charbonnier")
    _check_fit(fit1, vol, before, 5, 1)


def _zs(seed, b):
    g = torch.Generator().manual_seed(seed)
    return {"z_nerf": torch.randn(b, 256, generator=g).to(dev()), "z_inr": torch.randn(b, 512, generator=g).to(dev())}


def test_fit_volume_to_the_generators_own_pictures(monkeypatch):
    from cips3d_amd import evaluation, ops
    N, L, FOV = 17, 0.3, 12
    G = seeded_generator(8, device=dev())
    zs = _zs(82, 1)
    yaws, pitches = [1.2, 1.6, 1.9], [1.45, 1.5, 1.7]
    with torch.no_grad():
        styles = G.styles(zs)
        targets = torch.cat(evaluation.render_views(G, styles, yaws, pitches, img_size=16, num_steps=12), 0).contiguous()
    assert targets.shape == (3, 3, 16, 16)
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    vol = G.bake(zs, resolution=N, cube_length=L)
    cams = evaluation.orbit_cameras(yaws, pitches, device=dev())
    before = vol.rgbs.clone()
    fit = evaluation.fit_volume(vol, targets, cams, FOV, 0.88, 1.12, 12, steps=30, lr=0.02)
    _check_fit(fit, vol, before, 30, 3)
    assert fit.resolution == N
    # render_volume(grad=True) carries a grad_fn where the nodes ask for one; the default never does
    leaf = SimpleNamespace(**{**vars(fit), "rgbs": fit.rgbs.clone().requires_grad_(True)})
    out = evaluation.render_volume(leaf, cams, FOV, 16, 0.88, 1.12, 12, grad=True)
    assert out.imgs.grad_fn is not None and out.depth.grad_fn is not None and out.opacity.grad_fn is not None
    plain = evaluation.render_volume(leaf, cams, FOV, 16, 0.88, 1.12, 12)
    assert plain.imgs.grad_fn is None and not plain.imgs.requires_grad and torch.equal(plain.imgs, out.imgs)
    assert evaluation.render_volume(fit, cams, FOV, 16, 0.88, 1.12, 12, grad=True).imgs.grad_fn is None       # nothing asks


def test_warp_view_of_two_volume_renders_reaches_the_nodes(monkeypatch):
    from cips3d_amd import evaluation, ops
    N, L, FOV = 17, 0.3, 12
    G = seeded_generator(8, device=dev())
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    vol = G.bake(_zs(82, 1), resolution=N, cube_length=L)
    cams = evaluation.orbit_cameras([1.2, 1.6, 1.9], [1.45, 1.5, 1.7], device=dev())
    leaf = SimpleNamespace(**{**vars(vol), "rgbs": vol.rgbs.clone().requires_grad_(True)})
    a = evaluation.render_volume(leaf, cams, FOV, 16, 0.88, 1.12, 12, last_back=True, grad=True)
    b = evaluation.render_volume(leaf, cams.roll(1, 0), FOV, 16, 0.88, 1.12, 12, last_back=True, grad=True)
    warped = evaluation.warp_view(a, b, FOV)
    assert int((warped.mask == 1).sum()) > 0
    loss = ((warped.imgs - b.imgs) ** 2 * (warped.mask == 1)).sum()
    g, = torch.autograd.grad(loss, leaf.rgbs)
    assert g.shape == vol.rgbs.shape and bool(torch.isfinite(g).all())
    assert float(g[..., :3].abs().max()) > 0 and float(g[..., 3].abs().max()) > 0
