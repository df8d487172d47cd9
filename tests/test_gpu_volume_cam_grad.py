"""GPU: the gradient of the baked-volume renderer with respect to its cameras — cips_volume_render_bwd_cam through ctypes and
through ops.render_volume's autograd Function, evaluation.render_volume(grad=True) and evaluation.fit_cameras.

  oracle     against the fp64 yardstick tests/volume_cam_grad_oracle.py (torch autograd through volume_oracle.render with the
             camera as the leaf) on volume_grad_oracle's twelve cases and four two-blob volumes: per camera
             max|g - g64| / max|g64| over the 3 x 4 block within the bar, which is 8 x the same measure of fp32 torch autograd on
             that case (floor 16 * 2^-24) and comes from nothing the kernel computes.  Upstreams are zero on the pixels the oracle
             flags (a sample within rounding of a box face, of a cell face, or of sigma = 0 under relu).
             tests/test_volume_cam_grad_oracle_cpu.py shows that wrong rules leave the bar.
  exactness  what is exactly zero is exactly zero, and the kernel has no atomics, so what should be the same bits is compared
             bit for bit: two calls, the skip on and off, a camera alone and in a batch, ctypes and autograd.
  fit        fit_cameras lowers every view's loss and both angle errors and leaves the volume alone.

MEASURED on an MI355X (`pytest -s` prints every figure; profiles/volume_cam_grad.txt keeps those of the sixteen cases): the
kernel's error over its bar is 0.04 - 0.37 per camera on the cases that see the volume (errors 1.7e-7 ... 2.7e-5 against bars
9.5e-7 ... 2.9e-4; largest: blobs_16_s12_relu_white camera 0 at 0.371, corner_16_s12_relu_last at 0.340), 0.06 - 0.21 with one
output alone; the node gradient next to the camera's sits at 0.06 - 0.12 of volume_grad_oracle's bar.  fit_cameras: loss
1.5e-2 -> 8.3e-5 and 8.2e-3 -> 2.9e-4, yaw errors 0.1 -> 0.0045 and 0.0067, pitch errors 0.1 -> 0.0056 and 0.0057 (30 steps)."""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch

import volume_cam_grad_oracle as co
import volume_grad_oracle as go

pytestmark = pytest.mark.gpu
CASES = list(co.all_cases())


def dev():
    return torch.device("cuda")


def _bake(case):
    from cips3d_amd import ops
    return ops.bake_volume(case.sigma.to(dev()), case.rgb.to(dev()))


def _dcam(case, ups, packed, occ, skip=None, cam2world=None):
    """cips_volume_render_bwd_cam through ctypes -> dcam2world (b,4,4) on the CPU; the output starts as NaN: all 16 entries of
    every camera must be written"""
    from cips3d_amd import _lib, ops
    lib = _lib.load()
    cams = (case.cam2world if cam2world is None else cam2world).to(dev()).contiguous()
    b, (Bv, nx, ny, nz) = cams.shape[0], packed.shape[:4]
    skip = case.clamp_mode == 'relu' if skip is None else skip
    flags = (1 if case.last_back else 0) | (2 if case.white_back else 0) | (4 if skip else 0)
    xg, yg, _ = ops.pixel_grids(case.W, case.H, 2, 0., 1., dev())
    zg = case.zg.to(dev())
    lo_c, hi_c = (C.c_float * 3)(*case.lo), (C.c_float * 3)(*case.hi)
    d = [u.to(dev()).contiguous() if u is not None else None for u in ups]
    assert d[0] is not None
    out = torch.full((b, 4, 4), math.nan, device=dev())
    size = lib.cips_volume_render_bwd_cam_scratch(b, case.H, case.W, case.S)
    assert size > 0
    scratch = torch.empty(size // 4, device=dev())
    p = ops._p
    rc = lib.cips_volume_render_bwd_cam(p(packed), p(occ), lo_c, hi_c, p(xg), p(yg), p(zg), p(cams), case.zc,
                                        0 if case.clamp_mode == 'relu' else 1, flags, p(d[0]), p(d[1]), p(d[2]), p(out), p(scratch),
                                        b, Bv, nx, ny, nz, case.H, case.W, case.S, ops._stream())
    assert rc == 0
    return out.cpu()


def _render(case, packed, occ, cams, **over):
    from cips3d_amd import ops
    a = dict(clamp_mode=case.clamp_mode, last_back=case.last_back, white_back=case.white_back, skip=case.clamp_mode == 'relu')
    a.update(over)
    return ops.render_volume(packed, occ, case.lo, case.hi, cams, case.zc, case.H, case.W, zg=case.zg.to(dev()), **a)


def _backward(out, ups):
    used = [(o, u.to(dev())) for o, u in zip(out, ups) if u is not None]
    torch.autograd.backward([o for o, _ in used], [u for _, u in used])


def _report(what, m, bar):
    print(f"{what}: " + ", ".join(f"{a:.3e} (bar {b:.3e}, ratio {a / b:.3f})" for a, b in zip(m, bar)))


# ------------------------------------------------------------------ against the oracle

@pytest.mark.parametrize("name", CASES)
def test_kernel_against_the_oracle(name):
    ref = co.reference(name)
    packed, occ = _bake(ref.case)
    g = _dcam(ref.case, ref.ups, packed, occ)
    assert bool(torch.isfinite(g).all()) and bool((g[:, 3] == 0).all())
    m = co.measure(g, ref.g64)
    _report(name, m, ref.bar)
    assert co.within(m, ref.bar)


@pytest.mark.parametrize("which", ["rgb", "depth", "opacity"])
def test_each_output_alone(which):
    """ddepth and dopacity as NULL; alone they need a drgb of zeros (the entry point requires the pointer)"""
    ref = co.reference("inside_16_s12_relu_last_white", 1, (which,))
    packed, occ = _bake(ref.case)
    ups = ref.ups if which == "rgb" else (torch.zeros(1, 3, ref.case.H, ref.case.W),) + ref.ups[1:]
    g = _dcam(ref.case, ups, packed, occ)
    m = co.measure(g, ref.g64)
    _report(f"{which} alone", m, ref.bar)
    assert co.within(m, ref.bar) and float(g.abs().max()) > 1e-3


# ------------------------------------------------------------------ exact zeros

def test_what_is_zero_is_exactly_zero():
    for name in ("miss_5x7_s12_relu_white", "nonpositive_16_s12_relu_white"):
        ref = co.reference(name)
        packed, occ = _bake(ref.case)
        assert bool((ref.g64 == 0).all())
        for skip in (True, False):
            assert bool((_dcam(ref.case, ref.ups, packed, occ, skip=skip) == 0).all()), (name, skip)
    for name in ("turntable_16_s12_relu", "pairs_5x7_s12_softplus_last"):
        ref = co.reference(name)
        packed, occ = _bake(ref.case)
        zeros = tuple(torch.zeros_like(u) for u in ref.ups)
        assert bool((_dcam(ref.case, zeros, packed, occ) == 0).all()), name
        assert float(_dcam(ref.case, ref.ups, packed, occ).abs().max()) > 1.0


# ------------------------------------------------------------------ the same bits

def test_two_calls_give_the_same_bits():
    for name in ("corner_16_s12_relu_last", "pairs_5x7_s12_softplus_last"):
        ref = co.reference(name)
        packed, occ = _bake(ref.case)
        assert torch.equal(_dcam(ref.case, ref.ups, packed, occ), _dcam(ref.case, ref.ups, packed, occ))


@pytest.mark.parametrize("name", list(co.blob_cases()))
def test_skip_on_and_off_give_the_same_bits(name):
    """4 x 3 x 2 bricks, Bv = 2: a skipped sample and a fetched sample that is not live both add nothing"""
    ref = co.reference(name)
    packed, occ = _bake(ref.case)
    assert occ.shape == (2, 4, 3, 2) and int((occ > 0).sum()) in (0, 6)
    on = _dcam(ref.case, ref.ups, packed, occ, skip=True)
    assert torch.equal(on, _dcam(ref.case, ref.ups, packed, occ, skip=False))
    assert torch.equal(on, _dcam(ref.case, ref.ups, packed, None, skip=False))


def test_a_camera_in_a_batch_has_the_bits_of_that_camera_alone():
    """Bv = 1 under three cameras of 16 x 16, and under two of 9 x 10 (partial tiles, the second image behind the first)"""
    for name in ("turntable_16_s12_relu", "pairs_9x10_s12_relu_last"):
        ref = co.reference(name)
        case = ref.case
        packed, occ = _bake(case)
        batch = _dcam(case, ref.ups, packed, occ)
        for i in range(case.cam2world.shape[0]):
            alone = _dcam(case, tuple(u[i:i + 1] for u in ref.ups), packed, occ, cam2world=case.cam2world[i:i + 1])
            assert torch.equal(batch[i:i + 1], alone) and float(alone.abs().max()) > 1.0, (name, i)
    # one volume per camera, 5 x 7 pixels: camera 1 with volume 1 alone
    ref = co.reference("pairs_5x7_s12_softplus_last")
    packed, occ = _bake(ref.case)
    batch = _dcam(ref.case, ref.ups, packed, occ)
    alone = _dcam(ref.case, tuple(u[1:2] for u in ref.ups), packed[1:2].contiguous(), occ[1:2].contiguous(),
                  cam2world=ref.case.cam2world[1:2])
    assert torch.equal(batch[1:2], alone)


# ------------------------------------------------------------------ autograd

@pytest.mark.parametrize("name", ["pairs_9x10_s12_relu_last", "outside_16_s12_softplus_last", "blobs_16_s12_relu_white"])
def test_autograd_carries_the_kernels_bits(name):
    ref = co.reference(name)
    case = ref.case
    packed, occ = _bake(case)
    want = _dcam(case, ref.ups, packed, occ)
    with torch.no_grad():
        plain = _render(case, packed, occ, case.cam2world.to(dev()))
    # the camera alone
    cams = case.cam2world.to(dev()).requires_grad_(True)
    out = _render(case, packed, occ, cams)
    assert all(o.grad_fn is not None and torch.equal(o, p) for o, p in zip(out, plain))
    _backward(out, ref.ups)
    assert cams.grad.shape == (cams.shape[0], 4, 4) and torch.equal(cams.grad.cpu(), want)
    # the camera and the nodes: the camera's bits do not move, the nodes' gradient is within volume_grad_oracle's bar
    cams2, leaf = case.cam2world.to(dev()).requires_grad_(True), packed.clone().requires_grad_(True)
    _backward(_render(case, leaf, occ, cams2), ref.ups)
    assert torch.equal(cams2.grad.cpu(), want)
    n64 = go.autograd_gradient(case, ref.ups)
    bar, m = go.bar_of(case, ref.ups, n64), go.measure(leaf.grad.cpu(), n64)
    print(f"{name}: nodes next to the camera: sigma {m[0]:.3e} (bar {bar[0]:.3e}), colour {m[1]:.3e} (bar {bar[1]:.3e})")
    assert go.within(m, bar)
    # the nodes alone: nothing for the camera
    cams3, leaf3 = case.cam2world.to(dev()), packed.clone().requires_grad_(True)
    _backward(_render(case, leaf3, occ, cams3), ref.ups)
    assert cams3.grad is None and leaf3.grad is not None and go.within(go.measure(leaf3.grad.cpu(), n64), bar)
    # nothing asks: the plain launch; and no Function under no_grad, whatever the camera asks for
    nothing = _render(case, packed, occ, case.cam2world.to(dev()))
    assert all(o.grad_fn is None and not o.requires_grad and torch.equal(o, p) for o, p in zip(nothing, plain))
    with torch.no_grad():
        assert all(o.grad_fn is None for o in _render(case, packed, occ, cams))


def _two_blobs():
    from cips3d_amd import ops
    case = go.blob_case(False)
    packed, occ = ops.bake_volume(case.sigma.to(dev()), case.rgb.to(dev()))
    return case, SimpleNamespace(rgbs=packed, occupancy=occ, lo=case.lo, hi=case.hi, resolution=None)


def test_evaluation_render_volume_reaches_leaf_angles():
    from cips3d_amd import evaluation
    from cips3d_amd.generator import _normalize, camera_origin_from_angles, create_cam2world_matrix
    case, vol = _two_blobs()
    yaw = torch.tensor([[0.8], [2.2]], device=dev(), requires_grad=True)
    pitch = torch.tensor([[1.2], [1.9]], device=dev(), requires_grad=True)
    offset, _ = camera_origin_from_angles(yaw, pitch, 1.0)
    cams = create_cam2world_matrix(_normalize(-offset), offset)
    assert torch.equal(cams.detach(), evaluation.orbit_cameras([0.8, 2.2], [1.2, 1.9], device=dev()))
    out = evaluation.render_volume(vol, cams, 16, 16, 0.8, 1.2, 12, grad=True)
    assert out.imgs.grad_fn is not None and out.depth.grad_fn is not None and out.opacity.grad_fn is not None
    (out.imgs.square().sum() + out.depth.sum() + out.opacity.sum()).backward()
    for leaf in (yaw, pitch):
        assert leaf.grad is not None and bool(torch.isfinite(leaf.grad).all()) and bool((leaf.grad != 0).all())
    plain = evaluation.render_volume(vol, cams, 16, 16, 0.8, 1.2, 12)
    assert plain.imgs.grad_fn is None and torch.equal(plain.imgs, out.imgs)


# ------------------------------------------------------------------ fitting

def test_fit_cameras_moves_towards_the_true_angles():
    """The two-blob volumes, one per view, 16 x 16, S = 12; the start is 0.1 rad off in yaw and in pitch."""
    from cips3d_amd import evaluation
    case, vol = _two_blobs()
    true_yaw, true_pitch = [0.8, 2.2], [1.2, 1.9]
    FOV, steps = 16, 30
    targets = evaluation.render_volume(vol, evaluation.orbit_cameras(true_yaw, true_pitch, device=dev()), FOV, 16, 0.8, 1.2, 12).imgs
    assert float(targets.abs().max()) > 0.1
    before = vol.rgbs.clone()
    y0, p0 = [y - 0.1 for y in true_yaw], [p + 0.1 for p in true_pitch]
    fit = evaluation.fit_cameras(vol, targets, FOV, 0.8, 1.2, 12, yaws=y0, pitches=p0, steps=steps, lr=0.01)
    assert fit.losses.shape == (steps, 2) and fit.losses.is_cuda and bool(torch.isfinite(fit.losses).all())
    first, last = fit.losses[0].cpu(), fit.losses[-1].cpu()
    yaw_err = (fit.yaws.cpu() - torch.tensor(true_yaw)).abs()
    pitch_err = (fit.pitches.cpu() - torch.tensor(true_pitch)).abs()
    print("fit_cameras: loss per view", [f"{float(a):.3e} -> {float(z):.3e}" for a, z in zip(first, last)],
          "yaw error", yaw_err.tolist(), "pitch error", pitch_err.tolist())
    assert bool((last < first).all())
    assert bool((yaw_err < 0.1).all()) and bool((pitch_err < 0.1).all())
    assert torch.equal(vol.rgbs, before) and not vol.rgbs.requires_grad
    assert fit.yaws.shape == (2,) and fit.pitches.shape == (2,) and not fit.yaws.requires_grad
    assert torch.equal(fit.radius.cpu(), torch.ones(2))
    assert torch.equal(fit.cam2world, evaluation.orbit_cameras(fit.yaws.tolist(), fit.pitches.tolist(), device=dev()))
    # the first iterate is orbit_cameras' camera: one step's first loss is the loss of that render
    one = evaluation.fit_cameras(vol, targets, FOV, 0.8, 1.2, 12, yaws=y0, pitches=p0, steps=1, lr=0.01, fit_radius=True)
    from cips3d_amd import ops
    start = evaluation.render_volume(vol, evaluation.orbit_cameras(y0, p0, device=dev()), FOV, 16, 0.8, 1.2, 12).imgs
    assert torch.equal(one.losses[0], ops.pyramid_loss(start, targets)) and torch.equal(one.losses[0], fit.losses[0])
    assert bool((one.radius != 1).all())
