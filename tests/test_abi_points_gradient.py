"""CPU: the point / camera gradient entry points of the C-ABI (cips_siren_bwd_points_x3, cips_siren_bwd_points_x3_rays,
cips_rays_bwd_cam) are exported, bound with the documented signatures and refuse malformed arguments before any HIP call;
SirenFunction with points that require grad refuses CPU tensors instead of falling back."""
import ctypes

import pytest
import torch

SYMBOLS = ("cips_siren_bwd_points_x3", "cips_siren_bwd_points_x3_rays", "cips_rays_bwd_cam")
INVALID = 1          # hipErrorInvalidValue


def test_points_gradient_symbols_are_exported_and_bound():
    from cips3d_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    W, R = ctypes.POINTER(_lib.SirenWeights), ctypes.POINTER(_lib.RayParams)
    assert _lib.SIGNATURES["cips_siren_bwd_points_x3"] == (i32, [W, vp, vp, vp, vp, i32, i32, vp])
    assert _lib.SIGNATURES["cips_siren_bwd_points_x3_rays"] == (i32, [W, R, vp, vp, vp, i32, vp])
    assert _lib.SIGNATURES["cips_rays_bwd_cam"] == (i32, [R, vp, vp, i32, vp])
    assert lib.cips_version() == 9           # adding symbols changes no signature


def _rays(_lib, pv, **kw):
    """a cips_ray_params fill_raygen accepts (4 x 4 pixels, 3 samples), with the fields of `kw` replaced"""
    f = dict(xg=pv, yg=pv, zg=pv, cam2world=pv, jitter=None, zvals=None, zc=-9.5, H=4, W=4, S=3)
    f.update(kw)
    r = _lib.RayParams()
    for k, v in f.items():
        setattr(r, k, v)
    return ctypes.byref(r)


# what fill_raygen refuses: a missing grid or matrix, no pixels, fewer than two samples per ray; and a point count past INT_MAX
BAD_RAYS = [dict(xg=None), dict(yg=None), dict(zg=None), dict(cam2world=None), dict(W=0), dict(H=0), dict(W=-4), dict(S=1),
            dict(S=0), dict(W=1 << 16, H=1 << 16, S=2), dict(W=46341, H=46341, S=2), dict(W=(1 << 31) - 1, H=(1 << 31) - 1, S=(1 << 31) - 1)]


def test_points_gradient_entry_points_validate_arguments_before_touching_the_device():
    """every malformed call returns hipErrorInvalidValue with no device present: each NULL pointer, B / P <= 0, and ray
    parameters that fill_raygen refuses or whose W * H * S does not fit an int"""
    from cips3d_amd import _lib
    lib = _lib.load()
    w = _lib.SirenWeights()
    buf = (ctypes.c_float * 64)()
    pv = ctypes.cast(buf, ctypes.c_void_p)
    wr = ctypes.byref(w)

    f = lib.cips_siren_bwd_points_x3
    good = [wr, pv, pv, pv, pv, 1, 1, None]
    for i in range(5):                                   # w, points, dfeat, dsigma, dpoints
        a = list(good)
        a[i] = None
        assert f(*a) == INVALID, i
    for B, P in ((0, 1), (1, 0), (-1, 4), (4, -1)):
        assert f(wr, pv, pv, pv, pv, B, P, None) == INVALID, (B, P)

    f = lib.cips_siren_bwd_points_x3_rays
    good = [wr, _rays(_lib, pv), pv, pv, pv, 1, None]
    for i in range(5):                                   # w, rays, dfeat, dsigma, dpoints
        a = list(good)
        a[i] = None
        assert f(*a) == INVALID, i
    for B in (0, -2):
        assert f(wr, _rays(_lib, pv), pv, pv, pv, B, None) == INVALID, B
    for kw in BAD_RAYS:
        assert f(wr, _rays(_lib, pv, **kw), pv, pv, pv, 1, None) == INVALID, kw

    f = lib.cips_rays_bwd_cam
    good = [_rays(_lib, pv), pv, pv, 1, None]
    for i in range(3):                                   # rays, dpoints, dcam2world
        a = list(good)
        a[i] = None
        assert f(*a) == INVALID, i
    for B in (0, -2):
        assert f(_rays(_lib, pv), pv, pv, B, None) == INVALID, B
    for kw in BAD_RAYS:
        assert f(_rays(_lib, pv, **kw), pv, pv, 1, None) == INVALID, kw


def test_siren_function_with_points_that_require_grad_refuses_the_cpu():
    from cips3d_amd import ops
    siren = [torch.zeros(2, 128, requires_grad=True) for _ in ops._SIREN_NAMES]
    with pytest.raises(RuntimeError, match="GPU"):
        ops.SirenFunction.apply(torch.zeros(2, 5, 3, requires_grad=True), *siren)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.siren_bwd_points({n: torch.zeros(2, 128) for n in ops._SIREN_NAMES}, torch.zeros(2, 5, 32), torch.zeros(2, 5), 2, 5,
                             points=torch.zeros(2, 5, 3))


def test_camera_setup_is_differentiable_only_when_asked():
    """camera_setup on the CPU (no kernels): under the caller's grad mode an explicit camera or a tensor mean that requires grad
    reaches cam2world; without one, or under no_grad, the result carries no graph — the GAN step's form"""
    import math
    from cips3d_amd.generator import RenderSettings, camera_setup
    kw = dict(img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=4, h_stddev=0.3, v_stddev=0.155,
              hierarchical_sample=False, sample_dist="gaussian")
    c = torch.tensor([[0.1, 0.2, 1.0], [-0.2, 0.1, 0.9]], requires_grad=True)
    look = torch.tensor([[-0.1, -0.2, -1.0], [0.2, -0.1, -0.9]], requires_grad=True)
    s = RenderSettings(**kw, h_mean=math.pi / 2, v_mean=math.pi / 2, camera_pos=c, camera_lookup=look)
    origin, c2w, _ = camera_setup(s, None, None, 2, "cpu")
    assert c2w.requires_grad and origin.requires_grad
    c2w.sum().backward()
    assert c.grad is not None and look.grad is not None and bool(torch.isfinite(c.grad).all()) and float(look.grad.abs().max()) > 0
    with torch.no_grad():
        assert not camera_setup(s, None, None, 2, "cpu")[1].requires_grad
    s0 = RenderSettings(**kw, h_mean=math.pi / 2, v_mean=math.pi / 2, camera_pos=c.detach(), camera_lookup=look.detach())
    assert not camera_setup(s0, None, None, 2, "cpu")[1].requires_grad
    hm, vm = torch.tensor(1.5, requires_grad=True), torch.tensor([[1.4], [1.6]], requires_grad=True)
    s = RenderSettings(**kw, h_mean=hm, v_mean=vm)
    c2w = camera_setup(s, torch.tensor([[0.3], [-0.2]]), torch.tensor([[0.1], [0.4]]), 2, "cpu")[1]
    c2w[:, :3].square().sum().backward()
    assert hm.grad.shape == () and vm.grad.shape == (2, 1) and float(hm.grad.abs()) > 0 and float(vm.grad.abs().min()) > 0
