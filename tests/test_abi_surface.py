"""CPU: the surface ray-cast entry point of the C-ABI (cips_siren_surface_x3) is exported, bound with the documented signature
and refuses malformed arguments before any HIP call; the Python wrappers refuse CPU tensors instead of falling back."""
import ctypes

import pytest
import torch

INVALID = 1          # hipErrorInvalidValue


def test_surface_symbol_is_exported_and_bound():
    from cips3d_amd import _lib
    lib = _lib.load()
    assert "cips_siren_surface_x3" in _lib.SIGNATURES and hasattr(lib, "cips_siren_surface_x3")
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    W, R = ctypes.POINTER(_lib.SirenWeights), ctypes.POINTER(_lib.RayParams)
    # (w, rays, level, refine, depth, hit, sigma, points, trace, B, stream)
    assert _lib.SIGNATURES["cips_siren_surface_x3"] == (i32, [W, R, f32, i32, vp, vp, vp, vp, vp, i32, vp])
    assert lib.cips_version() == 9           # adding symbols changes no signature


def _rays(_lib, pv, **kw):
    """a cips_ray_params the entry point accepts (4 x 4 pixels, 3 samples, no jitter, no zvals), with the fields of `kw` replaced"""
    f = dict(xg=pv, yg=pv, zg=pv, cam2world=pv, jitter=None, zvals=None, zc=-9.5, H=4, W=4, S=3)
    f.update(kw)
    r = _lib.RayParams()
    for k, v in f.items():
        setattr(r, k, v)
    return ctypes.byref(r)


def test_surface_entry_point_validates_arguments_before_touching_the_device():
    """every malformed call returns hipErrorInvalidValue with no device present: NULL w / rays / depth / hit, NULL grids or
    camera, a jitter or zvals pointer (the walk is on the unjittered grid), S <= 1, no pixels, H * W past INT_MAX, B <= 0 or
    past the grid's 65535, refine outside 0..32"""
    from cips3d_amd import _lib
    lib = _lib.load()
    w = _lib.SirenWeights()
    buf = (ctypes.c_float * 64)()
    pv = ctypes.cast(buf, ctypes.c_void_p)
    wr = ctypes.byref(w)
    f = lib.cips_siren_surface_x3
    good = [wr, _rays(_lib, pv), 1.0, 4, pv, pv, pv, pv, pv, 1, None]
    for i in (0, 1, 4, 5):                               # w, rays, depth, hit
        a = list(good)
        a[i] = None
        assert f(*a) == INVALID, i
    for kw in (dict(xg=None), dict(yg=None), dict(zg=None), dict(cam2world=None), dict(jitter=pv), dict(zvals=pv), dict(S=1),
               dict(S=0), dict(S=-3), dict(W=0), dict(H=0), dict(W=-4), dict(W=1 << 16, H=1 << 16),
               dict(W=(1 << 31) - 1, H=(1 << 31) - 1)):
        a = list(good)
        a[1] = _rays(_lib, pv, **kw)
        assert f(*a) == INVALID, kw
    for B in (0, -1, 65536):
        a = list(good)
        a[9] = B
        assert f(*a) == INVALID, B
    for refine in (-1, 33, 1 << 20):
        a = list(good)
        a[3] = refine
        assert f(*a) == INVALID, refine
    # NULL sigma / points / trace are allowed: with everything else malformed in one more way the answer is still INVALID,
    # never a launch
    a = list(good)
    a[6] = a[7] = a[8] = None
    a[9] = 0
    assert f(*a) == INVALID


def test_surface_wrappers_refuse_the_cpu():
    from cips3d_amd import ops
    from cips3d_amd.generator import GeneratorNerfINR
    from conftest import G_CFG
    siren = [torch.zeros(2, 128) for _ in ops._SIREN_NAMES]
    xg = yg = torch.linspace(-1, 1, 4)
    zg = torch.linspace(0.88, 1.12, 3)
    c2w = torch.eye(4).expand(2, 4, 4).contiguous()
    with pytest.raises(RuntimeError, match="GPU"):
        ops.siren_surface(0.5, 4, (2, 4, 4, 3, -9.5), xg, yg, zg, c2w, *siren)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.siren_surface_composed(0.5, 4, (2, 4, 4, 3, -9.5), xg, yg, zg, c2w, *siren)
    G = GeneratorNerfINR(**G_CFG, device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        G.surface({"z_nerf": torch.zeros(1, 256)}, 0.5, img_size=4, fov=12, ray_start=0.88, ray_end=1.12, num_steps=3,
                  h_stddev=0.3, v_stddev=0.155, sample_dist="gaussian")
