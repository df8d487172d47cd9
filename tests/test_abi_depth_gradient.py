"""CPU: the entry points of the differentiable depth / opacity maps (cips_composite_fwd_geo, cips_march_fwd_x3_geo,
cips_composite_bwd_geo, cips_composite_bwd_live_geo, cips_composite_bwd_listed_geo) are exported, bound with the documented
signatures — the arguments of the entry point they extend, then opacity resp. ddepth and dopacity, then the stream — and refuse
malformed arguments before any HIP call; G.render refuses the partial / staged forms and a CPU module."""
import ctypes

import pytest
import torch

from conftest import seeded_generator

SYMBOLS = ("cips_composite_fwd_geo", "cips_march_fwd_x3_geo", "cips_composite_bwd_geo", "cips_composite_bwd_live_geo",
           "cips_composite_bwd_listed_geo")
INVALID = 1          # hipErrorInvalidValue


def test_depth_gradient_symbols_are_exported_and_bound():
    from cips3d_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    vp = ctypes.c_void_p
    for s in SYMBOLS:
        old = _lib.SIGNATURES[s[:-len("_geo")]]
        extra = 1 if "fwd" in s else 2
        assert _lib.SIGNATURES[s] == (old[0], old[1][:-1] + [vp] * extra + [vp]), s
    assert lib.cips_version() == 9           # adding symbols changes no signature


def _bad(f, good, required, what):
    for i in required:
        a = list(good)
        a[i] = None
        assert f(*a) == INVALID, (what, i)


def test_depth_gradient_entry_points_validate_arguments_before_touching_the_device():
    """every malformed call returns hipErrorInvalidValue with no device present: each NULL required pointer, R <= 0, S < 1, a
    fine set without all of its tensors, a live_f without a live_c"""
    from cips3d_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    pv = ctypes.cast(buf, ctypes.c_void_p)
    sizes = ((0, 3), (-2, 3), (4, 0), (4, -1))

    # feat_c sig_c z_c feat_f sig_f z_f noise std | fea depth weights order zsorted | R S clamp flags | pin rec | opacity stream
    f = lib.cips_composite_fwd_geo
    good = [pv, pv, pv, None, None, None, None, 0.0, pv, pv, pv, pv, pv, 4, 3, 0, 0, None, None, pv, None]
    _bad(f, good, (0, 1, 2, 8), "fwd")
    hier = list(good)
    hier[3:6] = [pv, pv, pv]
    _bad(f, hier, (4, 5), "fwd fine")
    for R, S in sizes:
        a = list(good)
        a[13:15] = [R, S]
        assert f(*a) == INVALID, (R, S)

    # ... noise std order | dfea dfeat_c dsig_c dfeat_f dsig_f | R S clamp flags pin | ddepth dopacity stream
    f = lib.cips_composite_bwd_geo
    good = [pv, pv, pv, None, None, None, None, 0.0, None, pv, pv, pv, None, None, 4, 3, 0, 0, None, pv, pv, None]
    _bad(f, good, (0, 1, 2, 9, 10, 11), "bwd")
    hier = list(good)
    hier[3:6] = [pv, pv, pv]
    hier[8] = pv
    hier[12:14] = [pv, pv]
    _bad(f, hier, (4, 5, 8, 12, 13), "bwd fine")
    for R, S in sizes:
        a = list(good)
        a[14:16] = [R, S]
        assert f(*a) == INVALID, (R, S)

    # ... dfeat_f dsig_f | live_c live_f | R S clamp flags pin | ddepth dopacity stream
    f = lib.cips_composite_bwd_live_geo
    good = [pv, pv, pv, None, None, None, None, 0.0, None, pv, pv, pv, None, None, pv, None, 4, 3, 0, 0, None, pv, pv, None]
    _bad(f, good, (0, 1, 2, 9, 10, 11), "live")
    a = list(good)
    a[14:16] = [None, pv]                                # a live_f without a live_c
    assert f(*a) == INVALID
    hier = list(good)
    hier[3:6] = [pv, pv, pv]
    hier[8] = pv
    hier[12:14] = [pv, pv]
    hier[15] = pv
    _bad(f, hier, (4, 5, 8, 12, 13, 15), "live fine")    # 15: with a fine set, a live_c without a live_f
    for R, S in sizes:
        a = list(good)
        a[16:18] = [R, S]
        assert f(*a) == INVALID, (R, S)

    # feat sigma z noise std | dfea dfeat dsigma | R S clamp flags | ddepth dopacity stream
    f = lib.cips_composite_bwd_listed_geo
    good = [pv, pv, pv, None, 0.0, pv, pv, pv, 4, 3, 0, 0, pv, pv, None]
    _bad(f, good, (0, 1, 2, 5, 6, 7), "listed")
    for R, S in sizes:
        a = list(good)
        a[8:10] = [R, S]
        assert f(*a) == INVALID, (R, S)

    # w rays noise std clamp flags | fea depth weights feat sigma z | B | pin rec | opacity stream
    f = lib.cips_march_fwd_x3_geo
    rays = _lib.RayParams()
    for k, v in dict(xg=pv, yg=pv, zg=pv, cam2world=pv, jitter=None, zvals=None, zc=-9.5, H=4, W=4, S=3).items():
        setattr(rays, k, v)
    wr, rr_ = ctypes.byref(_lib.SirenWeights()), ctypes.byref(rays)
    good = [wr, rr_, None, 0.0, 0, 0, pv, pv, None, None, None, None, 1, None, None, pv, None]
    _bad(f, good, (0, 1, 6), "march")
    for B in (0, -3):
        a = list(good)
        a[12] = B
        assert f(*a) == INVALID, B
    for kw in (dict(S=1), dict(S=0), dict(W=0), dict(xg=None), dict(cam2world=None)):
        bad = _lib.RayParams()
        for k in ("xg", "yg", "zg", "cam2world", "jitter", "zvals", "zc", "H", "W", "S"):
            setattr(bad, k, kw.get(k, getattr(rays, k)))
        a = list(good)
        a[1] = ctypes.byref(bad)
        assert f(*a) == INVALID, kw


KW = dict(img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=4, h_stddev=0.3, v_stddev=0.155, hierarchical_sample=False,
          sample_dist="gaussian")


def test_render_refuses_the_partial_and_staged_forms_and_the_cpu():
    G = seeded_generator(3)
    zs = {"z_nerf": torch.zeros(1, 256), "z_inr": torch.zeros(1, 512)}
    with pytest.raises(ValueError, match="grad_points"):
        G.render(zs, grad_points=16, **KW)
    with pytest.raises(ValueError, match="forward_points"):
        G.render(zs, forward_points=16, **KW)
    with pytest.raises(RuntimeError, match="GPU"):
        G.render(zs, **KW)


def test_geo_functions_refuse_cpu_tensors():
    from cips3d_amd import ops
    f, s, z = torch.zeros(4, 3, 32, requires_grad=True), torch.zeros(4, 3, requires_grad=True), torch.rand(4, 3).sort(-1).values
    with pytest.raises(RuntimeError, match="GPU"):
        ops.CompositeGeoFunction.apply(f, s, z, None, None, None, None, 0.0, 0, 0)
