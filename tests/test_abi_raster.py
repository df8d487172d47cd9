"""CPU: the C-ABI of the mesh rasteriser (csrc/raster.hip) and the refusals of ops.rasterize / ops.raster_interpolate — what can
be checked without a GPU.  Both entry points validate before any HIP call, so a malformed call returns hipErrorInvalidValue on a
machine that has no device."""
import ctypes as C

import pytest
import torch

INVALID = 1                      # hipErrorInvalidValue
SYMBOLS = ("cips_raster_fwd", "cips_raster_interp")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from cips3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbols_are_exported_and_bound_and_the_version_stays(lib):
    from cips3d_amd import _lib, build
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_longlong, C.c_float
    declared = {
        "cips_raster_fwd": [vp] * 5 + [f32] * 3 + [i32] + [vp] * 4 + [i64] + [vp] * 4 + [i32] * 5 + [vp],
        "cips_raster_interp": [vp] * 4 + [f32] + [vp] + [i32] * 6 + [vp],
    }
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert _lib.SIGNATURES[s] == (i32, declared[s])
        assert getattr(lib, s).argtypes == declared[s] and getattr(lib, s).restype == i32
    assert lib.cips_version() == 9
    assert "raster.hip" in build.SOURCES
    header = open(build.HERE + "/../include/cips3d_hip.h").read()
    assert "int cips_raster_fwd(" in header and "int cips_raster_interp(" in header


def _dummy():
    buf = (C.c_float * 64)()
    return buf, C.cast(buf, C.c_void_p)


FWD_POINTERS = ("vertices", "faces", "world2cam", "xg", "yg", "screen", "keys", "big_list", "big_count", "face", "bary", "depth", "mask")


def _fwd(lib, **over):
    """a well-formed call on host dummies (never dereferenced: every case here is refused first) with overrides"""
    buf, p = _dummy()
    a = dict({k: p for k in FWD_POINTERS}, zc=-9.5, near=1e-4, far=INF, cull=0, big_cap=None, B=2, V=5, T=7, H=4, W=6)
    a.update(over)
    if a["big_cap"] is None:
        a["big_cap"] = max(a["B"], 0) * max(a["T"], 0)
    return lib.cips_raster_fwd(a["vertices"], a["faces"], a["world2cam"], a["xg"], a["yg"], a["zc"], a["near"], a["far"], a["cull"],
                               a["screen"], a["keys"], a["big_list"], a["big_count"], a["big_cap"], a["face"], a["bary"], a["depth"],
                               a["mask"], a["B"], a["V"], a["T"], a["H"], a["W"], None)


INTERP_POINTERS = ("face", "bary", "faces", "attr", "out")


def _interp(lib, **over):
    buf, p = _dummy()
    a = dict({k: p for k in INTERP_POINTERS}, fill=0.0, B=2, H=4, W=6, T=7, V=5, C=3)
    a.update(over)
    return lib.cips_raster_interp(a["face"], a["bary"], a["faces"], a["attr"], a["fill"], a["out"], a["B"], a["H"], a["W"], a["T"],
                                  a["V"], a["C"], None)


IDS = dict(ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
FRAMES = [dict(H=1), dict(W=1), dict(H=0), dict(W=-3), dict(B=-1), dict(V=-1), dict(T=-2)]


@pytest.mark.parametrize("over", [{k: None} for k in FWD_POINTERS] + FRAMES + [
    dict(near=0.0), dict(near=-1e-3), dict(near=NAN), dict(near=INF), dict(zc=0.0), dict(zc=1.5), dict(zc=NAN), dict(zc=-INF),
    dict(far=NAN), dict(cull=2), dict(cull=-1), dict(big_cap=13),
    dict(B=4, H=1 << 15, W=1 << 15), dict(B=1 << 16, V=1 << 15, T=0), dict(B=1 << 16, V=1, T=1 << 15)], **IDS)
def test_malformed_raster_calls_are_refused_without_a_device(lib, over):
    assert _fwd(lib, **over) == INVALID


@pytest.mark.parametrize("over", [{k: None} for k in INTERP_POINTERS] + FRAMES + [
    dict(C=0), dict(C=-1), dict(B=4, H=1 << 15, W=1 << 15)], **IDS)
def test_malformed_interpolation_calls_are_refused_without_a_device(lib, over):
    assert _interp(lib, **over) == INVALID


def test_no_cameras_launch_nothing(lib):
    assert _fwd(lib, B=0) == 0 and _interp(lib, B=0) == 0              # no device here: a launch or a memset would not return 0


def test_rasterize_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import ops
    v, f, m = torch.zeros(5, 3), torch.zeros(7, 3, dtype=torch.int32), torch.eye(3, 4).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="GPU"):
        ops.rasterize(v, f, m, -9.5, 4, 6)
    for bad in [(v[:, :2], f, m), (v, f[:, :2], m), (v, f, m[0]), (v, f, m[:, :2]), (v.double(), f, m), (v, f.long(), m),
                (v, f, m.double()), (v.tolist(), f, m)]:
        with pytest.raises(ValueError, match="rasterize"):
            ops.rasterize(*bad, -9.5, 4, 6)
    for kw, what in [(dict(H=1), "H, W"), (dict(W=1), "H, W"), (dict(zc=0.0), "zc"), (dict(zc=2.0), "zc"), (dict(zc=NAN), "zc"),
                     (dict(near=0.0), "near"), (dict(near=INF), "near"), (dict(near=NAN), "near"), (dict(far=NAN), "far"),
                     (dict(cull="front"), "cull")]:
        a = dict(zc=-9.5, H=4, W=6)
        a.update(kw)
        with pytest.raises(ValueError, match=what):
            ops.rasterize(v, f, m, **a)
    with pytest.raises(ValueError, match="int32"):
        ops.rasterize(v, f, m, -9.5, 1 << 15, 1 << 15)


def test_raster_interpolate_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import ops
    face, bary = torch.zeros(2, 4, 6, dtype=torch.int32), torch.zeros(2, 4, 6, 3)
    f, attr = torch.zeros(7, 3, dtype=torch.int32), torch.zeros(5, 3)
    with pytest.raises(ValueError, match="GPU"):
        ops.raster_interpolate(face, bary, f, attr)
    for bad in [(face[0], bary, f, attr), (face, bary[..., :2], f, attr), (face, bary[:1], f, attr), (face, bary, f[:, :2], attr),
                (face, bary, f, attr[:, 0]), (face.long(), bary, f, attr), (face, bary.double(), f, attr), (face, bary, f, attr.double()),
                (face, bary, f, attr[:, :0])]:
        with pytest.raises(ValueError, match="raster_interpolate"):
            ops.raster_interpolate(*bad)


def test_world2cam_and_orbit_cameras_on_the_host():
    """plain torch: they run on a CPU device too"""
    import math
    from cips3d_amd import evaluation
    import raster_oracle as ro
    cams = evaluation.orbit_cameras([1.3, math.pi / 2, 0.4], [1.4, math.pi / 2, 2.0], device='cpu')
    assert cams.shape == (3, 4, 4) and cams.dtype == torch.float32
    w2c = evaluation.world2cam(cams)
    assert w2c.shape == (3, 3, 4) and w2c.dtype == torch.float32
    want = ro.orbit_world2cam([1.3, math.pi / 2, 0.4], [1.4, math.pi / 2, 2.0])
    assert float((w2c - want).abs().max()) <= 4e-7                     # fp32 angles and an fp32 cam2world against fp64
    eye = torch.cat([w2c, torch.tensor([0., 0., 0., 1.]).expand(3, 1, 4)], 1).double() @ cams.double()
    assert float((eye - torch.eye(4).double()).abs().max()) <= 4e-7
    shifted = evaluation.orbit_cameras([1.3], [1.4], radius=2.0, lookat=(0.1, -0.2, 0.3), device='cpu')
    assert float((shifted[0, :3, 3] - (2 * cams[0, :3, 3] + torch.tensor([0.1, -0.2, 0.3]))).abs().max()) <= 4e-7
    assert torch.equal(shifted[0, :3, :3], cams[0, :3, :3]) or float((shifted[0, :3, :3] - cams[0, :3, :3]).abs().max()) <= 4e-7
    with pytest.raises(ValueError, match="pitches"):
        evaluation.orbit_cameras([1.0, 2.0], [1.0], device='cpu')
    with pytest.raises(ValueError, match="world2cam"):
        evaluation.world2cam(torch.eye(4))
