"""CPU: the C-ABI of the view reprojection (csrc/reproject.hip) and the refusals of ops.reproject — what can be checked without
a GPU.  Both entry points validate before any HIP call, so a malformed call returns hipErrorInvalidValue on a machine that has
no device."""
import ctypes as C

import pytest
import torch

INVALID = 1                      # hipErrorInvalidValue
SYMBOLS = ("cips_reproject_fwd", "cips_reproject_bwd")


@pytest.fixture(scope="module")
def lib():
    from cips3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbols_are_exported_and_bound_and_the_version_stays(lib):
    from cips3d_amd import _lib, build
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    declared = {
        "cips_reproject_fwd": [vp] * 4 + [f32] * 3 + [vp] * 3 + [i32] * 6 + [vp],
        "cips_reproject_bwd": [vp] * 5 + [f32] * 2 + [vp] * 2 + [i32] * 6 + [vp],
    }
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert _lib.SIGNATURES[s] == (i32, declared[s])
        assert getattr(lib, s).argtypes == declared[s] and getattr(lib, s).restype == i32
    assert lib.cips_version() == 9
    assert "reproject.hip" in build.SOURCES
    header = open(build.HERE + "/../include/cips3d_hip.h").read()
    assert "int cips_reproject_fwd(" in header and "int cips_reproject_bwd(" in header


def _dummy():
    buf = (C.c_float * 64)()
    return buf, C.cast(buf, C.c_void_p)


def _fwd(lib, **over):
    """a well-formed forward call on host dummies (never dereferenced: every case here is refused first) with overrides"""
    buf, p = _dummy()
    a = dict(src=p, src_depth=None, tgt_depth=p, tgt2src=p, zc_tgt=-9.5, zc_src=-9.5, occ_tol=0.0, out=p, mask=p, uv=None,
             B=2, C=3, Hs=4, Ws=6, Ht=5, Wt=7)
    a.update(over)
    if a["src_depth"] is True:
        a["src_depth"] = p
    return lib.cips_reproject_fwd(a["src"], a["src_depth"], a["tgt_depth"], a["tgt2src"], a["zc_tgt"], a["zc_src"], a["occ_tol"],
                                  a["out"], a["mask"], a["uv"], a["B"], a["C"], a["Hs"], a["Ws"], a["Ht"], a["Wt"], None)


def _bwd(lib, **over):
    buf, p = _dummy()
    a = dict(dout=p, src=p, tgt_depth=p, tgt2src=p, mask=p, zc_tgt=-9.5, zc_src=-9.5, d_src=p, d_tgt_depth=p,
             B=2, C=3, Hs=4, Ws=6, Ht=5, Wt=7)
    a.update(over)
    return lib.cips_reproject_bwd(a["dout"], a["src"], a["tgt_depth"], a["tgt2src"], a["mask"], a["zc_tgt"], a["zc_src"],
                                  a["d_src"], a["d_tgt_depth"], a["B"], a["C"], a["Hs"], a["Ws"], a["Ht"], a["Wt"], None)


SHAPES = [dict(B=0), dict(B=-1), dict(C=0), dict(C=-2), dict(Hs=1), dict(Ws=1), dict(Ht=1), dict(Wt=1), dict(Hs=0), dict(Wt=-3)]
PLANES = [dict(zc_tgt=0.0), dict(zc_src=0.0), dict(zc_tgt=float("nan")), dict(zc_src=float("inf")), dict(zc_tgt=float("-inf")),
          dict(zc_src=float("nan"))]
IDS = dict(ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))


@pytest.mark.parametrize("over", [dict(src=None), dict(tgt_depth=None), dict(tgt2src=None), dict(out=None), dict(mask=None)] + SHAPES
                         + PLANES + [dict(src_depth=True, occ_tol=-1e-3), dict(src_depth=True, occ_tol=float("nan")),
                                     dict(src_depth=True, occ_tol=float("inf"))], **IDS)
def test_malformed_forward_calls_are_refused_without_a_device(lib, over):
    assert _fwd(lib, **over) == INVALID


@pytest.mark.parametrize("over", [dict(dout=None), dict(src=None), dict(tgt_depth=None), dict(tgt2src=None), dict(mask=None)] + SHAPES
                         + PLANES, **IDS)
def test_malformed_backward_calls_are_refused_without_a_device(lib, over):
    assert _bwd(lib, **over) == INVALID


def test_a_backward_with_nothing_to_write_launches_nothing(lib):
    assert _bwd(lib, d_src=None, d_tgt_depth=None) == 0          # no device here: a launch or a memset would not return 0


def test_reproject_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import ops
    src, depth, pose = torch.zeros(2, 3, 4, 6), torch.ones(2, 1, 5, 7), torch.eye(3, 4).repeat(2, 1, 1)
    with pytest.raises(ValueError, match="GPU"):
        ops.reproject(src, depth, pose, -9.5)
    for bad in [(src[0], depth, pose), (src[:, :, :1], depth, pose), (src, depth[:, 0], pose), (src, depth.expand(2, 2, 5, 7), pose),
                (src, depth[:, :, :, :1], pose), (src, depth[:1], pose), (src, depth, pose[:1]), (src, depth, torch.eye(4).repeat(2, 1, 1))]:
        with pytest.raises(ValueError, match="reproject"):
            ops.reproject(*bad, -9.5)
    with pytest.raises(ValueError, match="src_depth"):
        ops.reproject(src, depth, pose, -9.5, src_depth=torch.ones(2, 1, 5, 7), occ_tol=0.01)       # the target's shape
    with pytest.raises(ValueError, match="occ_tol"):
        ops.reproject(src, depth, pose, -9.5, src_depth=torch.ones(2, 1, 4, 6))
    with pytest.raises(ValueError, match="occ_tol"):
        ops.reproject(src, depth, pose, -9.5, src_depth=torch.ones(2, 1, 4, 6), occ_tol=-1.0)
    for zc in (0.0, float("nan")):
        with pytest.raises(ValueError, match="zc"):
            ops.reproject(src, depth, pose, zc)
        with pytest.raises(ValueError, match="zc"):
            ops.reproject(src, depth, pose, -9.5, zc_src=zc)
    with pytest.raises(ValueError, match="fp32"):
        ops.reproject(src.double(), depth, pose, -9.5)
