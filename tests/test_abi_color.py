"""CPU: the point-colour entry points of the C-ABI (cips_siren_rgb_x3, cips_siren_rgb_x3_grid) are declared, exported, bound with
the declared argument types, built from a source of their own, and refuse malformed arguments before any HIP call with the
return code of the sigma entry points (tests/test_abi_density.py)."""
import ctypes
import os

from conftest import ROOT

SYMBOLS = ("cips_siren_rgb_x3", "cips_siren_rgb_x3_grid")
INVALID = 1          # hipErrorInvalidValue


def test_color_symbols_are_declared_exported_and_bound():
    from cips3d_amd import _lib, build
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
        assert f"int {s}(" in header, s
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    # (w, points, proj_w, proj_b, tanh_out, rgb, sigma, B, P, stream)
    assert _lib.SIGNATURES["cips_siren_rgb_x3"] == (i32, [ctypes.POINTER(_lib.SirenWeights), vp, vp, vp, i32, vp, vp, i32, i32, vp])
    # (w, grid, proj_w, proj_b, tanh_out, rgb, sigma, B, stream)
    assert _lib.SIGNATURES["cips_siren_rgb_x3_grid"] == (i32, [ctypes.POINTER(_lib.SirenWeights), ctypes.POINTER(_lib.GridParams),
                                                                vp, vp, i32, vp, vp, i32, vp])
    assert lib.cips_version() == 9           # unchanged: the projection is an argument, cips_siren_weights is as it was
    assert "siren_color_x3.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "cips3d_amd", "csrc", "siren_color_x3.hip"))


def test_the_kernels_are_not_in_the_forward_module():
    """the forward module's kernel order hides a defect of the sigma kernel (its header comment): nothing was added to it"""
    csrc = os.path.join(ROOT, "cips3d_amd", "csrc")
    for name in ("siren_fwd_x3.hip", "siren_sigma_x3.inc", "siren_fwd_chain.inc"):
        assert "siren_color" not in open(os.path.join(csrc, name)).read() and "rgb_x3" not in open(os.path.join(csrc, name)).read()
    assert '#include "siren_fwd_chain.inc"' in open(os.path.join(csrc, "siren_color_x3.hip")).read()


def test_color_entry_points_validate_arguments_before_touching_the_device():
    """every malformed call returns hipErrorInvalidValue with no device present: NULL w / points / projection / rgb / grid /
    coordinate arrays, non-positive sizes, a batch beyond the launch grid's second dimension, and a lattice of more than
    INT_MAX points; a NULL sigma is not an error (it is optional), so it is NULL in every call here"""
    from cips3d_amd import _lib
    lib = _lib.load()
    w = _lib.SirenWeights()
    buf = (ctypes.c_float * 128)()
    pv = ctypes.cast(buf, ctypes.c_void_p)
    wr = ctypes.byref(w)
    f = lib.cips_siren_rgb_x3
    assert f(None, pv, pv, pv, 1, pv, None, 1, 1, None) == INVALID
    assert f(wr, None, pv, pv, 1, pv, None, 1, 1, None) == INVALID
    assert f(wr, pv, None, pv, 1, pv, None, 1, 1, None) == INVALID
    assert f(wr, pv, pv, None, 1, pv, None, 1, 1, None) == INVALID
    assert f(wr, pv, pv, pv, 1, None, None, 1, 1, None) == INVALID
    assert f(wr, pv, pv, pv, 1, pv, None, 0, 1, None) == INVALID
    assert f(wr, pv, pv, pv, 1, pv, None, 1, 0, None) == INVALID
    assert f(wr, pv, pv, pv, 1, pv, None, -1, 4, None) == INVALID
    assert f(wr, pv, pv, pv, 1, pv, None, 65536, 4, None) == INVALID

    def grid(gx=pv, gy=pv, gz=pv, nx=2, ny=2, nz=2):
        return ctypes.byref(_lib.GridParams(gx, gy, gz, nx, ny, nz))
    g = lib.cips_siren_rgb_x3_grid
    assert g(None, grid(), pv, pv, 1, pv, None, 1, None) == INVALID
    assert g(wr, None, pv, pv, 1, pv, None, 1, None) == INVALID
    assert g(wr, grid(), None, pv, 1, pv, None, 1, None) == INVALID
    assert g(wr, grid(), pv, None, 1, pv, None, 1, None) == INVALID
    assert g(wr, grid(), pv, pv, 1, None, None, 1, None) == INVALID
    assert g(wr, grid(), pv, pv, 1, pv, None, 0, None) == INVALID
    assert g(wr, grid(), pv, pv, 1, pv, None, 65536, None) == INVALID
    for k in ("gx", "gy", "gz"):
        assert g(wr, grid(**{k: None}), pv, pv, 1, pv, None, 1, None) == INVALID, k
    for k in ("nx", "ny", "nz"):
        assert g(wr, grid(**{k: 0}), pv, pv, 1, pv, None, 1, None) == INVALID, k
        assert g(wr, grid(**{k: -3}), pv, pv, 1, pv, None, 1, None) == INVALID, k
    # 1291^3 > INT_MAX > 1290^3; and products that overflow 64 bits if taken at once
    assert g(wr, grid(nx=1291, ny=1291, nz=1291), pv, pv, 1, pv, None, 1, None) == INVALID
    assert g(wr, grid(nx=1 << 16, ny=1 << 16, nz=1), pv, pv, 1, pv, None, 1, None) == INVALID
    big = (1 << 31) - 1
    assert g(wr, grid(nx=big, ny=big, nz=big), pv, pv, 1, pv, None, 1, None) == INVALID
