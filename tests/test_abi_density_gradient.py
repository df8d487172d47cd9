"""CPU: the density-gradient entry points of the C-ABI (cips_siren_sigma_grad_x3, cips_siren_sigma_grad_x3_grid) are exported,
bound with the documented signatures and refuse malformed arguments before any HIP call; the Python entry points on top of them
refuse CPU tensors / a CPU module instead of falling back."""
import ctypes

import pytest
import torch

from conftest import seeded_generator

SYMBOLS = ("cips_siren_sigma_grad_x3", "cips_siren_sigma_grad_x3_grid")
INVALID = 1          # hipErrorInvalidValue


def test_density_gradient_symbols_are_exported_and_bound():
    from cips3d_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["cips_siren_sigma_grad_x3"] == (i32, [ctypes.POINTER(_lib.SirenWeights), vp, vp, vp, i32, i32, vp])
    assert _lib.SIGNATURES["cips_siren_sigma_grad_x3_grid"] == (i32, [ctypes.POINTER(_lib.SirenWeights),
                                                                       ctypes.POINTER(_lib.GridParams), vp, vp, i32, vp])
    assert lib.cips_version() == 9           # unchanged by this entry point; 9 came with cips_upfirdn2d_form


def test_density_gradient_entry_points_validate_arguments_before_touching_the_device():
    """every malformed call returns hipErrorInvalidValue with no device present: NULL w / points / grad / grid / coordinate
    arrays, non-positive sizes, and a lattice of more than INT_MAX points (sigma may be NULL: that is no error by itself, so
    every call below is malformed in another argument)"""
    from cips3d_amd import _lib
    lib = _lib.load()
    w = _lib.SirenWeights()
    buf = (ctypes.c_float * 8)()
    pv = ctypes.cast(buf, ctypes.c_void_p)
    wr = ctypes.byref(w)
    f = lib.cips_siren_sigma_grad_x3
    assert f(None, pv, pv, pv, 1, 1, None) == INVALID
    assert f(wr, None, pv, pv, 1, 1, None) == INVALID
    assert f(wr, pv, pv, None, 1, 1, None) == INVALID
    assert f(wr, pv, None, None, 1, 1, None) == INVALID
    assert f(wr, pv, pv, pv, 0, 1, None) == INVALID
    assert f(wr, pv, pv, pv, 1, 0, None) == INVALID
    assert f(wr, pv, None, pv, -1, 4, None) == INVALID
    assert f(wr, pv, None, pv, 4, -1, None) == INVALID

    def grid(gx=pv, gy=pv, gz=pv, nx=2, ny=2, nz=2):
        return ctypes.byref(_lib.GridParams(gx, gy, gz, nx, ny, nz))
    f = lib.cips_siren_sigma_grad_x3_grid
    assert f(None, grid(), pv, pv, 1, None) == INVALID
    assert f(wr, None, pv, pv, 1, None) == INVALID
    assert f(wr, grid(), pv, None, 1, None) == INVALID
    assert f(wr, grid(), pv, pv, 0, None) == INVALID
    assert f(wr, grid(), None, pv, -2, None) == INVALID
    for k in ("gx", "gy", "gz"):
        assert f(wr, grid(**{k: None}), pv, pv, 1, None) == INVALID, k
    for k in ("nx", "ny", "nz"):
        assert f(wr, grid(**{k: 0}), pv, pv, 1, None) == INVALID, k
        assert f(wr, grid(**{k: -3}), pv, pv, 1, None) == INVALID, k
    # 1291^3 = 2 151 685 171 > INT_MAX = 2 147 483 647 > 1290^3; and products that overflow 64 bits if taken at once
    assert f(wr, grid(nx=1291, ny=1291, nz=1291), pv, pv, 1, None) == INVALID
    assert f(wr, grid(nx=1 << 16, ny=1 << 16, nz=1), pv, pv, 1, None) == INVALID
    big = (1 << 31) - 1
    assert f(wr, grid(nx=big, ny=big, nz=big), None, pv, 1, None) == INVALID


def test_python_entry_points_refuse_the_cpu():
    from cips3d_amd import ops
    siren = [torch.zeros(2, 128) for _ in ops._SIREN_NAMES]
    with pytest.raises(RuntimeError, match="GPU"):
        ops.siren_sigma_grad(torch.zeros(2, 5, 3), *siren)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.siren_sigma_grad_grid(torch.zeros(3), torch.zeros(3), torch.zeros(3), *siren)
    G = seeded_generator(1)
    zs = {"z_nerf": torch.zeros(1, 256), "z_inr": torch.zeros(1, 512)}
    with pytest.raises(RuntimeError, match="GPU"):
        G.geometry(zs, img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=6, h_stddev=0.3, v_stddev=0.155,
                   hierarchical_sample=False, sample_dist="gaussian")
