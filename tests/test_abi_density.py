"""CPU: the density entry points of the C-ABI (cips_siren_sigma_x3, cips_siren_sigma_x3_grid) are exported, bound and refuse
malformed arguments before any HIP call, and evaluation.density_lattice builds the integer lattice that
GeneratorNerfINR.density_grid documents — not the sheared one of exp/pigan/scripts/extract_shapes.py."""
import ctypes
import os
import re

import torch

from conftest import ROOT

SYMBOLS = ("cips_siren_sigma_x3", "cips_siren_sigma_x3_grid")
INVALID = 1          # hipErrorInvalidValue


def test_density_symbols_are_exported_and_bound():
    from cips3d_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert _lib.SIGNATURES["cips_siren_sigma_x3"] == (ctypes.c_int, [ctypes.POINTER(_lib.SirenWeights), ctypes.c_void_p,
                                                                      ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p])
    assert _lib.SIGNATURES["cips_siren_sigma_x3_grid"] == (ctypes.c_int, [ctypes.POINTER(_lib.SirenWeights),
                                                                           ctypes.POINTER(_lib.GridParams), ctypes.c_void_p,
                                                                           ctypes.c_int, ctypes.c_void_p])
    assert lib.cips_version() == 9           # unchanged by this entry point; 9 came with cips_upfirdn2d_form


def test_grid_params_layout_matches_header_field_order():
    """the parsing of test_abi.py::test_struct_layouts_match_header_field_order, on cips_grid_params"""
    from cips3d_amd import _lib
    txt = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    body = txt[txt.index("typedef struct cips_grid_params"):]
    body = body[body.index("{") + 1:body.index("} cips_grid_params")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, types = [], []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        for part in stmt.split(","):
            fields.append(part.replace("*", " ").split()[-1])
            types.append(ctypes.c_void_p if "*" in stmt else ctypes.c_int)
    assert fields == ["gx", "gy", "gz", "nx", "ny", "nz"]
    assert fields == [f[0] for f in _lib.GridParams._fields_]
    assert types == [f[1] for f in _lib.GridParams._fields_]


def test_density_entry_points_validate_arguments_before_touching_the_device():
    """every malformed call returns hipErrorInvalidValue with no device present: NULL w / sigma / points / grid / coordinate
    arrays, non-positive sizes, and a lattice of more than INT_MAX points"""
    from cips3d_amd import _lib
    lib = _lib.load()
    w = _lib.SirenWeights()
    buf = (ctypes.c_float * 8)()
    pv = ctypes.cast(buf, ctypes.c_void_p)
    wr = ctypes.byref(w)
    assert lib.cips_siren_sigma_x3(None, pv, pv, 1, 1, None) == INVALID
    assert lib.cips_siren_sigma_x3(wr, None, pv, 1, 1, None) == INVALID
    assert lib.cips_siren_sigma_x3(wr, pv, None, 1, 1, None) == INVALID
    assert lib.cips_siren_sigma_x3(wr, pv, pv, 0, 1, None) == INVALID
    assert lib.cips_siren_sigma_x3(wr, pv, pv, 1, 0, None) == INVALID
    assert lib.cips_siren_sigma_x3(wr, pv, pv, -1, 4, None) == INVALID

    def grid(gx=pv, gy=pv, gz=pv, nx=2, ny=2, nz=2):
        return ctypes.byref(_lib.GridParams(gx, gy, gz, nx, ny, nz))
    assert lib.cips_siren_sigma_x3_grid(None, grid(), pv, 1, None) == INVALID
    assert lib.cips_siren_sigma_x3_grid(wr, None, pv, 1, None) == INVALID
    assert lib.cips_siren_sigma_x3_grid(wr, grid(), None, 1, None) == INVALID
    assert lib.cips_siren_sigma_x3_grid(wr, grid(), pv, 0, None) == INVALID
    for k in ("gx", "gy", "gz"):
        assert lib.cips_siren_sigma_x3_grid(wr, grid(**{k: None}), pv, 1, None) == INVALID, k
    for k in ("nx", "ny", "nz"):
        assert lib.cips_siren_sigma_x3_grid(wr, grid(**{k: 0}), pv, 1, None) == INVALID, k
        assert lib.cips_siren_sigma_x3_grid(wr, grid(**{k: -3}), pv, 1, None) == INVALID, k
    # 1291^3 = 2 151 685 171 > INT_MAX = 2 147 483 647 > 1290^3; and products that overflow 64 bits if taken at once
    assert lib.cips_siren_sigma_x3_grid(wr, grid(nx=1291, ny=1291, nz=1291), pv, 1, None) == INVALID
    assert lib.cips_siren_sigma_x3_grid(wr, grid(nx=1 << 16, ny=1 << 16, nz=1), pv, 1, None) == INVALID
    big = (1 << 31) - 1
    assert lib.cips_siren_sigma_x3_grid(wr, grid(nx=big, ny=big, nz=big), pv, 1, None) == INVALID


def test_density_lattice_end_points():
    """N = 2 is the cube's two faces: c - L/2 and c + L/2.  With dyadic L and c every step of the formula is exact in fp32, so
    the end points are hit exactly; for general values the upper one is the formula's single fp32 addition
    fl(fl(L) + fl(c - L/2)), at most one rounding (2^-24 relative) and the two operand roundings away from c + L/2."""
    from cips3d_amd.evaluation import density_lattice
    L, c = 0.5, (0.25, -0.125, 1.0)
    for a, g in enumerate(density_lattice(2, L, c)):
        assert g.dtype == torch.float32 and g.shape == (2,)
        assert g.tolist() == [c[a] - L / 2, c[a] + L / 2]
    L, c = 0.3, (0.01, -0.02, 0.03)
    for a, g in enumerate(density_lattice(2, L, c)):
        assert g[0].item() == torch.tensor(c[a] - L / 2, dtype=torch.float32).item()
        assert abs(g[1].item() - (c[a] + L / 2)) <= 3 * 2.0 ** -24 * (abs(c[a]) + L)


def test_density_lattice_is_the_integer_lattice_not_the_reference_construction():
    from cips3d_amd.evaluation import density_lattice
    N, L, c = 5, 0.3, (0.01, -0.02, 0.03)
    axes = density_lattice(N, L, c)
    assert len(axes) == 3
    idx = torch.arange(N, dtype=torch.float32)
    for a, g in enumerate(axes):
        assert torch.equal(g, (idx * (L / (N - 1))) + (c[a] - L / 2))
        d = g[1:] - g[:-1]
        # evenly spaced up to rounding: a difference of two coordinates carries four roundings (a product and a sum each) and
        # twice the rounding of the voxel size's own conversion, each at most 2^-24 of a magnitude below |c| + L
        assert (d.double() - L / (N - 1)).abs().max().item() <= 6 * 2.0 ** -24 * (abs(c[a]) + L)
    # the lattice as points, index p = (i * N + j) * N + k <-> (x_i, y_j, z_k)
    own = torch.stack([axes[0].view(N, 1, 1).expand(N, N, N), axes[1].view(1, N, 1).expand(N, N, N),
                       axes[2].view(1, 1, N).expand(N, N, N)], -1).reshape(-1, 3)
    # the construction of extract_shapes.py:18-31 (create_samples), from its formula: the slower indices are float
    # quotients that are never floored, so axis 1 gains k / N of a voxel and axis 0 (j + k / N) / N
    p = torch.arange(0, N ** 3, 1)
    origin = [v - L / 2 for v in c]
    voxel = L / (N - 1)
    ref = torch.zeros(N ** 3, 3)
    ref[:, 2] = p % N
    ref[:, 1] = (p.float() / N) % N
    ref[:, 0] = ((p.float() / N) / N) % N
    ref[:, 0] = ref[:, 0] * voxel + origin[2]
    ref[:, 1] = ref[:, 1] * voxel + origin[1]
    ref[:, 2] = ref[:, 2] * voxel + origin[0]
    assert not torch.equal(own[:, 1], ref[:, 1])
    # ... by up to (N - 1) / N of a voxel on that axis, where the integer lattice has the same y for all k
    shear = (ref[:, 1] - own[:, 1]).view(N, N, N)
    assert abs(shear.max().item() - voxel * (N - 1) / N) < 1e-6 and shear[:, :, 0].abs().max().item() < 1e-6
