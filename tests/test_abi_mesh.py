"""CPU: the mesh entry points of the C-ABI (cips_mesh_scratch_bytes, cips_mesh_count, cips_mesh_emit) are exported, bound and
refuse malformed arguments before any HIP call; the scratch stays within 8 bytes per lattice point and image."""
import ctypes

SYMBOLS = ("cips_mesh_scratch_bytes", "cips_mesh_count", "cips_mesh_emit")
INVALID = 1          # hipErrorInvalidValue
INT_MAX = (1 << 31) - 1


def test_mesh_symbols_are_exported_and_bound():
    from cips3d_amd import _lib
    lib = _lib.load()
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    grid = ctypes.POINTER(_lib.GridParams)
    assert _lib.SIGNATURES["cips_mesh_scratch_bytes"] == (i64, [grid, i32])
    assert _lib.SIGNATURES["cips_mesh_count"] == (i32, [grid, vp, f32, i32, vp, i64, vp, vp])
    assert _lib.SIGNATURES["cips_mesh_emit"] == (i32, [grid, vp, f32, i32, vp, i64, vp, vp, vp, vp])
    assert lib.cips_version() == 9           # adding symbols changes no signature


def _grid(pv, gx=True, gy=True, gz=True, nx=2, ny=2, nz=2):
    from cips3d_amd import _lib
    return ctypes.byref(_lib.GridParams(pv if gx else None, pv if gy else None, pv if gz else None, nx, ny, nz))


def test_scratch_size_is_reported_on_the_host_and_within_8_bytes_per_point():
    from cips3d_amd import _lib
    lib = _lib.load()
    for (nx, ny, nz), B in [((2, 2, 2), 1), ((2, 2, 2), 3), ((5, 3, 7), 2), ((17, 17, 17), 1), ((9, 9, 300), 1), ((256, 256, 256), 4),
                            ((2, 2, 3), 1), ((513, 2, 2), 5)]:
        n = lib.cips_mesh_scratch_bytes(_grid(None, nx=nx, ny=ny, nz=nz), B)       # reads the sizes only
        assert 5 * B * nx * ny * nz <= n <= 8 * B * nx * ny * nz, (nx, ny, nz, B, n)     # a 4-byte id and a mask byte per point
    assert lib.cips_mesh_scratch_bytes(None, 1) == -1
    assert lib.cips_mesh_scratch_bytes(_grid(None), 0) == -1
    assert lib.cips_mesh_scratch_bytes(_grid(None), -2) == -1
    for k in ("nx", "ny", "nz"):
        for bad in (1, 0, -3):
            assert lib.cips_mesh_scratch_bytes(_grid(None, **{k: bad}), 1) == -1, (k, bad)


def test_lattice_size_limits():
    """7 nx ny nz <= INT_MAX (vertex ids) and 12 (nx-1)(ny-1)(nz-1) <= INT_MAX (triangle ids), from either side"""
    from cips3d_amd import _lib
    lib = _lib.load()
    size = lambda nx, ny, nz: lib.cips_mesh_scratch_bytes(_grid(None, nx=nx, ny=ny, nz=nz), 1)
    # 7 * 2 * 2 * n: n = 76 695 844 gives 2 147 483 632 <= INT_MAX, one more does not fit
    n = INT_MAX // 28
    assert 7 * 4 * n <= INT_MAX < 7 * 4 * (n + 1)
    assert size(2, 2, n) > 0 and size(2, 2, n + 1) == -1 and size(n + 1, 2, 2) == -1 and size(2, n + 1, 2) == -1
    # the cube: 563^3 = 178 453 547 cells * 12 = 2 141 442 564 fits, and so do its 564^3 * 7 = 1 255 873 008 vertex ids;
    # 564^3 cells * 12 = 2 152 893 728 does not
    assert 12 * 563 ** 3 <= INT_MAX < 12 * 564 ** 3 and 7 * 565 ** 3 <= INT_MAX
    assert size(564, 564, 564) > 0 and size(565, 565, 565) == -1
    # products that overflow 64 bits if taken at once
    big = INT_MAX
    assert size(big, big, big) == -1 and size(1 << 16, 1 << 16, 2) == -1


def test_mesh_entry_points_validate_arguments_before_touching_the_device():
    """every malformed call returns hipErrorInvalidValue with no device present: NULL grid / coordinate arrays / sigma /
    scratch / totals / outputs, sizes below 2 per axis, a non-positive or too large B, lattices beyond the 32-bit limits, a
    scratch that is too small or misaligned"""
    from cips3d_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    pv = ctypes.cast(buf, ctypes.c_void_p)
    need = lib.cips_mesh_scratch_bytes(_grid(pv), 1)
    assert 0 < need <= 64

    def count(grid=None, sigma=pv, B=1, scratch=pv, nbytes=need, totals=pv):
        return lib.cips_mesh_count(grid if grid is not None else _grid(pv), sigma, 0.5, B, scratch, nbytes, totals, None)

    def emit(grid=None, sigma=pv, B=1, scratch=pv, nbytes=need, totals=pv, vertices=pv, faces=pv):
        return lib.cips_mesh_emit(grid if grid is not None else _grid(pv), sigma, 0.5, B, scratch, nbytes, totals, vertices, faces, None)

    for call in (count, emit):
        assert lib.cips_mesh_count(None, pv, 0.5, 1, pv, need, pv, None) == INVALID
        assert call(sigma=None) == INVALID
        assert call(scratch=None) == INVALID
        assert call(totals=None) == INVALID
        assert call(B=0) == INVALID and call(B=-1) == INVALID and call(B=65536) == INVALID
        for k in ("gx", "gy", "gz"):
            assert call(grid=_grid(pv, **{k: False})) == INVALID, k
        for k in ("nx", "ny", "nz"):
            for bad in (1, 0, -3):
                assert call(grid=_grid(pv, **{k: bad})) == INVALID, (k, bad)
        assert call(nbytes=need - 1) == INVALID and call(nbytes=0) == INVALID and call(nbytes=-8) == INVALID
        assert call(B=2) == INVALID                                             # the scratch of one image for two
        assert call(scratch=ctypes.c_void_p(pv.value + 1)) == INVALID           # not 4-byte aligned
        huge = 1 << 40                                                          # the limits hold whatever the scratch claims
        assert call(grid=_grid(pv, nx=565, ny=565, nz=565), nbytes=huge) == INVALID
        assert call(grid=_grid(pv, nx=2, ny=2, nz=INT_MAX // 28 + 1), nbytes=huge) == INVALID
        assert call(grid=_grid(pv, nx=INT_MAX, ny=INT_MAX, nz=INT_MAX), nbytes=huge) == INVALID
    assert lib.cips_mesh_emit(None, pv, 0.5, 1, pv, need, pv, pv, pv, None) == INVALID
    assert emit(vertices=None) == INVALID
    assert emit(faces=None) == INVALID
