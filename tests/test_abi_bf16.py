"""CPU: the C ABI of the single-pass ("bf16") GEMM family — cips_gemm_bf16, cips_gemm_bf16_km, cips_gemm_bf16_km_grouped and the
two capability queries — declared, listed in the ctypes table, exported, and validating their arguments like their 3-pass
counterparts before any device call (so nothing here needs a GPU)."""
import ctypes
import os
import re

from conftest import ROOT

NEW = ["cips_gemm_bf16", "cips_gemm_bf16_fuses_torgb", "cips_gemm_bf16_km", "cips_gemm_bf16_km_grouped", "cips_gemm_bf16_takes_addp"]
INVALID, UNSUPPORTED = 1, 801


def _lib():
    from cips3d_amd import build, _lib
    build.build(verbose=False)
    return _lib, _lib.load()


def test_entry_points_exist_in_header_ctypes_table_and_binary():
    import subprocess
    _l, lib = _lib()
    txt = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(cips_[a-z0-9_]+)\s*\(", txt))
    dyn = subprocess.run(["nm", "-D", _l.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in dyn.splitlines() if " T cips_" in l}
    for s in NEW:
        assert s in declared, s
        assert s in _l.SIGNATURES, s
        assert s in exported and hasattr(lib, s), s
    # same signatures as the 3-pass entry points they stand beside
    for s in NEW:
        assert _l.SIGNATURES[s] == _l.SIGNATURES[s.replace("cips_gemm_bf16", "cips_gemm_bf16x3")], s
    # no struct layout and no existing signature changed
    assert lib.cips_version() == 9


def test_malformed_descriptors_get_the_three_pass_entry_points_codes():
    """the malformed descriptors of test_abi.test_entry_points_validate_arguments_before_touching_the_device, through both
    families: same codes"""
    _l, lib = _lib()
    d = _l.GemmX3Desc()

    def both(suffix, *args):
        a = getattr(lib, "cips_gemm_bf16x3" + suffix)(*args)
        b = getattr(lib, "cips_gemm_bf16" + suffix)(*args)
        assert a == b, (suffix, a, b)
        return b

    d.M, d.N, d.K, d.lda, d.ldb, d.batch = 64, 64, 48, 48, 48, 1          # K not a multiple of 32
    assert both("", ctypes.byref(d), None) == INVALID
    assert both("_km", ctypes.byref(d), None) == INVALID
    d.K, d.lda, d.ldb = 64, 60, 64                                        # rows not 16-byte aligned
    assert both("", ctypes.byref(d), None) == INVALID
    d.lda, d.batch = 64, 0
    assert both("", ctypes.byref(d), None) == INVALID
    d.batch, d.N, d.ldp, d.gate_bits = 1, 72, 72, 1                       # bit-plane gate with 72-column rows
    assert both("", ctypes.byref(d), None) == INVALID
    assert both("", None, None) == INVALID
    assert both("_km", None, None) == INVALID
    assert both("_km_grouped", ctypes.byref(d), 0, None) == INVALID
    assert both("_km_grouped", ctypes.byref(d), 9, None) == UNSUPPORTED   # more than one launch holds
    assert both("_km_grouped", None, 1, None) == INVALID
    assert both("_fuses_torgb", None) == 0 and both("_takes_addp", None) == 0
    d.kernel = 7                                                          # no such kernel selector
    d.N, d.ldp, d.gate_bits = 64, 64, 0
    assert both("", ctypes.byref(d), None) == INVALID
    # the planes addend / fused ToRGB at a shape the 256 x 256-tile kernel does not take: refused, never dropped
    buf = (ctypes.c_float * 4)()
    pv = ctypes.cast(buf, ctypes.c_void_p)
    e = _l.GemmX3Desc()
    e.M, e.N, e.K, e.lda, e.ldb, e.batch, e.ldp, e.strideP, e.gate_bits = 160, 256, 64, 64, 64, 4, 256, 160 * 256, 1
    e.A_hi = e.A_lo = e.B_hi = e.B_lo = e.P_hi = e.P_lo = e.mask = e.addp_hi = e.addp_lo = e.addp_gate = pv
    e.addp_gain = 5.0
    assert both("_takes_addp", ctypes.byref(e)) == 0                     # 160 rows
    assert both("", ctypes.byref(e), None) == UNSUPPORTED
    e.addp_hi = None
    assert both("_takes_addp", ctypes.byref(e)) == 0                     # nothing to take


def test_null_lo_planes_are_not_a_reason_to_refuse():
    """A_lo = B_lo = NULL with an otherwise valid shape.  Checked without a launch: the capability queries (pure host code) accept
    the descriptor, and the grouped entry point gets past its per-problem pointer check — it refuses a two-problem group of
    unequal shapes as unsupported, where the 3-pass entry point has already refused the missing lo planes as invalid."""
    _l, lib = _lib()
    buf = (ctypes.c_float * 4)()
    pv = ctypes.cast(buf, ctypes.c_void_p)
    e = _l.GemmX3Desc()
    e.M, e.N, e.K, e.lda, e.ldb, e.batch = 4096, 512, 512, 512, 512, 32
    e.strideA, e.strideB = 4096 * 512, 512 * 512
    e.ldc, e.strideC, e.ldp, e.strideP, e.gate_bits = 512, 4096 * 512, 512, 4096 * 512, 1
    e.A_hi = e.B_hi = e.P_hi = e.P_lo = e.mask = e.addp_hi = e.addp_lo = e.addp_gate = pv
    e.A_lo = e.B_lo = None
    e.addp_gain, e.slope = 5.0, 0.2
    assert lib.cips_gemm_bf16_takes_addp(ctypes.byref(e)) == 1
    f = _l.GemmX3Desc()
    f.M, f.N, f.K, f.lda, f.ldb, f.batch = 4096, 512, 512, 512, 512, 32
    f.strideA, f.strideB = 4096 * 512, 512 * 512
    f.ldc, f.strideC, f.ldp, f.strideP, f.gate_bits, f.act, f.slope = 512, 4096 * 512, 512, 4096 * 512, 2, 1, 0.2
    part = (ctypes.c_float * 8)()
    f.A_hi = f.B_hi = f.P_hi = f.P_lo = f.mask_out = pv
    f.torgb_w = f.torgb_part = (ctypes.addressof(part) + 15) & ~15         # the query wants 16-byte aligned ToRGB buffers
    assert lib.cips_gemm_bf16_fuses_torgb(ctypes.byref(f)) == 1
    # the single-pass 256 x 256 kernel walks 64-deep k-tiles in pairs: K = 192 is the 3-pass kernel's shape only
    e.K = 192
    e.lda = e.ldb = 192
    assert lib.cips_gemm_bf16x3_takes_addp(ctypes.byref(e)) == 1 and lib.cips_gemm_bf16_takes_addp(ctypes.byref(e)) == 0
    g = (_l.GemmX3Desc * 2)()
    for i, K in enumerate((256, 512)):
        g[i].M, g[i].N, g[i].K, g[i].lda, g[i].ldb, g[i].batch, g[i].ldc, g[i].strideC = 512, 512, K, 512, 512, 1, 512, 512 * 512
        g[i].A_hi = g[i].B_hi = pv
        g[i].C = pv
    assert lib.cips_gemm_bf16x3_km_grouped(g, 2, None) == INVALID         # no lo planes
    assert lib.cips_gemm_bf16_km_grouped(g, 2, None) == UNSUPPORTED       # ... accepted; the shapes differ
