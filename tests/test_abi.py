"""CPU: the C-ABI shared library builds, loads and exports every symbol include/cips3d_hip.h
declares (no compute calls — there is no GPU here), and the product path refuses to run on CPU."""
import os
import re

import pytest
import torch

from conftest import ROOT, seeded_generator


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(cips_[a-z0-9_]+)\s*\(", txt)))


def test_library_builds_and_exports_every_declared_symbol():
    from cips3d_amd import build, _lib
    build.build(verbose=False)
    assert os.path.exists(_lib.LIB_PATH)
    syms = header_symbols()
    assert len(syms) >= 20
    assert sorted(_lib.SIGNATURES.keys()) == syms, "ctypes table and header disagree"
    lib = _lib.load()
    for s in syms:
        assert hasattr(lib, s), s
    assert lib.cips_version() == 9
    assert lib.cips_arch() == b"gfx950"


def test_library_is_stateless_reads_no_environment_and_exports_no_hooks():
    """the C-ABI keeps no mode between calls and no environment variable changes what it computes
    (round 4 shipped a process-global clamp hook, a process-global kernel selector and ~25 getenv sites, three of which
    produced wrong results by design).  Checked on the built binary: it does not import getenv, carries no CIPS_* variable
    name, and exports only what include/cips3d_hip.h declares — no cips_debug_* / cips_*_set_* entry points.  The tuning
    aids live behind -DCIPS_TUNING (csrc/common.h), which build.py never passes."""
    import subprocess
    from cips3d_amd import build, _lib
    build.build(verbose=False)
    dyn = subprocess.run(["nm", "-D", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    undefined = {l.split()[-1].split("@")[0] for l in dyn.splitlines() if " U " in l}
    assert not ({"getenv", "secure_getenv", "setenv", "putenv"} & undefined), undefined
    exported = sorted(l.split()[-1] for l in dyn.splitlines() if " T cips_" in l)
    assert exported == header_symbols(), set(exported) ^ set(header_symbols())
    assert not [e for e in exported if "debug" in e or "_set_" in e or "prof" in e]
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"CIPS_" not in blob, "an environment variable name is compiled into the production library"
    assert build.HIPCC_EXTRA == [] and "CIPS_TUNING" not in open(build.__file__).read()
    # the C sources read the environment only through the tuning helper of common.h
    csrc = os.path.join(ROOT, "cips3d_amd", "csrc")
    sites = [(f, i + 1) for f in sorted(os.listdir(csrc)) for i, l in enumerate(open(os.path.join(csrc, f)))
             if "getenv" in l and not l.lstrip().startswith("//")]
    assert sites == [("common.h", next(i + 1 for i, l in enumerate(open(os.path.join(csrc, "common.h"))) if "getenv(name)" in l))], sites


def test_struct_layouts_match_header_field_order():
    from cips3d_amd import _lib
    txt = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()

    def fields(struct):
        body = txt[txt.index("typedef struct " + struct):]
        body = body[body.index("{") + 1:body.index("} " + struct)]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for stmt in body.split(";"):
            stmt = stmt.strip()
            if not stmt:
                continue
            names = stmt.replace("*", " ").split()
            decl = stmt.split(None, 1)
            for part in stmt.split(","):
                out.append(part.replace("*", " ").split()[-1])
        return out
    assert fields("cips_siren_weights") == [f[0] for f in _lib.SirenWeights._fields_]
    assert fields("cips_gemm_desc") == [f[0] for f in _lib.GemmDesc._fields_]
    assert fields("cips_gemm_x3_desc") == [f[0] for f in _lib.GemmX3Desc._fields_]


def test_siren_tensor_order_agrees_with_the_structs():
    """ops._SIREN_NAMES is the one order of the 16 SIREN tensors (Function arguments, saved tensors, returned gradients):
    "d" + name must be the fields of SirenGrads in order, and the names exactly the 16 pointer fields of SirenWeights"""
    import ctypes
    from cips3d_amd import _lib, ops
    assert len(ops._SIREN_NAMES) == 16 and len(set(ops._SIREN_NAMES)) == 16
    assert ["d" + n for n in ops._SIREN_NAMES] == [f[0] for f in _lib.SirenGrads._fields_]
    pointers = [f[0] for f in _lib.SirenWeights._fields_ if f[1] is ctypes.c_void_p]
    assert len(pointers) == 16 and sorted(ops._SIREN_NAMES) == sorted(pointers)


def test_product_path_has_no_cpu_fallback():
    G = seeded_generator(0)
    zs = G.get_zs(1)
    with pytest.raises(RuntimeError, match="GPU"):
        G(zs, img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=4, h_stddev=0.3, v_stddev=0.155,
          hierarchical_sample=False, sample_dist="gaussian")


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "cips3d_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert "oracle" not in src.replace("# oracle", ""), f"{f} references the oracle"


def test_product_holds_no_copy_of_the_reference_diffaugment():
    """Round-2 verdict: the op-by-op torch DiffAugment (a renamed copy of exp/cips3d/models/diffaug.py:30-85) left the
    product; the policy runs on the HIP operator (cips_diffaug) only.  The function bodies must stay gone."""
    pkg = os.path.join(ROOT, "cips3d_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                for needle in ("rand_brightness", "rand_saturation", "rand_contrast", "rand_translation", "rand_cutout",
                               "AUGMENT_FNS", "torch.meshgrid", "mask[gb, gx, gy]", "F.pad(x, [1, 1, 1, 1"):
                    assert needle not in src, (f, needle)


def test_entry_points_validate_arguments_before_touching_the_device():
    """Malformed descriptors are refused with hipErrorInvalidValue (1) / hipErrorNotSupported (801) before any HIP
    call — so this runs without a GPU.  (Contraction lengths must be multiples of 32 bf16, planes 16-byte aligned,
    bit-plane gates need 32-column rows, the implicit-GEMM conv 32-channel slices, ...)"""
    import ctypes
    from cips3d_amd import _lib
    lib = _lib.load()
    INVALID, UNSUPPORTED = 1, 801
    d = _lib.GemmX3Desc()
    d.M, d.N, d.K, d.lda, d.ldb, d.batch = 64, 64, 48, 48, 48, 1          # K not a multiple of 32
    assert lib.cips_gemm_bf16x3(ctypes.byref(d), None) == INVALID
    assert lib.cips_gemm_bf16x3_km(ctypes.byref(d), None) == INVALID
    d.K, d.lda, d.ldb = 64, 60, 64                                        # rows not 16-byte aligned
    assert lib.cips_gemm_bf16x3(ctypes.byref(d), None) == INVALID
    d.lda, d.batch = 64, 0
    assert lib.cips_gemm_bf16x3(ctypes.byref(d), None) == INVALID
    d.batch, d.N, d.ldp, d.gate_bits = 1, 72, 72, 1                       # bit-plane gate with 72-column rows
    assert lib.cips_gemm_bf16x3(ctypes.byref(d), None) == INVALID
    assert lib.cips_gemm_bf16x3(None, None) == INVALID
    assert lib.cips_gemm_bf16x3_km_grouped(ctypes.byref(d), 0, None) == INVALID
    assert lib.cips_gemm_bf16x3_km_grouped(ctypes.byref(d), 9, None) == UNSUPPORTED   # more than one launch holds
    c = _lib.ConvX3Desc()
    c.B, c.C, c.H, c.W, c.O, c.kh, c.kw, c.stride, c.pad = 2, 48, 16, 16, 64, 3, 3, 1, 1   # 48 channels: no 32-slices
    assert lib.cips_conv2d_x3(ctypes.byref(c), None) == UNSUPPORTED
    c.C, c.stride = 64, 0
    assert lib.cips_conv2d_x3(ctypes.byref(c), None) == INVALID
    w = _lib.ConvWgradDesc()
    w.B, w.C, w.H, w.W, w.O, w.kh, w.kw, w.stride, w.pad, w.nchunks = 2, 64, 15, 15, 64, 3, 3, 1, 1, 1
    assert lib.cips_conv2d_x3_wgrad(ctypes.byref(w), None) == INVALID    # no output buffer
    buf = (ctypes.c_float * 4)()
    w.part = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.cips_conv2d_x3_wgrad(ctypes.byref(w), None) == UNSUPPORTED   # 450 pixels: no 32-row k-tiles
    # round-2 entry points: host-side helpers and argument validation (no launches)
    w.H = w.W = 16                                                          # 2 * 256 pixels = 16 k-tiles
    w.nchunks = 17
    assert lib.cips_conv2d_x3_wgrad(ctypes.byref(w), None) == UNSUPPORTED   # more chunks than k-tiles
    c.stride, c.ksplit, c.part = 1, 3, None
    assert lib.cips_conv2d_x3(ctypes.byref(c), None) == INVALID             # split contraction without its scratch
    for (B, O, N, K) in [(32, 512, 256, 4608), (32, 256, 4096, 2304), (4, 64, 65536, 576), (1, 32, 256, 288), (32, 512, 1024, 512)]:
        ks = lib.cips_conv2d_x3_ksplit(B, O, N, K)
        tiles = -(-O // 256) * -(-N // 256) * B
        assert 1 <= ks <= 8 and (ks == 1 or (K // 32) // ks >= 8)
        assert ks == 1 or tiles < 256                                       # a full chip is never split
    assert lib.cips_conv2d_x3_ksplit(32, 512, 256, 4608) == 4               # 64 tiles -> 256
    assert lib.cips_conv1x1_smallk_bwd_weight(None, None, None, 2, 3, 8, 64, None) == INVALID
    assert lib.cips_conv1x1_smallk_bwd_weight_splits(64, 65536) == 32 and lib.cips_conv1x1_smallk_bwd_weight_splits(512, 16) == 1
    assert lib.cips_conv1x1_smallk_bwd_weight_splits(8, 30) == 0            # pixels not a multiple of 4
    assert lib.cips_lrelu_bwd_bias(None, None, None, None, 4, 64, 0.2, 1.0, None) == INVALID
    assert lib.cips_lrelu_bwd_bias_slices(64) == 1 and lib.cips_lrelu_bwd_bias_slices(65536) == 16 and lib.cips_lrelu_bwd_bias_slices(1 << 20) == 64
    assert lib.cips_split_planes_nhwc(None, None, None, 2, 64, 16, None) == INVALID
    assert lib.cips_split_planes_nhwc(buf, buf, buf, 2, 60, 16, None) == INVALID        # channels not a multiple of 8
    assert lib.cips_conv_wgrad_finish(None, None, 1, 9, 8, 8, 1.0, None) == INVALID
    assert lib.cips_col2im(None, None, 0, 3, 8, 8, 3, 3, 2, 0, None) == INVALID
    assert lib.cips_conv1x1_smallk(None, None, None, 2, 5, 8, 64, None) == INVALID      # more than 4 input channels
    assert lib.cips_conv1x1_smallk(None, None, None, 2, 3, 8, 30, None) == INVALID      # pixels not a multiple of 4
    assert lib.cips_upfirdn2d(None, None, None, 1, 8, 8, 1, 9, 9, 1, 1, 1, 1, 0, 0, 0, 0, None) == INVALID   # > 64 taps
    assert lib.cips_upfirdn2d_form(8, 8, 1, 9, 9, 1, 1, 1, 1, 0, 0, 0, 0) < 0           # the query refuses what the call refuses
    assert lib.cips_upfirdn2d(None, None, None, 1, 8, 8, 1, 4, 4, 0, 1, 1, 1, 0, 0, 0, 0, None) == INVALID   # up_x 0
    assert lib.cips_upfirdn2d_form(8, 8, 1, 4, 4, 0, 1, 1, 1, 0, 0, 0, 0) < 0 and lib.cips_upfirdn2d_form(8, 8, 1, 4, 4, 1, 1, 1, 0, 0, 0, 0, 0) < 0
    assert lib.cips_upfirdn2d(None, None, None, 1, 2, 2, 1, 4, 4, 1, 1, 1, 1, 0, 0, 0, 0, None) == 0         # empty output: no-op
    # the other streaming kernels of the discriminator and of the mapping networks (no launches)
    assert lib.cips_conv1x1_smallk_bwd_data(None, None, None, 2, 5, 8, 64, None) == INVALID
    assert lib.cips_conv1x1_smallk_bwd_data(None, None, None, 2, 3, 8, 30, None) == INVALID
    assert lib.cips_conv1x1_smallk_bwd_weight(buf, buf, buf, 2, 5, 8, 64, None) == INVALID
    assert lib.cips_conv1x1_smallk_bwd_weight(buf, buf, buf, 2, 3, 8, 30, None) == INVALID
    assert lib.cips_avgpool2(buf, buf, 1, 3, 2, 0, None) == INVALID and lib.cips_avgpool2(buf, buf, 1, 2, 3, 1, None) == INVALID   # odd H / W
    assert lib.cips_avgpool2(None, buf, 1, 2, 2, 0, None) == INVALID and lib.cips_axpby(buf, buf, buf, 1.0, 1.0, 0, None) == INVALID
    assert lib.cips_rownorm_fwd(buf, buf, buf, buf, buf, 1, 1025, 1, 0.2, None) == INVALID               # more than 1024 columns
    assert lib.cips_rownorm_fwd(buf, buf, buf, buf, buf, 1, 4, 5, 0.2, None) == INVALID                  # PixelNorm with LayerNorm
    assert lib.cips_rownorm_fwd(buf, None, None, buf, buf, 1, 4, 1, 0.2, None) == INVALID                # LayerNorm without gamma
    assert lib.cips_rownorm_bwd(buf, buf, buf, buf, buf, buf, buf, buf, buf, 1, 1025, 1, 0.2, None) == INVALID
    assert lib.cips_rownorm_bwd(buf, buf, buf, buf, buf, buf, buf, buf, buf, 1, 4, 5, 0.2, None) == INVALID
    assert lib.cips_torgb_fwd(None, None, None, None, 16, 30, 0, None) == INVALID       # K not a multiple of 4
    assert lib.cips_fused_bias_act(None, buf, None, None, 16, 0, 1, 3, 0, 0.2, 1.0, None) == INVALID   # bias without its size
    assert lib.cips_fused_bias_act(None, None, None, None, 0, 0, 0, 3, 0, 0.2, 1.0, None) == 0          # empty tensor: no-op
    # round-3 entry points
    assert lib.cips_torgb_bwd_x_x3(None, None, None, 0.2, None, None, None, 16, 64, None) == INVALID    # no operands
    assert lib.cips_torgb_bwd_x_x3(buf, buf, None, 0.2, None, buf, buf, 16, 60, None) == INVALID        # K not a multiple of 8
    assert lib.cips_torgb_bwd_w_x3_batch(None, None, 2, None, None, None, None, 128, 512, None) == INVALID
    ptrs = (ctypes.c_void_p * 9)(*[ctypes.cast(buf, ctypes.c_void_p).value] * 9)
    assert lib.cips_torgb_bwd_w_x3_batch(ptrs, ptrs, 9, None, None, None, None, 128, 512, None) == UNSUPPORTED   # more than 8 taps
    assert lib.cips_torgb_bwd_w_x3_batch(ptrs, ptrs, 2, None, None, None, None, 128, 256, None) == UNSUPPORTED   # K != 512
    # the planes addend (ABI 4) is taken by the 256 x 256-tile kernel only: the query says no for anything else, and the
    # GEMM entry point refuses instead of dropping it
    e = _lib.GemmX3Desc()
    e.M, e.N, e.K, e.lda, e.ldb, e.batch, e.ldp, e.strideP, e.gate_bits = 160, 256, 64, 64, 64, 4, 256, 160 * 256, 1
    pv = ctypes.cast(buf, ctypes.c_void_p)
    e.A_hi = e.A_lo = e.B_hi = e.B_lo = e.P_hi = e.P_lo = e.mask = e.addp_hi = e.addp_lo = e.addp_gate = pv
    e.addp_gain = 5.0
    assert lib.cips_gemm_bf16x3_takes_addp(ctypes.byref(e)) == 0                                      # 160 rows: not a v3 shape
    assert lib.cips_gemm_bf16x3(ctypes.byref(e), None) == UNSUPPORTED
    e.addp_hi = None
    assert lib.cips_gemm_bf16x3_takes_addp(ctypes.byref(e)) == 0                                      # nothing to take


# --------------------------------------------------------------------------------------
# cips_upfirdn2d_form: the dispatch rule of cips_upfirdn2d, the very function the entry point switches on
# --------------------------------------------------------------------------------------
def _form(h, w, up, down, pad, minor=1, k=(4, 4)):
    """pad = (x0, x1, y0, y1), the op's order"""
    from cips3d_amd import ops
    return ops.upfirdn2d_form(h, w, minor, k[0], k[1], up, up, down, down, *pad)


def _backward_call(h, w, up, down, pad, k=(4, 4)):
    """(in_h, in_w, up, down, pad) of the call UpFirDn2dBackward makes for this forward (UpFirDn2d.forward's g_pad formulas)"""
    x0, x1, y0, y1 = pad
    out_h = (h * up + y0 + y1 - k[0]) // down + 1
    out_w = (w * up + x0 + x1 - k[1]) // down + 1
    g_pad = (k[1] - x0 - 1, w * up - out_w * down + x0 - up + 1, k[0] - y0 - 1, h * up - out_h * down + y0 - up + 1)
    return out_h, out_w, down, up, g_pad


def test_upfirdn2d_form_codes_agree_with_the_header():
    from cips3d_amd import ops
    txt = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    codes = {n.lower(): int(v) for n, v in re.findall(r"CIPS_UPFIRDN2D_([A-Z0-9_]+) = (\d+)", txt)}
    assert sorted(codes.values()) == list(range(14))             # "none" + the thirteen kernel instantiations
    norm = lambda s: s.replace("<", "_").replace(",", "_").replace(">", "")
    assert [norm(n) for n in ops.UPFIRDN2D_FORMS] == sorted(codes, key=codes.get)
    with pytest.raises(ValueError):
        _form(8, 8, 1, 1, (0, 0, 0, 0), k=(9, 9))
    assert _form(2, 2, 1, 1, (0, 0, 0, 0)) == "none"


def test_upfirdn2d_form_of_the_skip_branch_blur_and_its_backward():
    """ResBlock's skip: Blur pad (1, 1) + down 2 at the power-of-two stages -> the lanes-along-the-half-row kernels, forward
    (TH 4 below out_h 48, else 8) and backward (TU 2 below in_h 24, else 4)"""
    for n in (4, 8, 16, 32, 64, 128, 256):
        assert _form(n, n, 1, 2, (1, 1, 1, 1)) == ("down2_pairs<4>" if n // 2 < 48 else "down2_pairs<8>"), n
        h, w, up, down, g_pad = _backward_call(n, n, 1, 2, (1, 1, 1, 1))
        assert (h, w, up, down, g_pad) == (n // 2, n // 2, 2, 1, (2, 1, 2, 1))
        assert _form(h, w, up, down, g_pad) == ("up2_pairs<2>" if h < 24 else "up2_pairs<4>"), n
    # both thresholds from either side (rows only: the width stays a power of two)
    assert _form(94, 64, 1, 2, (1, 1, 1, 1)) == "down2_pairs<4>" and _form(96, 64, 1, 2, (1, 1, 1, 1)) == "down2_pairs<8>"   # out_h 47 | 48
    assert _form(23, 32, 2, 1, (2, 1, 2, 1)) == "up2_pairs<2>" and _form(24, 32, 2, 1, (2, 1, 2, 1)) == "up2_pairs<4>"
    # what the pairs kernels do not take: another low pad, a negative pad_y0, more output rows than 2 in_h
    assert _form(16, 16, 1, 2, (2, 0, 1, 1)) == "direct<2,8>" and _form(16, 16, 1, 2, (1, 1, -1, 3)) == "direct<2,8>"
    assert _form(8, 8, 2, 1, (2, 1, 1, 2)) == "up2<4>" and _form(8, 8, 2, 1, (2, 1, 2, 2)) == "up2<4>"


def test_upfirdn2d_form_of_widths_that_are_no_power_of_two():
    for n in (12, 24, 65):
        out_h = (n + 2 - 4) // 2 + 1
        assert _form(n, n, 1, 2, (1, 1, 1, 1)) == "direct<2,8>", n
        h, w, up, down, g_pad = _backward_call(n, n, 1, 2, (1, 1, 1, 1))
        assert (h, w) == (out_h, out_h) and _form(h, w, up, down, g_pad) == "up2<4>", n
    assert _form(98, 98, 1, 2, (1, 1, 1, 1)) == "direct<2,16>" and _form(94, 98, 1, 2, (1, 1, 1, 1)) == "direct<2,8>"


def test_upfirdn2d_form_of_the_conv_branch_blur_and_of_other_kernels():
    for n in (4, 8, 16, 32, 46, 47, 48, 64, 65, 128, 256):       # pad (2, 2), down 1: out_h = n + 1
        assert _form(n, n, 1, 1, (2, 2, 2, 2)) == ("direct<1,8>" if n + 1 < 48 else "direct<1,16>"), n
    # its backward is the same blur with the pads of the flipped kernel
    assert _backward_call(32, 32, 1, 1, (2, 2, 2, 2)) == (33, 33, 1, 1, (1, 1, 1, 1)) and _form(33, 33, 1, 1, (1, 1, 1, 1)) == "direct<1,8>"
    # fewer than 4 x 4 taps: the LDS row-band kernel; a band that cannot hold one output row: the generic kernel
    assert _form(17, 19, 1, 1, (1, 0, 1, 1), k=(3, 2)) == "blur<1>" and _form(17, 19, 1, 2, (1, 0, 1, 1), k=(3, 2)) == "blur<2>"
    assert _form(17, 19, 1, 1, (1, 2, 0, 0), k=(1, 4)) == "blur<1>" and _form(200, 260, 1, 2, (1, 2, 0, 0), k=(1, 4)) == "blur<2>"
    assert _form(4, 2100, 1, 1, (1, 1, 1, 1), k=(4, 3)) == "blur_spill" and _form(4, 2000, 1, 1, (1, 1, 1, 1), k=(4, 3)) == "blur<1>"
    assert _form(17, 19, 1, 1, (-1, 2, 1, 1), k=(3, 2)) == "generic"                     # a negative pad
    # interleaved channels, other factors, mixed factors
    assert _form(6, 7, 2, 1, (2, 1, 2, 1), minor=2) == "generic" and _form(16, 16, 1, 2, (1, 1, 1, 1), minor=2) == "generic"
    assert _form(9, 9, 3, 2, (2, 2, 2, 2)) == "generic" and _form(9, 9, 3, 2, (2, 2, 2, 2), k=(5, 3)) == "generic"
    from cips3d_amd import _lib
    assert _lib.load().cips_upfirdn2d_form(16, 16, 1, 4, 4, 1, 1, 2, 1, 1, 1, 1, 1) == 1     # down_x != down_y


# --------------------------------------------------------------------------------------
# cips_modfc_prep_x3_batch_form / cips_modfc_prep_bwd_batch_form: the dispatch rule of the two batch entries of the INR head's
# modulate / demodulate prep, the very functions the entry points switch on
# --------------------------------------------------------------------------------------
def test_modfc_batch_form_codes_agree_with_the_header():
    txt = open(os.path.join(ROOT, "include", "cips3d_hip.h")).read()
    prep = {n: int(v) for n, v in re.findall(r"CIPS_MODFC_PREP_([A-Z0-9_]+) = (\d+)", txt)}
    bwd = {n: int(v) for n, v in re.findall(r"CIPS_MODFC_BWD_([A-Z0-9_]+) = (\d+)", txt)}
    assert prep == {"COLSUM16": 1, "TILES64": 2} and bwd == {"SCALAR": 0, "FUSED2": 2, "FUSED4": 4}


def test_modfc_batch_forms_follow_the_rule():
    """every out_dim % 4 == 0 -> 16-byte column sums; also every in_dim % 8 == 0 -> 64 x 64 tiles; backward: the fused pass
    for every out_dim % 4 == 0, B <= 64 and the largest out_dim <= 512 (2 chunks) or <= 1024 (4 chunks).  The rule is over
    the whole job list: one job that breaks a condition moves every job of the call."""
    from cips3d_amd import ops
    pf, bf = ops.modfc_prep_x3_batch_form, ops.modfc_prep_bwd_batch_form
    assert pf([(512, 512)], 4) == 3 and pf([(8, 4)], 1) == 3 and pf([(72, 1028)], 2) == 3        # no limit on out_dim or B here
    assert pf([(512, 512)], 65) == 3 and pf([(32, 512), (512, 512), (512, 512)] * 8, 4) == 3     # 24 jobs: the head's 18 and more
    assert pf([(36, 520)], 3) == 1 and pf([(36, 520), (8, 4)], 3) == 1 and pf([(4, 8), (8, 4)], 2) == 1   # an in_dim % 8 != 0
    assert pf([(64, 96), (40, 30)], 3) == 0 and pf([(33, 33)], 2) == 0 and pf([(40, 3)], 3) == 0
    assert pf([(8, 6)], 2) == 0                                       # in_dim % 8 == 0 alone selects nothing: bit 1 never without bit 0
    assert bf([(512, 512)], 4) == 2 and bf([(5, 4)], 1) == 2 and bf([(32, 512), (512, 512)], 64) == 2
    assert bf([(8, 516)], 2) == 4 and bf([(8, 516), (8, 1024)], 2) == 4 and bf([(128, 1024)], 64) == 4
    assert bf([(8, 1028)], 2) == 0 and bf([(8, 4), (8, 1028)], 2) == 0                           # largest out_dim above 1024
    assert bf([(16, 64)], 64) == 2 and bf([(16, 64)], 65) == 0                                   # lane b keeps image b: B <= 64
    assert bf([(64, 96), (40, 30)], 3) == 0 and bf([(1, 7)], 1) == 0                             # an out_dim % 4 != 0
    assert bf([(7, 8)], 2) == 2                                                                  # in_dim does not matter here


def test_modfc_batch_forms_refuse_what_the_entries_refuse():
    """no launch is reached: the queries never launch, and the entry points return before they do"""
    import ctypes
    from cips3d_amd import _lib, ops
    lib = _lib.load()
    INVALID = 1
    mx = lib.cips_modfc_max_jobs()
    assert mx == 24
    for form, entry, job_type, wrapper in [
            (lib.cips_modfc_prep_x3_batch_form, lambda j, n, B: lib.cips_modfc_prep_x3_batch(j, n, B, 1e-8, None), _lib.ModfcPrepJob,
             ops.modfc_prep_x3_batch_form),
            (lib.cips_modfc_prep_bwd_batch_form, lambda j, n, B: lib.cips_modfc_prep_bwd_batch(j, n, B, None), _lib.ModfcBwdJob,
             ops.modfc_prep_bwd_batch_form)]:
        jobs = (job_type * (mx + 1))()
        for j in jobs:
            j.in_dim, j.out_dim = 8, 4            # every pointer stays NULL: the query reads none of them
        assert form(jobs, mx, 2) >= 0 and form(jobs, 1, 1) >= 0
        for n, B in [(0, 2), (-1, 2), (mx + 1, 2), (1, 0), (1, -3)]:
            assert form(jobs, n, B) == -INVALID and entry(jobs, n, B) == INVALID, (n, B)
        assert form(None, 1, 2) == -INVALID and entry(None, 1, 2) == INVALID
        for bad in [(0, 4), (8, 0), (-8, 4)]:
            jobs[1].in_dim, jobs[1].out_dim = bad
            assert form(jobs, 2, 2) == -INVALID and entry(jobs, 2, 2) == INVALID, bad
            assert form(jobs, 1, 2) >= 0                              # ... a job past njobs is not read
        with pytest.raises(ValueError):
            wrapper([(8, 4), (0, 4)], 2)
        with pytest.raises(ValueError):
            wrapper([(8, 4)] * (mx + 1), 2)
        with pytest.raises(ValueError):
            wrapper([], 2)
    # the co-resident entry keeps its own refusals (it has one form)
    jobs = (_lib.ModfcBwdJob * 1)()
    jobs[0].in_dim, jobs[0].out_dim = 16, 64
    assert lib.cips_modfc_prep_bwd_batch_cores(jobs, 1, 65, None) == 801
    jobs[0].out_dim = 30
    assert lib.cips_modfc_prep_bwd_batch_cores(jobs, 1, 2, None) == 801
