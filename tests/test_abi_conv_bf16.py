"""CPU: the C ABI of the single-pass ("bf16") convolution family — cips_conv2d_bf16, cips_conv2d_bf16_ksplit,
cips_conv2d_bf16_dgrad_s2 and cips_conv2d_bf16_wgrad — declared, listed in the ctypes table, exported, validating their
arguments like their 3-pass twins, and refusing the shapes the single-pass kernels do not take with hipErrorNotSupported
before any device call (so nothing here needs a GPU)."""
import ctypes
import os
import re

from conftest import ROOT

NEW = ["cips_conv2d_bf16", "cips_conv2d_bf16_ksplit", "cips_conv2d_bf16_dgrad_s2", "cips_conv2d_bf16_wgrad"]
INVALID, UNSUPPORTED = 1, 801


def _lib():
    from cips3d_amd import build, _lib
    build.build(verbose=False)
    return _lib, _lib.load()


def _twin(s):
    return s.replace("cips_conv2d_bf16", "cips_conv2d_x3")


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
        assert _l.SIGNATURES[s] == _l.SIGNATURES[_twin(s)], s          # the 3-pass twin's signature
    # the header's prototypes agree as text, too: same parameter lists
    protos = dict(re.findall(r"\bint\s+(cips_conv2d_[a-z0-9_]+)\s*\(([^)]*)\)", txt))
    for s in NEW:
        assert protos[s].split() == protos[_twin(s)].split(), s
    # additive: no struct layout and no existing signature changed
    assert lib.cips_version() == 9


def _pv():
    buf = (ctypes.c_float * 4)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_malformed_descriptors_get_the_three_pass_entry_points_codes():
    """the malformed convolution descriptors of test_abi.test_entry_points_validate_arguments_before_touching_the_device, and a
    few more, through both families: same codes (every one is refused before a launch)"""
    _l, lib = _lib()
    keep, pv = _pv()

    def both(suffix, *args):
        a = getattr(lib, "cips_conv2d_x3" + suffix)(*args)
        b = getattr(lib, "cips_conv2d_bf16" + suffix)(*args)
        assert a == b, (suffix, a, b)
        return b

    assert both("", None, None) == INVALID
    c = _l.ConvX3Desc()
    c.B, c.C, c.H, c.W, c.O, c.kh, c.kw, c.stride, c.pad = 2, 48, 16, 16, 64, 3, 3, 1, 1      # 48 channels: no k-tile slices
    assert both("", ctypes.byref(c), None) == UNSUPPORTED
    c.C, c.stride = 64, 0
    assert both("", ctypes.byref(c), None) == INVALID
    c.stride, c.ksplit, c.part = 1, 3, None
    assert both("", ctypes.byref(c), None) == INVALID                     # split contraction without its scratch
    c.ksplit, c.part = 19, pv
    assert both("", ctypes.byref(c), None) == INVALID                     # more chunks than 32-deep k-tiles (18)
    c.ksplit, c.part, c.act = 1, None, 2
    assert both("", ctypes.byref(c), None) == INVALID                     # no such activation
    c.act, c.H, c.W, c.pad = 0, 5, 5, 0
    assert both("", ctypes.byref(c), None) == UNSUPPORTED                 # 9 output pixels: no 8-pixel vectors
    c.H, c.W = 2, 2
    assert both("", ctypes.byref(c), None) == UNSUPPORTED                 # no output pixel at all

    w = _l.ConvWgradDesc()
    assert both("_wgrad", None, None) == INVALID
    w.B, w.C, w.H, w.W, w.O, w.kh, w.kw, w.stride, w.pad, w.nchunks = 2, 64, 15, 15, 64, 3, 3, 1, 1, 1
    assert both("_wgrad", ctypes.byref(w), None) == INVALID              # no output buffer
    w.part = pv
    assert both("_wgrad", ctypes.byref(w), None) == UNSUPPORTED          # 450 pixels: no k-tiles
    w.H = w.W = 16
    w.nchunks = 17
    assert both("_wgrad", ctypes.byref(w), None) == UNSUPPORTED          # more chunks than k-tiles
    w.nchunks, w.C = 1, 60
    assert both("_wgrad", ctypes.byref(w), None) == UNSUPPORTED          # channels not in 8-element vectors
    w.C, w.nchunks = 64, 0
    assert both("_wgrad", ctypes.byref(w), None) == INVALID

    s = _l.ConvDgradS2Desc()
    assert both("_dgrad_s2", None, None) == INVALID
    s.B, s.C, s.H, s.W, s.O, s.kh, s.kw = 2, 64, 17, 17, 128, 3, 3
    assert both("_dgrad_s2", ctypes.byref(s), None) == INVALID           # no planes, no output
    s.w_hi = s.w_lo = s.dy_hi = s.dy_lo = s.dxp = pv
    s.H = 2
    assert both("_dgrad_s2", ctypes.byref(s), None) == INVALID           # input smaller than the filter
    s.H, s.O = 17, 48
    assert both("_dgrad_s2", ctypes.byref(s), None) == UNSUPPORTED       # 48 output channels: no k-tile slices
    s.O, s.C = 128, 60
    assert both("_dgrad_s2", ctypes.byref(s), None) == UNSUPPORTED       # channels not in 8-element vectors
    s.C = 64
    s.w_off[1] = 4                                                        # a filter bank that is not 16-byte aligned
    assert both("_dgrad_s2", ctypes.byref(s), None) == INVALID
    del keep


def test_null_lo_planes_are_not_a_reason_to_refuse():
    """dgrad_s2 is the entry point that checks its plane pointers: without the lo planes the 3-pass twin refuses the
    descriptor as invalid, the single-pass one gets past that check (and on to the next refusal, so nothing is launched)"""
    _l, lib = _lib()
    keep, pv = _pv()
    s = _l.ConvDgradS2Desc()
    s.B, s.C, s.H, s.W, s.O, s.kh, s.kw = 2, 60, 17, 17, 128, 3, 3
    s.w_hi = s.dy_hi = s.dxp = pv
    s.w_lo = s.dy_lo = None
    assert lib.cips_conv2d_x3_dgrad_s2(ctypes.byref(s), None) == INVALID
    assert lib.cips_conv2d_bf16_dgrad_s2(ctypes.byref(s), None) == UNSUPPORTED      # ... accepted; 60 channels
    del keep


def test_shapes_the_single_pass_form_does_not_take_are_refused_not_run():
    """hipErrorNotSupported, never a wrong result and never a silent 3-pass run: 32 contraction channels (a 64-deep k-tile
    would straddle two taps), O = 64 in the parity data gradient (its single-tap class has one k-tile), 96 output pixels in
    the weight gradient (no 64-row k-tiles), a contraction of exactly one 64-deep k-tile — and chunks (ksplit / nchunks)
    that leave a chunk fewer than two k-tiles"""
    _l, lib = _lib()
    keep, pv = _pv()
    c = _l.ConvX3Desc()
    c.w_hi = c.x_hi = c.y = pv
    c.B, c.C, c.H, c.W, c.O, c.kh, c.kw, c.stride, c.pad, c.ksplit = 2, 32, 16, 16, 64, 3, 3, 1, 1, 1
    assert lib.cips_conv2d_bf16(ctypes.byref(c), None) == UNSUPPORTED             # C = 32
    c.C, c.kh, c.kw, c.pad = 64, 1, 1, 0
    assert lib.cips_conv2d_bf16(ctypes.byref(c), None) == UNSUPPORTED             # K = 64: one k-tile
    c.C, c.ksplit, c.part = 192, 2, pv
    assert lib.cips_conv2d_bf16(ctypes.byref(c), None) == UNSUPPORTED             # K = 192 in two chunks: 1 + 2 k-tiles
    s = _l.ConvDgradS2Desc()
    s.w_hi = s.dy_hi = s.dxp = pv
    s.B, s.C, s.H, s.W, s.O, s.kh, s.kw = 2, 64, 17, 17, 64, 3, 3
    assert lib.cips_conv2d_bf16_dgrad_s2(ctypes.byref(s), None) == UNSUPPORTED    # O = 64
    s.O = 96
    assert lib.cips_conv2d_bf16_dgrad_s2(ctypes.byref(s), None) == UNSUPPORTED    # O = 96: no 64-channel slices
    w = _l.ConvWgradDesc()
    w.dy_hi = w.x_hi = w.part = pv
    w.B, w.C, w.H, w.W, w.O, w.kh, w.kw, w.stride, w.pad, w.nchunks = 6, 64, 4, 4, 64, 3, 3, 1, 1, 1
    assert lib.cips_conv2d_bf16_wgrad(ctypes.byref(w), None) == UNSUPPORTED       # B * N = 96
    w.B = 4
    assert lib.cips_conv2d_bf16_wgrad(ctypes.byref(w), None) == UNSUPPORTED       # B * N = 64: one k-tile
    w.B, w.nchunks = 16, 3
    assert lib.cips_conv2d_bf16_wgrad(ctypes.byref(w), None) == UNSUPPORTED       # 4 k-tiles in three chunks
    del keep


def test_ksplit_proposal_cuts_at_64_deep_granularity():
    """the proposal of cips_conv2d_bf16_ksplit leaves every chunk eight 64-deep k-tiles or more (so always two), never splits a
    full chip, and is 1 wherever the contraction has fewer than sixteen k-tiles"""
    _l, lib = _lib()
    for (B, O, N, K) in [(32, 512, 256, 4608), (32, 256, 4096, 2304), (4, 64, 65536, 576), (1, 64, 256, 576), (32, 512, 1024, 512),
                         (2, 64, 256, 1152), (3, 64, 256, 576), (2, 128, 64, 128), (8, 512, 16, 4608)]:
        ks = lib.cips_conv2d_bf16_ksplit(B, O, N, K)
        tiles = -(-O // 256) * (-(-B * N // 256) if N < 256 and B > 1 else -(-N // 256) * B)
        assert 1 <= ks <= 8 and (ks == 1 or (K // 64) // ks >= 8), (B, O, N, K, ks)
        assert ks == 1 or tiles < 256
        assert ks == 1 or K // 64 >= 16
    assert lib.cips_conv2d_bf16_ksplit(32, 512, 256, 4608) == 4               # 64 tiles -> 256, 18 k-tiles each
