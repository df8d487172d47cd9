"""GPU: the single-pass ("bf16") implicit-GEMM convolution kernels at the op level — cips_conv2d_bf16 (forward and stride-1 data
gradient, fused epilogue, split contraction), cips_conv2d_bf16_dgrad_s2 (parity data gradient), cips_conv2d_bf16_wgrad — and
dm.conv2d in CONV_MODE "bf16" through every order of differentiation.

Yardstick (derived, as in test_gpu_gemm_bf16.py): fp64 conv2d / conv_transpose2d / torch.nn.grad.conv2d_weight on the SAME hi
planes, i.e. on x.bfloat16().double().  The kernels' products hi * hi are exact in fp32, so only the fp32 accumulation differs
from the fp64 sum: per element
    |err| <= 4 * K * 2^-24 * S,    S = the same convolution of the absolute values, K = the contraction length
(K roundings of at most one fp32 ulp of a partial sum that never exceeds S, doubled for the matrix core's own rounding of its
internal partial sums; the partial sums of a split contraction or of the weight gradient's chunks add ksplit <= K roundings of
the same kind and are inside the factor 4).  The parity data gradient contracts over the taps of the pixel's parity class only:
K is taken per class.  The fused epilogue y = leaky_relu(acc + bias) * act_scale is 1-Lipschitz in acc up to act_scale:
act_scale * bound, plus three fp32 roundings of the value itself (add, slope, scale: 4 * 2^-24 |y|).

Every case also shows
  * that the lo planes are not read: NaN-filled lo planes (the zero row's lo included) give the same bits, all finite;
  * that it is ONE pass: the 3-pass entry point on the same planes differs by more than the bound somewhere.  For operands of
    random sign the lo terms are a random walk of ~sqrt(2K) * 2^-10 * rms|a b| against a bound that grows like K * S ~ K^2: at
    K = 576 the largest of 50 000 elements is about twice the bound, at K = 1152 it is below it, and the case list has
    K = 1728.  So this part runs on a second data set per case whose lo terms add up instead of cancelling: non-negative
    operands of the form h * (1 + 2^-9), h a bf16 value — hi = h and lo = 2^-9 h exactly, so the 3-pass result is
    (1 + 2^-8) x the single-pass one and the difference, 2^-8 S, is 2^14 / K bounds (9.5 at K = 1728) at every element.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
SLOPE, ACT_SCALE = 0.2, 2 ** 0.5
UNSUPPORTED = "hipError 801"


def dev():
    return torch.device("cuda:0")


def _hi(t):
    """the value of the hi plane, in fp64"""
    return t.float().bfloat16().double()


def _coherent(t):
    """|t| rounded to bf16, times (1 + 2^-9): hi plane h, lo plane 2^-9 h, both exact (module docstring)"""
    return t.abs().float().bfloat16().float() * (1 + 2.0 ** -9)


def _nan_lo(ops, P):
    return ops.Planes(P.hi, torch.full_like(P.lo, float("nan")))


def _w_planes(ops, w):
    O, C, kh, kw = w.shape
    P, _ = ops.split_planes(w.permute(0, 2, 3, 1).reshape(1, O, kh * kw * C).contiguous(), want_p=True, want_t=False)
    return P


def _w_planes_flipT(ops, w):
    return _w_planes(ops, w.flip(2, 3).transpose(0, 1).contiguous())


def _within(got, want, bound, what):
    err = (got.detach().double().cpu() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst |err| / bound {worst:.3f}, rel L2 {float(err.norm() / want.norm()):.2e}")
    assert torch.isfinite(got).all(), what
    assert bool((err <= bound).all()), (what, worst)


def _one_pass(y1, y3, bound, what):
    """the 3-pass result differs from the single-pass one by more than the bound somewhere"""
    diff = (y3.detach().double().cpu() - y1.detach().double().cpu()).abs()
    ratio = float((diff / bound.clamp_min(1e-300)).max())
    print(f"{what}: largest |3-pass - single| / bound {ratio:.2f}")
    assert bool((diff > bound).any()), (what, ratio)


# --------------------------------------------------------------------------------------------------------------------------
# forward and stride-1 data gradient
# --------------------------------------------------------------------------------------------------------------------------
FWD = [(3, 64, 64, 16, 3, 1, 1),        # 9 stages: an odd count
       (2, 64, 96, 20, 3, 1, 1),        # ragged: 400 pixels, 96 rows
       (1, 192, 64, 24, 3, 1, 1),       # 3 stages per tap
       (2, 128, 128, 8, 1, 1, 0),       # exactly two stages; 64-pixel planes, batch folded
       (8, 64, 64, 4, 3, 1, 1),         # 16-pixel planes folded
       (2, 128, 64, 17, 3, 2, 0)]       # stride 2


def _fwd_data(cfg, seed, coherent=False):
    B, C, O, H, k, stride, pad = cfg
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, H, generator=g)
    w = torch.randn(O, C, k, k, generator=g) / (C * k * k) ** 0.5
    if coherent:
        x, w = _coherent(x), _coherent(w)
    return x, w


def _fwd_ref(x, w, stride, pad):
    xh, wh = _hi(x), _hi(w)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return F.conv2d(xh, wh, stride=stride, padding=pad), 4 * K * EPS * F.conv2d(xh.abs(), wh.abs(), stride=stride, padding=pad)


@pytest.mark.parametrize("cfg", FWD)
def test_forward_single_pass(cfg):
    from cips3d_amd import ops
    B, C, O, H, k, stride, pad = cfg
    d = dev()
    x, w = _fwd_data(cfg, 100 + H + C)
    want, bound = _fwd_ref(x, w, stride, pad)
    wP, xP = _w_planes(ops, w.to(d)), ops.split_planes_nhwc(x.to(d))
    args = (B, C, H, H, O, k, k, stride, pad)
    y = ops.conv2d_x3(wP, xP, *args, single=True)
    _within(y, want, bound, f"forward {cfg}")
    y_nan = ops.conv2d_x3(_nan_lo(ops, wP), _nan_lo(ops, xP), *args, single=True)
    assert torch.equal(y_nan, y) and torch.isfinite(y_nan).all()
    # one pass (the second data set of the module docstring)
    xc, wc = _fwd_data(cfg, 100 + H + C, coherent=True)
    wantc, boundc = _fwd_ref(xc, wc, stride, pad)
    wPc, xPc = _w_planes(ops, wc.to(d)), ops.split_planes_nhwc(xc.to(d))
    y1 = ops.conv2d_x3(wPc, xPc, *args, single=True)
    _within(y1, wantc, boundc, f"forward {cfg}, coherent lo planes")
    _one_pass(y1, ops.conv2d_x3(wPc, xPc, *args), boundc, f"forward {cfg}")


@pytest.mark.parametrize("cfg", [c for c in FWD if c[5] == 1])
def test_stride1_data_gradient_single_pass(cfg):
    """dx = conv(dy, flipped weights with the channel roles swapped, padding k - 1 - pad): the same kernel, contraction over
    (tap, O).  O = 96 is no multiple of 64: refused (801), not run"""
    from cips3d_amd import ops
    B, C, O, H, k, stride, pad = cfg
    d = dev()
    g = torch.Generator().manual_seed(200 + H + C)
    w = torch.randn(O, C, k, k, generator=g) / (C * k * k) ** 0.5
    Ho = H + 2 * pad - k + 1
    dy = torch.randn(B, O, Ho, Ho, generator=g)
    args = (B, O, Ho, Ho, C, k, k, 1, k - 1 - pad)
    if O % 64:
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            ops.conv2d_x3(_w_planes_flipT(ops, w.to(d)), ops.split_planes_nhwc(dy.to(d)), *args, single=True)
        return

    def ref(dy_, w_):
        dh, wh = _hi(dy_), _hi(w_)
        return F.conv_transpose2d(dh, wh, padding=pad), 4 * k * k * O * EPS * F.conv_transpose2d(dh.abs(), wh.abs(), padding=pad)

    want, bound = ref(dy, w)
    wP, dP = _w_planes_flipT(ops, w.to(d)), ops.split_planes_nhwc(dy.to(d))
    dx = ops.conv2d_x3(wP, dP, *args, single=True)
    assert dx.shape == (B, C, H, H)
    _within(dx, want, bound, f"dgrad-s1 {cfg}")
    assert torch.equal(ops.conv2d_x3(_nan_lo(ops, wP), _nan_lo(ops, dP), *args, single=True), dx)
    dyc, wc = _coherent(dy), _coherent(w)
    wantc, boundc = ref(dyc, wc)
    wPc, dPc = _w_planes_flipT(ops, wc.to(d)), ops.split_planes_nhwc(dyc.to(d))
    y1 = ops.conv2d_x3(wPc, dPc, *args, single=True)
    _within(y1, wantc, boundc, f"dgrad-s1 {cfg}, coherent lo planes")
    _one_pass(y1, ops.conv2d_x3(wPc, dPc, *args), boundc, f"dgrad-s1 {cfg}")


@pytest.mark.parametrize("cfg", [FWD[0], FWD[4]])
def test_forward_single_pass_with_bias_and_activation_in_the_epilogue(cfg):
    from cips3d_amd import ops
    B, C, O, H, k, stride, pad = cfg
    d = dev()
    x, w = _fwd_data(cfg, 300 + H)
    bias = torch.randn(O, generator=torch.Generator().manual_seed(3)) * 0.3
    acc, bound = _fwd_ref(x, w, stride, pad)
    want = F.leaky_relu(acc + bias.double().view(1, -1, 1, 1), SLOPE) * ACT_SCALE
    bound = ACT_SCALE * bound + 4 * EPS * want.abs()
    wP, xP = _w_planes(ops, w.to(d)), ops.split_planes_nhwc(x.to(d))
    args = (B, C, H, H, O, k, k, stride, pad)
    kw = dict(bias=bias.to(d), act=True, slope=SLOPE, act_scale=ACT_SCALE)
    y = ops.conv2d_x3(wP, xP, *args, single=True, **kw)
    _within(y, want, bound, f"forward + bias + LeakyReLU {cfg}")
    assert torch.equal(ops.conv2d_x3(_nan_lo(ops, wP), _nan_lo(ops, xP), *args, single=True, **kw), y)
    xc, wc = _fwd_data(cfg, 300 + H, coherent=True)
    accc, boundc = _fwd_ref(xc, wc, stride, pad)
    boundc = ACT_SCALE * boundc + 4 * EPS * (F.leaky_relu(accc + bias.double().view(1, -1, 1, 1), SLOPE) * ACT_SCALE).abs()
    wPc, xPc = _w_planes(ops, wc.to(d)), ops.split_planes_nhwc(xc.to(d))
    _one_pass(ops.conv2d_x3(wPc, xPc, *args, single=True, **kw), ops.conv2d_x3(wPc, xPc, *args, **kw), boundc, f"fused {cfg}")


def test_forward_single_pass_split_contraction():
    """ksplit forced to 2 and 3 (18 64-deep k-tiles: 9 + 9, 6 + 6 + 6) and the helper's own proposal: every one inside the
    bound; a split that leaves a chunk one k-tile is refused"""
    from cips3d_amd import ops, _lib
    cfg = (2, 128, 64, 16, 3, 1, 1)
    B, C, O, H, k, stride, pad = cfg
    d = dev()
    x, w = _fwd_data(cfg, 400)
    want, bound = _fwd_ref(x, w, stride, pad)
    wP, xP = _w_planes(ops, w.to(d)), ops.split_planes_nhwc(x.to(d))
    args = (B, C, H, H, O, k, k, stride, pad)
    xc, wc = _fwd_data(cfg, 400, coherent=True)
    _, boundc = _fwd_ref(xc, wc, stride, pad)
    wPc, xPc = _w_planes(ops, wc.to(d)), ops.split_planes_nhwc(xc.to(d))
    proposal = _lib.load().cips_conv2d_bf16_ksplit(B, O, H * H, k * k * C)
    assert proposal == 1 or (k * k * C // 64) // proposal >= 8
    print("proposal:", proposal)
    for ks in (1, 2, 3, None):
        y = ops.conv2d_x3(wP, xP, *args, ksplit=ks, single=True)
        _within(y, want, bound, f"ksplit {ks}")
        assert torch.equal(ops.conv2d_x3(_nan_lo(ops, wP), _nan_lo(ops, xP), *args, ksplit=ks, single=True), y)
        _one_pass(ops.conv2d_x3(wPc, xPc, *args, ksplit=ks, single=True), ops.conv2d_x3(wPc, xPc, *args, ksplit=ks), boundc, f"ksplit {ks}")
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        ops.conv2d_x3(wP, xP, *args, ksplit=10, single=True)              # 18 k-tiles in ten chunks


# --------------------------------------------------------------------------------------------------------------------------
# parity data gradient
# --------------------------------------------------------------------------------------------------------------------------
def _parity_ref(dy, w, H, k):
    O = w.shape[0]
    dh, wh = _hi(dy), _hi(w)
    op = (H - k) % 2
    want = F.conv_transpose2d(dh, wh, stride=2, output_padding=op)
    S = F.conv_transpose2d(dh.abs(), wh.abs(), stride=2, output_padding=op)
    taps = torch.tensor([len(range(p % 2, k, 2)) for p in range(H)], dtype=torch.float64)       # taps of the pixel's parity class
    K = taps.view(-1, 1) * taps.view(1, -1) * O
    return want, 4 * K * EPS * S


@pytest.mark.parametrize("cfg", [(2, 64, 128, 16, 3),       # O = 128: the minimum (the single-tap class has two k-tiles)
                                 (2, 64, 192, 33, 3),       # odd size, ragged blocks
                                 (8, 64, 128, 9, 3)])       # small blocks, batch folded
def test_parity_data_gradient_single_pass(cfg):
    from cips3d_amd import ops
    B, C, O, H, k = cfg
    d = dev()
    g = torch.Generator().manual_seed(500 + H)
    Ho = (H - k) // 2 + 1
    w = torch.randn(O, C, k, k, generator=g) / (C * k * k) ** 0.5
    dy = torch.randn(B, O, Ho, Ho, generator=g)
    want, bound = _parity_ref(dy, w, H, k)
    assert want.shape == (B, C, H, H)

    def run(w_, dy_, single, nan=False):
        banks, w_off = ops.dgrad_s2_banks(w_.to(d))
        dP = ops.split_planes_nhwc(dy_.to(d))
        if nan:
            banks, dP = _nan_lo(ops, banks), _nan_lo(ops, dP)
        dxp, out_off = ops.conv2d_x3_dgrad_s2(banks, w_off, dP, B, C, H, H, O, k, k, single=single)
        blocks = torch.cat([dxp[o:o + B * C * n] for o, n in zip(out_off, ops.dgrad_s2_layout(H, H))])     # without the gaps between them
        return ops.parity_to_nchw(dxp, out_off, B, C, H, H), blocks

    got, blocks = run(w, dy, True)
    _within(got, want, bound, f"parity dgrad {cfg}")
    got_nan, blocks_nan = run(w, dy, True, nan=True)
    assert torch.equal(blocks_nan, blocks) and torch.isfinite(blocks_nan).all()  # the blocks' padding elements included
    wc, dyc = _coherent(w), _coherent(dy)
    wantc, boundc = _parity_ref(dyc, wc, H, k)
    y1, _ = run(wc, dyc, True)
    _within(y1, wantc, boundc, f"parity dgrad {cfg}, coherent lo planes")
    _one_pass(y1, run(wc, dyc, False)[0], boundc, f"parity dgrad {cfg}")
    if cfg == (2, 64, 128, 16, 3):
        b64, o64 = ops.dgrad_s2_banks(w[:64].to(d))                              # O = 64: one k-tile in the single-tap class
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            ops.conv2d_x3_dgrad_s2(b64, o64, ops.split_planes_nhwc(dy[:, :64].contiguous().to(d)), B, C, H, H, 64, k, k, single=True)


# --------------------------------------------------------------------------------------------------------------------------
# weight gradient
# --------------------------------------------------------------------------------------------------------------------------
def _wgrad_ref(x, dy, w_shape, stride, pad):
    xh, dh = _hi(x), _hi(dy)
    K = dy.shape[0] * dy.shape[2] * dy.shape[3]
    want = torch.nn.grad.conv2d_weight(xh, w_shape, dh, stride=stride, padding=pad)
    return want, 4 * K * EPS * torch.nn.grad.conv2d_weight(xh.abs(), w_shape, dh.abs(), stride=stride, padding=pad)


@pytest.mark.parametrize("cfg", [(4, 64, 96, 8, 3, 1, 1),        # 256 output pixels: 4 k-tiles
                                 (2, 128, 64, 16, 1, 1, 0),      # 512: 8 k-tiles
                                 (2, 64, 64, 17, 3, 2, 0)])      # stride 2, B * N = 128: exactly two k-tiles
def test_weight_gradient_single_pass(cfg):
    """the chunk count forced to 1 and 3 and left free.  Three chunks leave every chunk two 64-row k-tiles only at the
    512-pixel case (2 + 3 + 3); at the other two (4 and 2 k-tiles) that count is refused (801), not run"""
    from cips3d_amd import ops
    B, C, O, H, k, stride, pad = cfg
    d = dev()
    g = torch.Generator().manual_seed(600 + H)
    Ho = (H + 2 * pad - k) // stride + 1
    x = torch.randn(B, C, H, H, generator=g)
    dy = torch.randn(B, O, Ho, Ho, generator=g)
    scale = 0.5
    want, bound = _wgrad_ref(x, dy, (O, C, k, k), stride, pad)
    T = B * Ho * Ho // 64
    assert (B * Ho * Ho) % 64 == 0 and T >= 2 and not ops.conv2d_bf16_wgrad_declines(B, Ho * Ho)
    dP, xP = ops.split_planes_nhwc(dy.to(d)), ops.split_planes_nhwc(x.to(d))
    xc, dyc = _coherent(x), _coherent(dy)
    wantc, boundc = _wgrad_ref(xc, dyc, (O, C, k, k), stride, pad)
    dPc, xPc = ops.split_planes_nhwc(dyc.to(d)), ops.split_planes_nhwc(xc.to(d))
    args = (B, C, H, H, O, k, k, stride, pad)
    for nch in (1, 3, None):
        if nch is not None and T // nch < 2:
            with pytest.raises(RuntimeError, match=UNSUPPORTED):
                ops.conv2d_x3_wgrad(dP, xP, *args, scale, nch=nch, single=True)
            continue
        dw = ops.conv2d_x3_wgrad(dP, xP, *args, scale, nch=nch, single=True)
        assert dw is not None and dw.shape == (O, C, k, k)
        _within(dw, scale * want, scale * bound, f"wgrad {cfg} nch {nch}")
        assert torch.equal(ops.conv2d_x3_wgrad(_nan_lo(ops, dP), _nan_lo(ops, xP), *args, scale, nch=nch, single=True), dw)
        y1 = ops.conv2d_x3_wgrad(dPc, xPc, *args, scale, nch=nch, single=True)
        _within(y1, scale * wantc, scale * boundc, f"wgrad {cfg} nch {nch}, coherent lo planes")
        _one_pass(y1, ops.conv2d_x3_wgrad(dPc, xPc, *args, scale, nch=nch), scale * boundc, f"wgrad {cfg} nch {nch}")


def test_weight_gradient_single_pass_declines():
    """B * N = 32 output pixels: no 64-row k-tile.  None, as conv2d_x3_wgrad returns where it declines"""
    from cips3d_amd import ops
    B, C, O, H, k, stride, pad = (2, 64, 64, 4, 3, 1, 1)
    d = dev()
    x, dy = torch.randn(B, C, H, H), torch.randn(B, O, H, H)
    dP, xP = ops.split_planes_nhwc(dy.to(d)), ops.split_planes_nhwc(x.to(d))
    assert ops.conv2d_bf16_wgrad_declines(B, H * H) and not ops.conv2d_x3_wgrad_declines(B, H * H)
    assert ops.conv2d_x3_wgrad(dP, xP, B, C, H, H, O, k, k, stride, pad, single=True) is None
    assert ops.conv2d_x3_wgrad(dP, xP, B, C, H, H, O, k, k, stride, pad) is not None


# --------------------------------------------------------------------------------------------------------------------------
# dm.conv2d in CONV_MODE "bf16": forward, autograd.grad(create_graph=True), backward of (gx**2).sum() + (y**2).sum()
# --------------------------------------------------------------------------------------------------------------------------
def _rb(t):
    return t.to(torch.bfloat16).to(t.dtype)


class EmuConv(torch.autograd.Function):
    """y = conv(x, w) with the operands of its GEMM rounded to bf16 where `rnd[0]`; with EmuConvDgrad and EmuConvWgrad the same
    three mutually differentiating Functions as the product's (discriminator.Conv2dFunction / Conv2dBwdDataFunction /
    Conv2dBwdWeightFunction): every convolution GEMM of every order rounds ITS operands — x and w in the forward, dy and the
    saved operand in each gradient.  rnd = (forward, data gradient, weight gradient) booleans: what runs single-pass."""

    @staticmethod
    def forward(ctx, x, w, stride, pad, rnd):
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, pad, rnd)
        r = _rb if rnd[0] else (lambda t: t)
        return F.conv2d(r(x), r(w), stride=stride, padding=pad)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        stride, pad, rnd = ctx.cfg
        dx = EmuConvDgrad.apply(dy, w, tuple(x.shape), stride, pad, rnd) if ctx.needs_input_grad[0] else None
        dw = EmuConvWgrad.apply(dy, x, tuple(w.shape), stride, pad, rnd) if ctx.needs_input_grad[1] else None
        return dx, dw, None, None, None


class EmuConvDgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, w, in_shape, stride, pad, rnd):
        ctx.save_for_backward(dy, w)
        ctx.cfg = (in_shape, stride, pad, rnd)
        r = _rb if rnd[1] else (lambda t: t)
        op = (in_shape[2] + 2 * pad - w.shape[2]) % stride
        return F.conv_transpose2d(r(dy), r(w), stride=stride, padding=pad, output_padding=op)

    @staticmethod
    def backward(ctx, ggx):
        dy, w = ctx.saved_tensors
        in_shape, stride, pad, rnd = ctx.cfg
        g_dy = EmuConv.apply(ggx, w, stride, pad, rnd) if ctx.needs_input_grad[0] else None
        g_w = EmuConvWgrad.apply(dy, ggx, tuple(w.shape), stride, pad, rnd) if ctx.needs_input_grad[1] else None
        return g_dy, g_w, None, None, None, None


class EmuConvWgrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, x, w_shape, stride, pad, rnd):
        ctx.save_for_backward(dy, x)
        ctx.cfg = (w_shape, stride, pad, rnd)
        r = _rb if rnd[2] else (lambda t: t)
        return torch.nn.grad.conv2d_weight(r(x), w_shape, r(dy), stride=stride, padding=pad)

    @staticmethod
    def backward(ctx, ggw):
        dy, x = ctx.saved_tensors
        w_shape, stride, pad, rnd = ctx.cfg
        g_dy = EmuConv.apply(x, ggw, stride, pad, rnd) if ctx.needs_input_grad[0] else None
        g_x = EmuConvDgrad.apply(dy, ggw, tuple(x.shape), stride, pad, rnd) if ctx.needs_input_grad[1] else None
        return g_dy, g_x, None, None, None, None


# margin of the product over the emulation's own distance from exact: tests/test_gpu_discriminator_bf16.py (measured there)
MARGIN = 1.5


@pytest.mark.parametrize("cfg", [(3, 64, 64, 16, 3, 1, 1), (2, 128, 128, 8, 1, 1, 0)])
def test_conv2d_in_bf16_mode_double_backward(cfg, monkeypatch):
    """the pattern of test_gpu_discriminator.test_conv2d_x3_eligible_shapes_double_backward on two shapes whose forward, data
    and weight gradient all qualify: product and emulation are each compared with the exact fp64 graph, never with each other;
    every quantity stays within MARGIN x the emulation's own distance from exact, and the forward's is at least half of it
    (the mode is in effect)"""
    from cips3d_amd import discriminator as dm
    B, C, O, H, k, stride, pad = cfg
    assert dm._single_pass((B, C, H, H), (O, C, k, k), stride, pad) == (True, True, True)
    d = dev()
    g = torch.Generator().manual_seed(700 + H)
    x0 = torch.randn(B, C, H, H, generator=g, dtype=torch.float64)
    w0 = torch.randn(O, C, k, k, generator=g, dtype=torch.float64) / (C * k * k) ** 0.5
    Ho = (H + 2 * pad - k) // stride + 1
    up = torch.randn(B, O, Ho, Ho, generator=g, dtype=torch.float64)

    def graph(conv, x, w, up_):
        y = conv(x, w)
        gx, = torch.autograd.grad((y * up_).sum(), x, create_graph=True)
        ((gx ** 2).sum() + (y ** 2).sum()).backward()
        return [t.detach().double().cpu() for t in (y, gx, x.grad, w.grad)]

    def leaves(dtype, device):
        return (x0.clone().to(dtype).to(device).requires_grad_(True), w0.clone().to(dtype).to(device).requires_grad_(True),
                up.to(dtype).to(device))

    exact = graph(lambda x, w: F.conv2d(x, w, stride=stride, padding=pad), *leaves(torch.float64, "cpu"))
    emu = graph(lambda x, w: EmuConv.apply(x, w, stride, pad, (True, True, True)), *leaves(torch.float64, "cpu"))
    monkeypatch.setattr(dm, "CONV_MODE", "bf16")
    got = graph(lambda x, w: dm.conv2d(x, w, stride=stride, padding=pad), *leaves(torch.float32, d))
    for what, p, e, t in zip(("y", "gx", "x.grad", "w.grad"), got, emu, exact):
        pe, ee = rel_err(p, t), rel_err(e, t)
        print(f"conv2d [bf16] {cfg} {what}: product {pe:.3e}, emulation {ee:.3e}, ratio {pe / ee:.2f}")
        assert torch.isfinite(p).all() and pe <= MARGIN * ee, (what, pe, ee)
    assert rel_err(got[0], exact[0]) >= 0.5 * rel_err(emu[0], exact[0])
