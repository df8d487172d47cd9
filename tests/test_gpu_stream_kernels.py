"""GPU: the streaming kernels of the discriminator path (cips3d_amd/csrc/disc_ops.hip) and of the z -> style mapping path
(the row kernels of small_ops.hip), ONE KERNEL AT A TIME against a float64 restatement of the operation built on the CPU
from seeded inputs.  The model-level tests (d_r16, the real-size discriminator, the mapping networks) run all of them,
but with tolerances sized for a whole network and at shapes that are multiples of every tile; here every kernel
instantiation is reached at the smallest shapes that take each of its edges: ragged tiles, one-lane tails, rows wider than a
wave, negative pads, grid-stride second trips.

Which upfirdn2d kernel a case reaches is asserted through ops.upfirdn2d_form (cips_upfirdn2d_form, the function the entry
point itself switches on): a change of the dispatch rule that takes a kernel's only test away fails here.

Not covered: the 131 072-workgroup grid caps of the register-tiled upfirdn2d kernels (their grid-stride loops take a second
trip only from ~33 M work items on: several hundred MB per tensor)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from conftest import max_rel, rel_err
from oracle import cips3d_oracle as orc

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------
# upfirdn2d
# --------------------------------------------------------------------------------------
def upfirdn_ref(x, k, up, down, pad):
    """x (major, H, W, minor), k (kh, kw), pad = (x0, x1, y0, y1) -> float64 (major, out_h, out_w, minor): zero-stuff by `up`,
    pad (or crop, where a pad is negative), correlate with the flipped kernel, keep every `down`-th sample"""
    x0, x1, y0, y1 = pad
    mj, h, w, mi = x.shape
    kh, kw = k.shape
    t = x.double().permute(0, 3, 1, 2).reshape(mj * mi, 1, h, w)
    z = t.new_zeros(mj * mi, 1, h * up, w * up)
    z[:, :, ::up, ::up] = t
    z = F.pad(z, [max(x0, 0), max(x1, 0), max(y0, 0), max(y1, 0)])
    z = z[:, :, max(-y0, 0): z.shape[2] - max(-y1, 0), max(-x0, 0): z.shape[3] - max(-x1, 0)]
    z = F.conv2d(z, torch.flip(k.double(), [0, 1]).view(1, 1, kh, kw))[:, :, ::down, ::down]
    return z.reshape(mj, mi, z.shape[2], z.shape[3]).permute(0, 2, 3, 1).contiguous()


def backward_call(h, w, kh, kw, up, down, pad):
    """(up, down, pad) of the upfirdn2d call that is the transpose of this one: UpFirDn2d.forward's g_pad formulas
    (cips3d_amd/discriminator.py); it takes the flipped kernel and the (out_h, out_w) planes"""
    x0, x1, y0, y1 = pad
    out_h = (h * up + y0 + y1 - kh) // down + 1
    out_w = (w * up + x0 + x1 - kw) // down + 1
    return down, up, (kw - x0 - 1, w * up - out_w * down + x0 - up + 1, kh - y0 - 1, h * up - out_h * down + y0 - up + 1)


def test_upfirdn_reference_restates_the_oracle():
    """the four-pad float64 helper above against the oracle's upfirdn2d (symmetric pads, float32) on the shapes the golden
    fixtures use: up, down, both, negative pads"""
    g = torch.Generator().manual_seed(5)
    for (up, down, pad, ksh) in [(1, 1, (2, 2), (4, 4)), (1, 2, (1, 1), (4, 4)), (2, 1, (2, 1), (4, 4)), (2, 2, (1, 2), (3, 2)),
                                 (1, 1, (-1, 2), (4, 4)), (3, 2, (2, 2), (5, 3)), (2, 1, (-1, -1), (4, 4))]:
        x = torch.randn(3, 9, 11, 1, generator=g, dtype=torch.float64)
        k = torch.randn(*ksh, generator=g, dtype=torch.float64)
        ref = upfirdn_ref(x, k, up, down, (pad[0], pad[1], pad[0], pad[1]))
        yo = orc.upfirdn2d(x.view(1, 3, 9, 11), k, up=up, down=down, pad=pad)
        assert ref.shape[1:3] == yo.shape[2:] and max_rel(ref[..., 0], yo[0]) < 1e-14, (up, down, pad)


def _uf(major, h, w, up, down, pad, form, minor=1, k=(4, 4)):
    return pytest.param(major, h, w, up, down, pad, form, minor, k,
                        id=f"{form}-{major}x{h}x{w}" + (f"x{minor}" if minor > 1 else "") + f"-u{up}d{down}-p{'_'.join(map(str, pad))}-k{k[0]}x{k[1]}")


# (major, H, W, up, down, (px0, px1, py0, py1), expected kernel[, minor, kernel shape]); the form of every row was worked
# out by hand from the rule (out_h / out_w from the op's formula) before the query was asked
UPFIRDN_CASES = [
    _uf(3, 16, 16, 1, 2, (1, 1, 1, 1), "down2_pairs<4>"),            # row segments of 8 lanes
    _uf(2, 20, 128, 1, 2, (1, 2, 0, 1), "down2_pairs<4>"),           # one 64-lane segment per row, pad_x1 2, pad_y0 0, out_h 9
    _uf(70, 4, 4, 1, 2, (1, 1, 1, 1), "down2_pairs<4>"),             # out_w 2: every lane is both edges' neighbour
    _uf(2, 100, 256, 1, 2, (1, 1, 2, 0), "down2_pairs<8>"),          # two segments per row (edge-lane loads), out_h 50 = 6 x 8 + 2
    _uf(3, 8, 8, 2, 1, (2, 1, 2, 1), "up2_pairs<2>"),                # segments of 8
    _uf(3, 7, 8, 2, 1, (2, 1, 2, 0), "up2_pairs<2>"),                # odd in_h, odd out_h 13
    _uf(5, 1, 2, 2, 1, (2, 1, 2, 1), "up2_pairs<2>"),                # one input row
    _uf(2, 26, 128, 2, 1, (2, 1, 2, 1), "up2_pairs<4>"),             # two segments per row, 26 = 6 x 4 + 2 input rows
    _uf(2, 24, 64, 2, 1, (2, 1, 2, -1), "up2_pairs<4>"),             # negative pad_y1: out_h 46 < 2 in_h
    _uf(3, 9, 12, 2, 1, (2, 1, 2, 1), "up2<4>"),                     # width no power of two
    _uf(2, 8, 8, 2, 1, (1, 1, 1, 1), "up2<4>"),                      # pad_x0 != 2
    _uf(2, 6, 7, 2, 1, (-1, 2, 3, -1), "up2<4>"),                    # negative pads
    _uf(3, 9, 11, 1, 1, (2, 2, 2, 2), "direct<1,8>"),
    _uf(2, 9, 11, 1, 1, (-1, 2, 2, -1), "direct<1,8>"),              # negative pads
    _uf(2, 50, 20, 1, 1, (2, 1, 1, 2), "direct<1,16>"),              # out_h 50 = 3 x 16 + 2
    _uf(4, 65, 65, 1, 2, (1, 1, 1, 1), "direct<2,8>"),
    _uf(1, 101, 33, 1, 2, (2, 1, 1, 2), "direct<2,16>"),             # out_h 51
    _uf(3, 17, 19, 1, 1, (1, 0, 1, 1), "blur<1>", k=(3, 2)),         # one band
    _uf(3, 17, 19, 1, 2, (1, 0, 1, 1), "blur<2>", k=(3, 2)),
    _uf(3, 17, 19, 1, 1, (1, 2, 0, 0), "blur<1>", k=(1, 4)),
    _uf(3, 17, 19, 1, 2, (1, 2, 0, 0), "blur<2>", k=(1, 4)),
    _uf(1, 200, 260, 1, 1, (1, 0, 1, 1), "blur<1>", k=(3, 2)),       # several row bands
    _uf(1, 200, 260, 1, 2, (1, 0, 1, 1), "blur<2>", k=(3, 2)),
    _uf(1, 200, 260, 1, 1, (1, 2, 0, 0), "blur<1>", k=(1, 4)),
    _uf(1, 200, 260, 1, 2, (1, 2, 0, 0), "blur<2>", k=(1, 4)),
    _uf(1, 4, 2100, 1, 1, (1, 1, 1, 1), "blur_spill", k=(4, 3)),     # 4 rows of 2104 floats exceed the 32 KiB band (34 KB input)
    _uf(2, 6, 7, 2, 1, (2, 1, 2, 1), "generic", minor=2),
    _uf(1, 5, 5, 2, 2, (2, 1, 2, 1), "generic", minor=3),
    _uf(2, 9, 9, 3, 2, (2, 2, 2, 2), "generic", k=(5, 3)),
]
# every kernel instantiation behind cips_upfirdn2d has a case ("none" launches nothing)
assert {c.values[6] for c in UPFIRDN_CASES} == {"generic", "direct<1,8>", "direct<1,16>", "direct<2,8>", "direct<2,16>", "up2<4>",
                                                "down2_pairs<4>", "down2_pairs<8>", "up2_pairs<2>", "up2_pairs<4>", "blur<1>",
                                                "blur<2>", "blur_spill"}


@pytest.mark.parametrize("major,h,w,up,down,pad,form,minor,ksh", UPFIRDN_CASES)
def test_upfirdn2d_every_kernel(major, h, w, up, down, pad, form, minor, ksh):
    """(a) the case reaches the kernel it is meant for; (b) max_rel < 1e-6 against float64 (the bar of this op's other tests);
    (c) the values are the generic kernel's bit for bit — channel 0 of the same call with a second interleaved channel
    (minor = 2 always takes the generic kernel; a case that is interleaved itself is compared the other way round, channel by
    channel against the minor = 1 calls) — which is what disc_ops.hip says of every fast form; (d) <upfirdn(x), g> =
    <x, upfirdn^T(g)> with the transpose computed by the call the backward makes.

    (d)'s bound: both products are formed in float64 from the kernels' float32 outputs, so they differ by the outputs'
    rounding.  The float64 reference rounded to float32 shows how large that is for correctly rounded outputs, element by
    element; the two products may differ by 4 x the sum of those errors weighted with the other factor, sum |g| |fl(y) - y| +
    sum |x| |fl(gx) - gx| (4: a chain of up to 16 fmas is not correctly rounded).  One tap of one border pixel taken from the
    wrong place moves a product by ~|x| |g| |k|, orders of magnitude more.
    (b) and (c) are checked with the kernel the discriminator uses (or a ramp of the case's own shape) AND with a random
    non-symmetric kernel of the same shape: flip and transpose conventions."""
    from cips3d_amd import ops
    d = dev()
    kh, kw = ksh
    assert ops.upfirdn2d_form(h, w, minor, kh, kw, up, up, down, down, *pad) == form                       # (a)
    assert ops.upfirdn2d_form(h, w, 2, kh, kw, up, up, down, down, *pad) == "generic"
    g = torch.Generator().manual_seed(1000 * h + 10 * w + up + down + minor)
    x = torch.randn(major, h, w, minor, generator=g)
    if ksh == (4, 4):
        k0 = torch.tensor([1., 3., 3., 1.]); k0 = k0[None] * k0[:, None]; k0 = k0 / k0.sum()
    else:
        k0 = (torch.arange(kh * kw, dtype=torch.float32).view(kh, kw) + 1) / (kh * kw)
    xd = x.to(d)
    other = torch.randn(major, h, w, generator=g).to(d)
    for k in (k0, torch.randn(kh, kw, generator=g)):
        kd = k.to(d)
        ref = upfirdn_ref(x, k, up, down, pad)
        y = ops.upfirdn2d_op(xd, kd, up, up, down, down, *pad)
        assert y.shape == ref.shape
        e = max_rel(y, ref)
        print(f"{form}: max_rel {e:.3e}")
        assert e < 1e-6                                                                                    # (b)
        if minor == 1:                                                                                     # (c)
            y2 = ops.upfirdn2d_op(torch.stack([xd[..., 0], other], -1), kd, up, up, down, down, *pad)
            assert torch.equal(y[..., 0], y2[..., 0])
        else:
            for c in range(minor):
                y1 = ops.upfirdn2d_op(xd[..., c:c + 1].contiguous(), kd, up, up, down, down, *pad)
                assert torch.equal(y[..., c], y1[..., 0]), c
        # (d)
        bup, bdown, bpad = backward_call(h, w, kh, kw, up, down, pad)
        gy = torch.randn(ref.shape, generator=g)
        kf = torch.flip(k, [0, 1])
        gx = ops.upfirdn2d_op(gy.to(d), kf.to(d), bup, bup, bdown, bdown, *bpad)
        gx_ref = upfirdn_ref(gy, kf, bup, bdown, bpad)
        assert gx.shape == x.shape == gx_ref.shape
        assert max_rel(gx, gx_ref) < 1e-6
        lhs_ref, rhs_ref = float((ref * gy.double()).sum()), float((x.double() * gx_ref).sum())
        scale = float((ref * gy.double()).abs().sum())
        assert abs(lhs_ref - rhs_ref) <= 1e-12 * scale                     # the reference's two calls are each other's transpose
        lhs, rhs = float((y.double().cpu() * gy.double()).sum()), float((x.double() * gx.double().cpu()).sum())
        bound = 4 * float((gy.double().abs() * (ref.float().double() - ref).abs()).sum() +
                          (x.double().abs() * (gx_ref.float().double() - gx_ref).abs()).sum())
        print(f"{form}: adjoint gap {abs(lhs - rhs):.3e}, bound {bound:.3e}, products {lhs_ref:.6e}")
        assert abs(lhs - rhs) <= bound


# --------------------------------------------------------------------------------------
# conv1x1_smallk: forward, data gradient, weight gradient
# --------------------------------------------------------------------------------------
SMALLK_BCO = [(1, 1, 1), (2, 3, 6), (3, 4, 130), (2, 2, 3), (2, 3, 512)]
# hw4 = 1 | 65: a second 64-lane block of the data gradient with one live lane | 576: two weight-gradient slices of 288 | 577: a
# ragged last slice
SMALLK_HW = [(2, 2), (4, 65), (48, 48), (4, 577)]


def _smallk_splits(O, HW):
    """cips_conv1x1_smallk_bwd_weight_splits restated: ceil(2048 / O) slices, each at least one 256-thread sweep of float4s"""
    return max(1, min(-(-2048 // O), (HW // 4) // 256))


assert any(_smallk_splits(O, H * W) > 1 for (_, _, O) in SMALLK_BCO for (H, W) in SMALLK_HW)


def _fp32_bound(cpu32, ref):
    """4 x the error torch's own float32 CPU evaluation shows against float64 (4: another summation order), floor 1e-6 (the
    project's bar for these ops)"""
    return max(1e-6, 4 * max_rel(cpu32, ref))


@pytest.mark.parametrize("H,W", SMALLK_HW)
@pytest.mark.parametrize("B,C,O", SMALLK_BCO)
def test_conv1x1_smallk_forward_and_both_gradients(B, C, O, H, W):
    """y = w x, dx = w^T dy, dw = sum_{b, p} dy x^T for the RGB input convolutions (at most 4 input channels): O off the four
    output channels of a workgroup and below the four waves of the data gradient, 1 / 2 / 3 / 4 input channels, pixel counts
    off the 64-lane and 256-thread blocks, one and two pixel slices of the weight gradient."""
    from cips3d_amd import ops, _lib
    d = dev()
    g = torch.Generator().manual_seed(B * 1000 + C * 100 + O + H * W)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(O, C, generator=g)
    dy = torch.randn(B, O, H, W, generator=g)
    S = _lib.load().cips_conv1x1_smallk_bwd_weight_splits(O, H * W)
    assert S == _smallk_splits(O, H * W)
    got = (ops.conv1x1_smallk(x.to(d), w.to(d)), ops.conv1x1_smallk_bwd_data(dy.to(d), w.to(d), C),
           ops.conv1x1_smallk_bwd_weight(dy.to(d), x.to(d)))
    eqs = ("oc,bchw->bohw", "oc,bohw->bchw", "bohw,bchw->oc")
    args = ((w, x), (w, dy), (dy, x))
    for what, out, eq, (a, b) in zip(("y", "dx", "dw"), got, eqs, args):
        ref = torch.einsum(eq, a.double(), b.double())
        bound = _fp32_bound(torch.einsum(eq, a, b), ref)
        e = max_rel(out, ref)
        print(f"{what} (S = {S}): max_rel {e:.3e}, bound {bound:.3e}")
        assert out.shape == ref.shape and e <= bound, what


# --------------------------------------------------------------------------------------
# avgpool2 (both directions) and axpby
# --------------------------------------------------------------------------------------
# the last one: 2.36 M outputs against the 8192 x 256 = 2.10 M threads of the capped grid -> a second grid-stride trip (38 MB)
@pytest.mark.parametrize("shape", [(2, 3, 2, 2), (3, 5, 6, 10), (1, 4, 64, 64), (36, 1, 512, 512)])
def test_avgpool2_and_its_transpose(shape):
    from cips3d_amd.discriminator import _AvgPool2Function
    d = dev()
    B, C, H, W = shape
    g = torch.Generator().manual_seed(H * W + B)
    x = torch.randn(*shape, generator=g) + 1                       # non-zero means: the two inner products below are far from 0
    gy = torch.randn(B, C, H // 2, W // 2, generator=g) + 1
    xd = x.to(d).requires_grad_(True)
    y = _AvgPool2Function.apply(xd, False)
    y.backward(gy.to(d))
    y, gx = y.detach().cpu(), xd.grad.cpu()
    a, b, c, e = x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]
    ref = (a.double() + b.double() + c.double() + e.double()) / 4
    assert y.shape == ref.shape and max_rel(y, ref) < 1e-6
    assert torch.equal(y, (0.5 * a + 0.5 * b) * 0.5 + (0.5 * c + 0.5 * e) * 0.5)         # the rounding order the kernel documents
    assert gx.shape == x.shape
    assert torch.equal(gx, (0.25 * gy).repeat_interleave(2, dim=2).repeat_interleave(2, dim=3))
    lhs, rhs = float((y.double() * gy.double()).sum()), float((x.double() * gx.double()).sum())
    print(f"adjoint: {lhs:.9e} {rhs:.9e}")
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs))


def test_avgpool2_refuses_odd_sizes():
    from cips3d_amd.discriminator import _AvgPool2Function
    d = dev()
    for shape in [(1, 2, 3, 4), (1, 2, 4, 5)]:
        with pytest.raises(RuntimeError, match="cips_avgpool2 failed with hipError 1"):
            _AvgPool2Function.apply(torch.zeros(*shape, device=d), False)


# 2 100 000 > 8192 x 256: the grid-stride loop takes a second trip for the first 2 848 elements (8.4 MB per tensor)
@pytest.mark.parametrize("n", [1, 255, 257, 2_100_000])
@pytest.mark.parametrize("a,b", [(2 ** -0.5, 2 ** -0.5), (0.75, 0.25)])
def test_axpby_is_the_separately_rounded_expression(a, b, n):
    from cips3d_amd.discriminator import _BlendFunction
    d = dev()
    g = torch.Generator().manual_seed(n)
    x, y = torch.randn(n, generator=g), torch.randn(n, generator=g)
    af, bf = torch.tensor(a, dtype=torch.float32), torch.tensor(b, dtype=torch.float32)
    out = _BlendFunction.apply(x.to(d), y.to(d), a, b).cpu()
    assert torch.equal(out, af * x + bf * y)
    out1 = _BlendFunction.apply(x.to(d), None, a, b).cpu()
    assert torch.equal(out1, af * x)
    xd, yd = x.to(d).requires_grad_(True), y.to(d).requires_grad_(True)
    up = torch.randn(n, generator=g)
    _BlendFunction.apply(xd, yd, a, b).backward(up.to(d))
    assert torch.equal(xd.grad.cpu(), af * up) and torch.equal(yd.grad.cpu(), bf * up)


# --------------------------------------------------------------------------------------
# rownorm: LayerNorm / LeakyReLU / PixelNorm rows of the mapping networks
# --------------------------------------------------------------------------------------
def _rownorm_inputs(rows, cols, mode):
    g = torch.Generator().manual_seed(rows * 100000 + cols * 10 + mode)
    x = torch.randn(rows, cols, generator=g) * 2 + 3               # a non-zero row mean: a wrong mean or tail mask shows
    gamma = torch.randn(cols, generator=g) if mode & 1 else None
    beta = torch.randn(cols, generator=g) if mode & 1 else None
    dy = torch.randn(rows, cols, generator=g)
    return x, gamma, beta, dy


def _rownorm_ref(x, gamma, beta, dy, mode, fused_ln=False):
    """float64 autograd: (out, pre-activation, dx, dgamma, dbeta).  LayerNorm is F.layer_norm(eps 1e-5) written out op by op
    (fused_ln: F.layer_norm itself): where the true dx is exactly zero — cols = 1 — the op-by-op form gives exactly zero,
    while F.layer_norm's fused backward leaves ~1e-14 of float64 rounding, which a RELATIVE error then divides by.  The two
    agree to float64 rounding (test_rownorm_reference_is_layer_norm)."""
    xd = x.double().requires_grad_(True)
    gd = gamma.double().requires_grad_(True) if gamma is not None else None
    bd = beta.double().requires_grad_(True) if beta is not None else None
    if mode & 4:
        pre = xd * torch.rsqrt((xd * xd).mean(dim=1, keepdim=True) + 1e-8)
    elif mode & 1 and fused_ln:
        pre = F.layer_norm(xd, (x.shape[1],), gd, bd, 1e-5)
    elif mode & 1:
        u = xd - xd.mean(dim=1, keepdim=True)
        pre = u * torch.rsqrt((u * u).mean(dim=1, keepdim=True) + 1e-5) * gd + bd
    else:
        pre = xd
    out = F.leaky_relu(pre, 0.2) if mode & 2 else pre
    out.backward(dy.double())
    return out.detach(), pre.detach(), xd.grad, (gd.grad if gd is not None else None), (bd.grad if bd is not None else None)


ROWNORM_COLS = [1, 63, 64, 65, 255, 256, 257, 1000, 1024]
ROWNORM_ROWS = [1, 3, 70]
ROWNORM_MODES = [0, 1, 2, 3, 4]                     # bit 0 LayerNorm, bit 1 LeakyReLU(0.2), 4 PixelNorm


def test_rownorm_reference_is_layer_norm():
    """CPU: the op-by-op float64 LayerNorm of _rownorm_ref is F.layer_norm(eps 1e-5), outputs and all three gradients, to
    float64 rounding measured against each tensor's own scale (rstd reaches 316 at cols = 1, hence the scale of dx)"""
    for mode in (1, 3):
        for cols in ROWNORM_COLS:
            for rows in ROWNORM_ROWS:
                args = _rownorm_inputs(rows, cols, mode)
                a, b = _rownorm_ref(*args, mode), _rownorm_ref(*args, mode, fused_ln=True)
                scale = 316 * float(args[3].abs().max()) * float(args[1].abs().max())
                for i, (p, q) in enumerate(zip(a, b)):
                    assert float((p - q).abs().max()) <= 1e-12 * max(scale, float(q.abs().max())), (mode, cols, rows, i)


def test_rownorm_inputs_stay_clear_of_the_activation_kink():
    """CPU part of the gradient comparison's premise: of the seeded inputs' float64 pre-activations fewer than 1 in 10 000
    lie within 1e-6 of zero (where a float32 kernel may take the other branch of LeakyReLU)"""
    near = total = 0
    for mode in (2, 3):
        for cols in ROWNORM_COLS:
            for rows in ROWNORM_ROWS:
                x, gamma, beta, dy = _rownorm_inputs(rows, cols, mode)
                pre = _rownorm_ref(x, gamma, beta, dy, mode)[1]
                near += int((pre.abs() < 1e-6).sum()); total += pre.numel()
    assert near * 10000 < total, (near, total)


@pytest.mark.parametrize("mode", ROWNORM_MODES)
@pytest.mark.parametrize("rows", ROWNORM_ROWS)
@pytest.mark.parametrize("cols", ROWNORM_COLS)
def test_rownorm_forward_backward(cols, rows, mode):
    """ops.RowNormFunction against float64 autograd: every tail of the 256-thread forward and of the 64-lane backward, one
    to 1024 columns, all five modes.  Bars: those of test_mapping_networks_on_hip_match_torch_modules, whose arithmetic
    this is.  cols = 1 with LayerNorm: variance 0, rstd = 1 / sqrt(1e-5), in the kernel and in the reference alike, and dx is
    exactly zero in both.  cols = 1 with PixelNorm: y = +-1 to 1e-9 and the true dx = dy 1e-8 (x^2 + 1e-8)^-1.5 is ~1e-9 of
    dy / |x| — the difference 1 - y^2, which dx = r (dy - y mean(dy y)) evaluated as written loses in float32 (rel_err 1.0 / 1.0 /
    0.78 at 1 / 3 / 70 rows before the kernel took each column's own term out of the row sums)."""
    from cips3d_amd import ops
    d = dev()
    x, gamma, beta, dy = _rownorm_inputs(rows, cols, mode)
    out_ref, pre, dx_ref, dgamma_ref, dbeta_ref = _rownorm_ref(x, gamma, beta, dy, mode)
    xd = x.to(d).requires_grad_(True)
    gd = gamma.to(d).requires_grad_(True) if gamma is not None else None
    bd = beta.to(d).requires_grad_(True) if beta is not None else None
    out = ops.RowNormFunction.apply(xd, gd, bd, mode)
    out.backward(dy.to(d))
    e = rel_err(out, out_ref)
    print(f"out rel_err {e:.3e}")
    assert out.shape == out_ref.shape and e < 2e-6
    # elements whose pre-activation is within 1e-6 of the kink may be gated the other way: left out (with their columns of
    # d gamma / d beta), and there must be next to none of them
    keep = torch.ones_like(pre, dtype=torch.bool) if not (mode & 2) else pre.abs() >= 1e-6
    assert int((~keep).sum()) * 10000 < max(keep.numel(), 10000)
    e = rel_err(xd.grad.cpu()[keep], dx_ref[keep])
    print(f"dx rel_err {e:.3e}")
    assert xd.grad.shape == x.shape and e < 2e-5
    if mode & 1:
        colkeep = keep.all(dim=0)
        eg, eb = rel_err(gd.grad.cpu()[colkeep], dgamma_ref[colkeep]), rel_err(bd.grad.cpu()[colkeep], dbeta_ref[colkeep])
        print(f"dgamma rel_err {eg:.3e}, dbeta rel_err {eb:.3e}")
        assert gd.grad.shape == gamma.shape and eg < 2e-5 and eb < 2e-5
