"""GPU: the discriminator in CONV_MODE "bf16" (single pass on the hi planes in every implicit-GEMM convolution that qualifies,
forward and both gradients) end to end on the golden fixtures, and its plumbing (switching back, graph capture).

Yardstick, computed here on the host: the fp64 oracle's full d_loss (test_discriminator_cpu.d_loss_grads: logits, R1 penalty
through the double-backward graph, parameter gradients) with the reference's LeakyReLU gates pinned, once plain ("exact") and once
with orc.conv_layer re-stated so that its convolution is test_gpu_conv_bf16.EmuConv — the three mutually differentiating
Functions that round the operands of every convolution GEMM to bf16 — wherever the product goes single-pass ("emulation"):
forward and data gradient where the contraction channels are a multiple of 64 (every EqualConv2d of the fixtures but conv_in:
512 / 256 channels), the weight gradient where ops.conv2d_bf16_wgrad_declines says it is not declined.  The Blur, the conv_in
layers, EqualLinear and the activations stay exact.

Product and emulation are each compared with exact, never with each other (bf16 rounding is chaotic enough that two correct
evaluations differ by as much as each differs from exact).  The product's logits, R1 input gradient and parameter gradients
(median and largest relative L2) stay within MARGIN x the emulation's own distance from exact.  MARGIN comes from a second
realisation of the same arithmetic — the emulation evaluated in fp32 instead of fp64 — measured on the CPU over the three
fixtures as (fp32 emulation's error) / (fp64 emulation's error), each against exact (the fp64 emulation's own errors: logits
2.1e-3 ... 3.2e-2 of the largest logit, R1 input gradient 3.7e-3 ... 4.7e-3, parameter gradients median 3.2e-3 ... 3.3e-3,
largest 4.2e-3 ... 4.6e-3; exact fp32 arithmetic sits at 4e-7 ... 1.8e-6):
                      logits   R1 input gradient   median parameter gradient   largest parameter gradient
    d_r16              0.86         1.07                   1.01                        1.03
    d_r16_aux_alpha    1.02         1.00                   1.01                        0.97
    d_r16_diffaug      0.79         0.99                   0.99                        1.02
1.25 x the largest of them is 1.33: MARGIN is the floor, 1.5.
And the mode must be in effect: the product's median parameter-gradient error is at least half the emulation's (exact fp32,
which the string "bf16" selected before the mode existed, sits orders of magnitude lower)."""
import math
import statistics

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, load_gates, max_rel, D_CFG, ReplayDraws
from oracle import cips3d_oracle as orc
from test_discriminator_cpu import d_loss_grads
from test_gpu_conv_bf16 import EmuConv

pytestmark = pytest.mark.gpu
TAGS = ["d_r16", "d_r16_aux_alpha", "d_r16_diffaug"]

# (fp32 emulation error) / (fp64 emulation error), measured on the CPU (module docstring): tag -> (logits, R1 input gradient,
# median parameter gradient, largest parameter gradient)
RATIOS = {
    "d_r16": (0.860, 1.066, 1.007, 1.029),
    "d_r16_aux_alpha": (1.015, 0.997, 1.008, 0.971),
    "d_r16_diffaug": (0.793, 0.985, 0.993, 1.020),
}
MARGIN = max(1.5, 1.25 * max(max(v) for v in RATIOS.values()))


def _single_pass_rule(x_shape, w_shape, stride, pad):
    """what the product runs single-pass, re-stated from the issue's eligibility (not read from the product): 64-channel
    multiples and two 64-deep k-tiles in the contraction; the weight gradient over B * Ho * Wo pixels in 64-row k-tiles"""
    B, C, H, W = x_shape
    O, _, k, _ = w_shape
    Ho = (H + 2 * pad - k) // stride + 1
    fwd = C % 64 == 0 and k * k * C >= 128
    dgrad = O % 64 == 0 and (O >= 128 if stride == 2 else k * k * O >= 128)
    wgrad = (B * Ho * Ho) % 64 == 0 and B * Ho * Ho >= 128
    return fwd, dgrad, wgrad


def conv_layer_bf16(sd, prefix, x, k, downsample=False, activate=True, bias=True):
    """orc.conv_layer with its convolution on bf16-rounded operands where the product goes single-pass"""
    w = sd[prefix + "equal_conv.weight"]
    cin = w.shape[1]
    scale = 1 / math.sqrt(cin * k * k)
    if downsample:
        p = (4 - 2) + (k - 1)
        x = orc.upfirdn2d(x, sd.get(prefix + "down_blur.kernel", orc._blur_kernel()), pad=((p + 1) // 2, p // 2))
        stride, padding = 2, 0
    else:
        stride, padding = 1, (k - 1) // 2
    cb = sd.get(prefix + "equal_conv.bias") if (bias and not activate) else None
    rnd = _single_pass_rule(tuple(x.shape), tuple(w.shape), stride, padding)
    if cin % 32:                                   # conv_in: the streaming RGB kernels, exact
        x = F.conv2d(x, w * scale, bias=cb, stride=stride, padding=padding)
    else:
        x = EmuConv.apply(x, w * scale, stride, padding, rnd)
        if cb is not None:
            x = x + cb.view(1, -1, 1, 1)
    if activate:
        x = orc.fused_leaky_relu(x, sd[prefix + "flrelu.bias"]) if bias else F.leaky_relu(x, 0.2) * math.sqrt(2)
    return x


def oracle(fix, gates, emulate, dtype=torch.float64):
    """full d_loss on the oracle, gates pinned -> logits, R1 input gradient, {name: parameter gradient} (fp64 tensors)"""
    tape = orc.GateTape(pin=gates)
    real = orc.conv_layer
    try:
        if emulate:
            orc.conv_layer = conv_layer_bf16
        out, g, grads = d_loss_grads(fix, dtype, tape)
    finally:
        orc.conv_layer = real
    tape.done()
    return out.double(), g.double(), {n: (None if t is None else t.double()) for n, t in grads.items()}


def grad_errs(grads, exact):
    """{name: relative L2 error against exact} over the parameters exact has a non-zero gradient for"""
    out = {}
    for n, t in exact.items():
        if t is None or float(t.abs().max()) == 0.0:
            assert grads.get(n) is None or float(grads[n].abs().max()) == 0.0, n
            continue
        assert grads[n] is not None, n
        out[n] = float((grads[n].reshape(-1) - t.reshape(-1)).norm() / t.norm())
    return out


def errors(run, exact):
    """(logits max_rel, R1 input gradient max_rel, median and largest parameter-gradient error, its name) of `run` against `exact`"""
    ge = grad_errs(run[2], exact[2])
    worst = max(ge, key=ge.get)
    return max_rel(run[0], exact[0]), max_rel(run[1], exact[1]), statistics.median(ge.values()), ge[worst], worst


@pytest.fixture
def bf16_mode(monkeypatch):
    from cips3d_amd import discriminator as dm
    assert dm.CONV_MODE == "bf16x3"
    monkeypatch.setattr(dm, "CONV_MODE", "bf16")


def _make_D(fix, d):
    from cips3d_amd.discriminator import Discriminator_MultiScale_Aux
    torch.manual_seed(fix["seed"])
    return Discriminator_MultiScale_Aux(**dict(D_CFG, diffaug=fix.get("diffaug", False))).to(d)


def _run_product(D, fix, d, pin=None):
    from cips3d_amd import discriminator as dm
    for p in D.parameters():
        p.grad = None
    x = fix["x"].to(d).requires_grad_(True)
    with dm.gate_debug(pin=pin):
        if fix.get("diffaug"):
            with ReplayDraws(fix["draws"]):
                out, _, _ = D(x, alpha=fix["alpha"], use_aux_disc=fix["use_aux"])
        else:
            out, _, _ = D(x, alpha=fix["alpha"], use_aux_disc=fix["use_aux"])
    grad_real, = torch.autograd.grad(outputs=out.sum(), inputs=x, create_graph=True)
    loss = F.softplus(-out).mean() + 0.5 * 10. * grad_real.flatten(1).pow(2).sum(1).mean()
    loss.backward()
    torch.cuda.synchronize()
    return (out.detach().cpu().double(), grad_real.detach().cpu().double(),
            {n: (None if p.grad is None else p.grad.detach().cpu().double()) for n, p in D.named_parameters()})


@pytest.mark.parametrize("tag", TAGS)
def test_bf16_discriminator_stays_within_the_emulations_distance_from_exact(tag, bf16_mode):
    fix, gates = load_golden(tag), load_gates(tag)
    d = torch.device("cuda:0")
    exact = oracle(fix, gates, False)
    emu = oracle(fix, gates, True)
    e_out, e_g, e_med, e_max, e_worst = errors(emu, exact)
    got = _run_product(_make_D(fix, d), fix, d, pin=gates)
    p_out, p_g, p_med, p_max, p_worst = errors(got, exact)
    print(f"{tag} [bf16]: logits max_rel {p_out:.3e} (emulation {e_out:.3e}, ratio {p_out / e_out:.2f}); R1 input gradient {p_g:.3e} "
          f"(emulation {e_g:.3e}, ratio {p_g / e_g:.2f}); parameter gradients median {p_med:.3e} (emulation {e_med:.3e}, ratio "
          f"{p_med / e_med:.2f}), largest {p_max:.3e} at {p_worst} (emulation {e_max:.3e} at {e_worst}, ratio {p_max / e_max:.2f}); "
          f"margin {MARGIN:.2f}")
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    assert all(torch.isfinite(t).all() for t in got[2].values() if t is not None)
    assert MARGIN <= 2.0, "a margin above 2 x is a finding, not a tolerance"
    assert p_out <= MARGIN * e_out, (p_out, e_out)
    assert p_g <= MARGIN * e_g, (p_g, e_g)
    assert p_med <= MARGIN * e_med, (p_med, e_med)
    assert p_max <= MARGIN * e_max, (p_max, e_max, p_worst)
    assert p_med >= 0.5 * e_med, ("the single-pass mode is not in effect", p_med, e_med)


def test_leaving_the_mode_reproduces_the_default_mode_bit_for_bit(monkeypatch):
    """no stale planes and no stale mode: bf16x3, bf16, bf16x3 on one network in one process — the first and the third run are
    identical in every logit, input gradient and parameter gradient; the second differs.  Free-running gates (so the fused
    bias + LeakyReLU epilogue and the planes-only gradients run)"""
    from cips3d_amd import discriminator as dm
    fix = load_golden("d_r16")
    d = torch.device("cuda:0")
    D = _make_D(fix, d)
    assert dm.CONV_MODE == "bf16x3"
    res = []
    for mode in ("bf16x3", "bf16", "bf16x3"):
        monkeypatch.setattr(dm, "CONV_MODE", mode)
        res.append(_run_product(D, fix, d))
    assert torch.equal(res[0][0], res[2][0]) and torch.equal(res[0][1], res[2][1])
    assert not torch.equal(res[0][0], res[1][0])
    for n, g in res[0][2].items():
        assert (g is None) == (res[2][2][n] is None)
        if g is not None:
            assert torch.equal(g, res[2][2][n]), n


def test_captured_d_step_in_bf16_mode_replays_the_eager_values(bf16_mode):
    """D forward + R1 + backward captured with torch.cuda.graph in "bf16" mode: a replay gives the eager run's logits, R1
    input gradient and parameter gradients bit for bit (weight planes are built inside the capture: discriminator._cached)"""
    fix = load_golden("d_r16")
    d = torch.device("cuda:0")
    D = _make_D(fix, d)
    params = [p for p in D.parameters()]
    x_static = fix["x"].to(d)
    out_buf = torch.zeros(fix["out"].shape, device=d)
    gr_buf = torch.zeros_like(x_static)

    def step():
        x = x_static.detach().requires_grad_(True)
        out, _, _ = D(x, alpha=fix["alpha"], use_aux_disc=fix["use_aux"])
        gr, = torch.autograd.grad(outputs=out.sum(), inputs=x, create_graph=True)
        (F.softplus(-out).mean() + 5.0 * gr.flatten(1).pow(2).sum(1).mean()).backward()
        out_buf.copy_(out.detach())
        gr_buf.copy_(gr.detach())

    def zero():
        for p in params:
            p.grad = torch.zeros_like(p) if p.grad is None else p.grad.zero_()

    zero()
    step()
    torch.cuda.synchronize()
    eager = (out_buf.clone(), gr_buf.clone(), [p.grad.clone() for p in params])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        zero()
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for p in params:
            p.grad.zero_()
        step()
    out_buf.zero_(); gr_buf.zero_()
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_buf, eager[0]) and torch.equal(gr_buf, eager[1])
    for p, g in zip(params, eager[2]):
        assert torch.equal(p.grad, g)
