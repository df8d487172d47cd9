"""GPU: the INR head in INR_MODE "bf16" (single pass on the hi planes in every GEMM of the head, forward and backward) end to
end on the golden fixtures, and its plumbing (graph capture, side-stream gradient tail, generator_v1, switching back).

Yardstick, computed here on the host: the fp64 oracle with the head's LeakyReLU gates pinned, once plain ("exact") and once with
the torch.bmm of its modulated FC replaced by an autograd Function that rounds both operands to bf16 in the forward and the incoming
gradient and both saved operands in the backward ("emulation": the AMP-class arithmetic this mode is, in fp64 otherwise).  The
product is held to the emulation's own distance from exact — image error at most 1.5 x the emulation's + 1e-5, median parameter
gradient error (over the parameters the head's arithmetic reaches) at most 1.25 x the emulation's median, largest at most 2 x the
emulation's largest + 2e-4 — margins within which a second realisation of the same arithmetic (the emulation evaluated in fp32)
stays (image ratio 0.85-1.13, median ratio 0.99-1.03, largest-to-largest up to 1.66).  Product and emulation are not compared
with each other: bf16 rounding is chaotic enough that two correct evaluations differ by as much as each differs from exact.
And the mode must be in effect: the product's median gradient error is at least half the emulation's (exact fp32 arithmetic,
which is what this mode string selected before the mode existed, sits three orders of magnitude lower)."""
import statistics

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, load_gates, seeded_generator, pack_bitplane, unpack_bitplane
from oracle import cips3d_oracle as orc
from test_generator_v1_cpu import seeded_generator_v1

pytestmark = pytest.mark.gpu
CASES = ["g_r16_hier", "g_r8_flat_noise", "g_r8_hier_noise", "g_r8_freeze", "g_r16_part"]


@pytest.fixture
def bf16_mode():
    from cips3d_amd import ops
    old = ops.INR_MODE
    ops.INR_MODE = "bf16"
    yield
    ops.INR_MODE = old


def _bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _BmmBf16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        xr, wr = _bf(x), _bf(w)
        ctx.save_for_backward(xr, wr)
        return torch.bmm(xr, wr)

    @staticmethod
    def backward(ctx, g):
        xr, wr = ctx.saved_tensors
        gr = _bf(g)
        return torch.bmm(gr, wr.transpose(1, 2)), torch.bmm(xr.transpose(1, 2), gr)


def _mod_fc_bf16(sd, prefix, x, style, eps=1e-8):
    """orc.mod_fc with its product taken on bf16-rounded operands"""
    s = F.linear(style, sd[prefix + "modulation.weight"], sd[prefix + "modulation.bias"])
    w = sd[prefix + "weight"] * (s.unsqueeze(-1) + 1)
    w = w * torch.rsqrt(w.pow(2).sum([1]) + eps).unsqueeze(1)
    return _BmmBf16.apply(x, w)


def _v1_oracle(mp):
    """the oracle's SIREN takes its colour FiLM style from nerf_rgb_mapping(w_inr): generator_v1's composition
    (as in test_gpu_generator_v1.test_afhq_recipe_geometry_r64_e96_forward_backward_vs_oracle)"""
    captured = {}
    real_mapping_inr = orc.mapping_inr

    def mapping_inr(sd, z, *a, **k):
        captured["w_inr"] = real_mapping_inr(sd, z, *a, **k)
        return captured["w_inr"]

    def siren_v1(sd, points, w_nerf, prefix="siren."):
        w_rgb = F.linear(captured["w_inr"], sd["nerf_rgb_mapping.weight"], sd["nerf_rgb_mapping.bias"])
        x = points * (2 / 0.24)
        idx = 0
        while prefix + f"network.{idx}.linear.weight" in sd:
            x = orc.film(sd, prefix + f"network.{idx}.", x, w_nerf)
            idx += 1
        sigma = F.linear(x, sd[prefix + "final_layer.weight"], sd[prefix + "final_layer.bias"])
        c = orc.film(sd, prefix + "color_layer_sine.", x, w_rgb)
        feat = F.linear(c, sd[prefix + "color_layer_linear.0.weight"], sd[prefix + "color_layer_linear.0.bias"])
        return torch.cat([feat, sigma], dim=-1)

    mp.setattr(orc, "mapping_inr", mapping_inr)
    mp.setattr(orc, "siren", siren_v1)


def _oracle64(fix, gates, emulate, make=seeded_generator, backward=True):
    """fp64 oracle, gates pinned (or recorded: gates=None) -> imgs, {name: grad}, tape"""
    G64 = make(fix["seed"], freeze=fix["freeze"]).double()
    kw = fix["G_kwargs"]
    dbl = lambda dd: {k: (v.double() if torch.is_floating_point(v) else v) for k, v in dd.items()}
    tape = orc.GateTape(pin=gates)
    real = orc.mod_fc
    torch.set_default_dtype(torch.float64)
    try:
        if emulate:
            orc.mod_fc = _mod_fc_bf16
        with orc.gate_tape(tape):
            o64 = orc.generator_forward(dict(G64.named_parameters()), dbl(fix["zs"]), dbl(fix["rand"]), fix["img_size"],
                                        kw["fov"], kw["ray_start"], kw["ray_end"], kw["num_steps"], kw["h_stddev"],
                                        kw["v_stddev"], kw["hierarchical_sample"], nerf_noise=fix["nerf_noise"],
                                        return_aux_img=fix["aux"], freeze_nerf=fix["freeze"],
                                        grad_points=fix.get("grad_points"))
        tape.done()
        if backward:
            (o64["imgs"] * fix["G0"].double()).sum().backward()
    finally:
        orc.mod_fc = real
        torch.set_default_dtype(torch.float32)
    return o64["imgs"].detach(), {n: p.grad for n, p in G64.named_parameters()}, tape


def _run_product(G, fix, d, pin=None, rec=None):
    from cips3d_amd import ops
    zs = {k: v.to(d) for k, v in fix["zs"].items()}
    rand = {k: v.to(d) for k, v in fix["rand"].items()}
    for p in G.parameters():
        p.grad = None
    with ops.gate_debug(pin=pin, rec=rec):
        imgs, _ = G(zs, img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"],
                    grad_points=fix.get("grad_points"), forward_points=None, rand_override=rand, **fix["G_kwargs"])
    (imgs * fix["G0"].to(d)).sum().backward()
    torch.cuda.synchronize()
    return imgs.detach().cpu().double(), {n: (None if p.grad is None else p.grad.detach().cpu().double()) for n, p in G.named_parameters()}


def _img_err(imgs, exact):
    return float((imgs - exact).abs().max() / exact.abs().max())


def _grad_errs(grads, exact):
    """{name: relative L2 error against exact} over the parameters exact has a non-zero gradient for"""
    out = {}
    for n, t in exact.items():
        if t is None or float(t.abs().max()) == 0.0:
            assert grads.get(n) is None or float(grads[n].abs().max()) == 0.0, n
            continue
        assert grads[n] is not None, n
        out[n] = float((grads[n].reshape(-1) - t.reshape(-1)).norm() / t.norm())
    return out


def _bars(tag, what, imgs, grads, exact_imgs, exact_grads, e_img, e_err, lower=True):
    """the pinned / free-running bars of the module docstring; e_img, e_err: the emulation's image error and gradient errors"""
    p_img, p_err = _img_err(imgs, exact_imgs), _grad_errs(grads, exact_grads)
    reach = [n for n, e in e_err.items() if e > 0.0 and n in p_err]              # the parameters the head's arithmetic reaches
    assert len(reach) >= 20, len(reach)
    e_med, p_med = statistics.median(e_err[n] for n in reach), statistics.median(p_err[n] for n in reach)
    e_max, p_max = max(e_err.values()), max(p_err.values())
    worst = max(p_err, key=p_err.get)
    print(f"{tag} [bf16] {what}: image error / max|img| {p_img:.3e} (emulation {e_img:.3e}, ratio {p_img / e_img:.2f}); gradient error "
          f"median {p_med:.3e} (emulation {e_med:.3e}, ratio {p_med / e_med:.2f}), largest {p_max:.3e} at {worst} (emulation "
          f"{e_max:.3e}, ratio {p_max / e_max:.2f}); {len(reach)} of {len(e_err)} parameters reached")
    assert torch.isfinite(imgs).all() and all(torch.isfinite(g).all() for g in grads.values() if g is not None)
    assert p_img <= 1.5 * e_img + 1e-5, (p_img, e_img)
    assert p_med <= 1.25 * e_med, (p_med, e_med)
    assert p_max <= 2.0 * e_max + 2e-4, (p_max, e_max, worst)
    if lower:
        assert p_med >= 0.5 * e_med, ("the single-pass mode is not in effect", p_med, e_med)


def _pinned_and_free(tag, fix, ref_gates, G, make, free=True):
    d = torch.device("cuda:0")
    exact_imgs, exact_grads, _ = _oracle64(fix, ref_gates, False, make)
    emu_imgs, emu_grads, _ = _oracle64(fix, ref_gates, True, make)
    e_img, e_err = _img_err(emu_imgs, exact_imgs), _grad_errs(emu_grads, exact_grads)
    imgs, grads = _run_product(G, fix, d, pin=[pack_bitplane(g) for g in ref_gates])
    _bars(tag, "pinned", imgs, grads, exact_imgs, exact_grads, e_img, e_err)
    if not free:
        return
    rec = []
    imgs, grads = _run_product(G, fix, d, rec=rec)
    own = [unpack_bitplane(p.cpu()) for p in rec]
    assert [tuple(g.shape) for g in own] == [tuple(g.shape) for g in ref_gates]
    flips = sum(int((a != b).sum()) for a, b in zip(own, ref_gates))
    _, _, tape = _oracle64(fix, None, True, make, backward=False)          # the gates the unpinned emulation takes
    emu_flips = sum(int((a.reshape(b.shape) != b).sum()) for a, b in zip(tape.rec, ref_gates))
    total = sum(g.numel() for g in ref_gates)
    print(f"{tag} [bf16] free: {flips} of {total} gates differ from the reference's (unpinned emulation: {emu_flips})")
    assert flips <= 4 + 2 * emu_flips, (flips, emu_flips)
    own_imgs, own_grads, _ = _oracle64(fix, own, False, make)
    _bars(tag, "free", imgs, grads, own_imgs, own_grads, e_img, e_err, lower=False)


@pytest.mark.parametrize("tag", CASES)
def test_bf16_head_stays_within_the_emulations_distance_from_exact(tag, bf16_mode):
    fix = load_golden(tag)
    G = seeded_generator(fix["seed"], freeze=fix["freeze"], device=torch.device("cuda:0"))
    _pinned_and_free(tag, fix, load_gates(tag), G, seeded_generator)


def test_generator_v1_inherits_the_mode(bf16_mode, monkeypatch):
    tag = "g_v1_r16_hier"
    fix = load_golden(tag)
    _v1_oracle(monkeypatch)
    G = seeded_generator_v1(fix["seed"], freeze=fix["freeze"], device=torch.device("cuda:0"))
    _pinned_and_free(tag, fix, load_gates(tag), G, seeded_generator_v1, free=False)


def test_captured_step_in_bf16_mode_replays_the_eager_step(bf16_mode):
    """as tests/test_gpu_graph.py requires of the default mode; the mode is fixed at capture: switching it afterwards does not
    change what the graph replays"""
    from cips3d_amd import ops
    from cips3d_amd.graph import capture
    fix = load_golden("g_r8_flat_noise")
    d = torch.device("cuda:0")
    G = seeded_generator(fix["seed"], freeze=fix["freeze"], device=d)
    zs = {k: v.to(d) for k, v in fix["zs"].items()}
    rand = {k: v.to(d) for k, v in fix["rand"].items()}
    G0 = fix["G0"].to(d)
    params = [p for p in G.parameters() if p.requires_grad]
    img_buf = torch.zeros_like(fix["imgs"], device=d)

    def step():
        for p in params:
            p.grad = None
        imgs, _ = G(zs, img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"], grad_points=None,
                    forward_points=None, rand_override=rand, **fix["G_kwargs"])
        (imgs * G0).sum().backward()
        img_buf.copy_(imgs.detach())

    step()
    torch.cuda.synchronize()
    eager_imgs = img_buf.clone()
    eager = [None if p.grad is None else p.grad.detach().clone() for p in params]
    cs = capture(step, warmup=1, params=params)
    ops.INR_MODE = "bf16x3"
    for _ in range(2):
        cs()
    torch.cuda.synchronize()
    assert torch.equal(img_buf, eager_imgs)
    for p, g in zip(params, eager):
        assert (p.grad is None) == (g is None)
        if g is not None:
            assert torch.allclose(p.grad, g, rtol=1e-6, atol=1e-9), float((p.grad - g).abs().max())
    step()                                     # eager, in the default mode now: other images
    torch.cuda.synchronize()
    assert not torch.equal(img_buf, eager_imgs)


@pytest.mark.parametrize("tag", ["g_r8_flat_noise", "g_r16_hier", "g_r8_freeze"])
def test_weight_gradient_tail_on_the_side_stream_in_bf16_mode(tag, bf16_mode):
    """as test_gpu_generator.test_weight_gradient_tail_on_the_side_stream_gives_the_same_gradients requires of the default mode"""
    from cips3d_amd import ops
    fix = load_golden(tag)
    d = torch.device("cuda:0")
    G = seeded_generator(fix["seed"], freeze=fix["freeze"], device=d)
    zs = {k: v.to(d) for k, v in fix["zs"].items()}
    rand = {k: v.to(d) for k, v in fix["rand"].items()}
    calls = []
    orig = ops.inr_head_with_ports
    ops.inr_head_with_ports = lambda *a, **k: (calls.append(a[3]), orig(*a, **k))[1]
    out = {}
    keep = ops.INR_TAIL
    try:
        for mode in ("main", "side", "side"):
            ops.INR_TAIL = mode
            for p in G.parameters():
                p.grad = None
            n0 = len(calls)
            imgs, _ = G(zs, img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"],
                        grad_points=None, forward_points=None, rand_override=rand, **fix["G_kwargs"])
            (imgs * fix["G0"].to(d)).sum().backward()
            torch.cuda.synchronize()
            assert (len(calls) - n0 == 1) == (mode == "side" and not fix["freeze"])
            assert all(ports.waited for ports in calls[n0:])
            assert not ops._TAIL_GATE
            out.setdefault(mode, []).append((imgs.detach().clone(), {n: p.grad.clone() for n, p in G.named_parameters() if p.grad is not None}))
    finally:
        ops.INR_TAIL = keep
        ops.inr_head_with_ports = orig
    (im_m, g_m), (im_s, g_s), (im_s2, g_s2) = out["main"][0], out["side"][0], out["side"][1]
    assert torch.equal(im_m, im_s) and torch.equal(im_s, im_s2)
    assert g_m.keys() == g_s.keys() == g_s2.keys()
    for k in g_m:
        assert torch.equal(g_s[k], g_s2[k]), k
        scale = float(g_m[k].abs().max()) + 1e-30
        assert float((g_m[k] - g_s[k]).abs().max()) <= 5e-6 * scale, (k, float((g_m[k] - g_s[k]).abs().max()) / scale)


def test_switching_back_reproduces_the_default_mode_bit_for_bit():
    """no state left behind: default, bf16, default in one process — the first and the third images and gradients are identical,
    the second differ"""
    from cips3d_amd import ops
    fix = load_golden("g_r16_hier")
    d = torch.device("cuda:0")
    G = seeded_generator(fix["seed"], freeze=fix["freeze"], device=d)
    assert ops.INR_MODE == "bf16x3"
    res = []
    try:
        for mode in ("bf16x3", "bf16", "bf16x3"):
            ops.INR_MODE = mode
            res.append(_run_product(G, fix, d))
    finally:
        ops.INR_MODE = "bf16x3"
    assert torch.equal(res[0][0], res[2][0]) and not torch.equal(res[0][0], res[1][0])
    for n, g in res[0][1].items():
        assert (g is None) == (res[2][1][n] is None)
        if g is not None:
            assert torch.equal(g, res[2][1][n]), n
