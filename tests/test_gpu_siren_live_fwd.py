"""GPU: the live samples of the flat path decided in the FORWARD pass (ops.SIREN_LIVE_FWD): one rule on sigma + noise
(cips_live_points_clamp), the compositing backward that writes the listed samples only (cips_composite_bwd_listed), the
finalisation that sums an image's rows itself (cips_siren_bwd_x3_finalize_segments), and RayMarchFunction / the generator with
the lists and the EVEN plan made on another stream behind the march.  In file order: the list against a numpy evaluation of the
rule, the list against the backward-time mask, the compositing, the finalisation, then the switch end to end and under capture."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, seeded_generator
from test_gpu_siren_bwd_live import TOL, P_, dev, _siren_setup

pytestmark = pytest.mark.gpu

SENTINEL = 1234.5


# --------------------------------------------------------------------------------------
# inputs: b = 3 images; image 0 has every sigma below -3 (no noise draw opens it), image 1 every sigma above 3, image 2 mixed
# --------------------------------------------------------------------------------------
SHAPES = [(8, 8, 24), (5, 8, 5)]           # two waves of ray segments, P = 1536; a partial wave, P = 200 (P % 16 = 8)
CASES = [(ns, fl) for ns in (0.0, 0.3) for fl in (0, 1, 2, 3)]


def _inputs(H, W, S, seed=41):
    b, n = 3, H * W
    g = torch.Generator().manual_seed(seed + S)
    feat = torch.randn(b, n, S, 32, generator=g)
    sig = torch.randn(b, n, S, generator=g)
    sig[0] = -3.0 - sig[0].abs()
    sig[1] = 3.0 + sig[1].abs()
    sig[2] += 0.43
    z = torch.linspace(0.88, 1.12, S).view(1, 1, S) + (torch.rand(b, n, S, generator=g) - 0.5) * (0.1 / S)
    noise = torch.randn(b, n, S, generator=g)
    dfea = torch.randn(b, n, 32, generator=g)
    return [t.to(dev()).contiguous() for t in (feat, sig, z, noise, dfea)]


def _rule(sig, noise, noise_std, flags):
    """the rule in numpy: x = sigma + noise * std in one rounding (the kernel's multiply-add is fused), live = !(x <= 0), plus
    the ray's last sample under last_back -> bool (b, n, S), x"""
    x = sig.cpu().numpy().astype(np.float64)
    if noise_std:
        x = x + noise.cpu().numpy().astype(np.float64) * np.float64(np.float32(noise_std))
    x = x.astype(np.float32)
    live = ~(x <= 0)
    if flags & 1:
        live[..., -1] = True
    return live, x


def _list(sig, noise, noise_std, flags, clamp="relu"):
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    b, n, S = sig.shape
    idx = torch.full((b, n * S), -7, dtype=torch.int32, device=dev())
    count = torch.full((b,), -7, dtype=torch.int32, device=dev())
    _lib.check(lib.cips_live_points_clamp(P_(sig), P_(noise) if noise_std else None, float(noise_std), b, n, S, ops._CLAMP[clamp],
                                          flags, P_(idx), P_(count), ops._stream()), "cips_live_points_clamp")
    return idx, count


def _listed_mask(idx, count, P):
    m = torch.zeros(idx.shape[0], P, dtype=torch.bool)
    for b in range(idx.shape[0]):
        m[b, idx[b, :int(count[b])].cpu().long()] = True
    return m


def _composite(inp, S, noise_std, flags, form, clamp="relu"):
    """form "dense" / "live" / "listed" on outputs pre-filled with SENTINEL -> dfeat (b,n,S,32), dsig (b,n,S), mask or None"""
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    feat, sig, z, noise, dfea = inp
    b, n = sig.shape[:2]
    R = b * n
    dfeat = torch.full((b, n, S, 32), SENTINEL, device=dev())
    dsig = torch.full((b, n, S), SENTINEL, device=dev())
    nz = P_(noise) if noise_std else None
    cm = ops._CLAMP[clamp]
    if form == "listed":
        _lib.check(lib.cips_composite_bwd_listed(P_(feat), P_(sig), P_(z), nz, float(noise_std), P_(dfea), P_(dfeat), P_(dsig), R, S,
                                                 cm, flags, ops._stream()), "cips_composite_bwd_listed")
        return dfeat, dsig, None
    head = (P_(feat), P_(sig), P_(z), None, None, None, nz, float(noise_std), None, P_(dfea), P_(dfeat), P_(dsig), None, None)
    tail = (R, S, cm, flags, None, ops._stream())
    if form == "live":
        mask = torch.full((b, n, S), 7, dtype=torch.uint8, device=dev())
        _lib.check(lib.cips_composite_bwd_live(*head, P_(mask), None, *tail), "cips_composite_bwd_live")
        return dfeat, dsig, mask
    _lib.check(lib.cips_composite_bwd(*head, *tail), "cips_composite_bwd")
    return dfeat, dsig, None


# --------------------------------------------------------------------------------------
# 1. the list
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,S", SHAPES)
def test_forward_list_is_the_rule(H, W, S):
    """idx / count of cips_live_points_clamp == the numpy rule, ascending; image 0 has no live sample without last_back and one
    per ray with it, image 1 all of them; white_back adds none; softplus lists everything"""
    from cips3d_amd import _lib
    feat, sig, z, noise, dfea = _inputs(H, W, S)
    b, n = sig.shape[:2]
    P = n * S
    got = {c: _list(sig, noise, c[0], c[1]) for c in CASES}
    soft = _list(sig, noise, 0.3, 0, clamp="softplus")
    torch.cuda.synchronize()
    for (ns, fl), (idx, count) in got.items():
        want, _ = _rule(sig, noise, ns, fl)
        want = want.reshape(b, P)
        assert count.tolist() == want.sum(1).tolist(), (ns, fl)
        for i in range(b):
            assert np.array_equal(idx[i, :int(count[i])].cpu().numpy(), np.nonzero(want[i])[0].astype(np.int32)), (ns, fl, i)
        assert count.tolist()[:2] == [n if fl & 1 else 0, P]
        assert 0.3 * P < int(count[2]) < 0.9 * P
        assert torch.equal(count, got[(ns, fl & 1)][1])          # white_back adds no live sample
    assert soft[1].tolist() == [P] * b
    lib = _lib.load()
    assert lib.cips_composite_has_dead_samples(0) == 1 and lib.cips_composite_has_dead_samples(1) == 0


# --------------------------------------------------------------------------------------
# 2. a superset of the backward-time mask
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,S", SHAPES)
@pytest.mark.parametrize("noise_std,flags", CASES)
def test_forward_list_contains_the_backward_mask(H, W, S, noise_std, flags):
    """the mask cips_composite_bwd_live writes for a random dfea is inside the list at every sample; where the list has more,
    the dense call's row and dsigma are exactly zero there with the clamp open (w or dsigma underflowed): at most 1 % of the
    samples"""
    inp = _inputs(H, W, S)
    feat, sig, z, noise, dfea = inp
    b, n = sig.shape[:2]
    idx, count = _list(sig, noise, noise_std, flags)
    d_feat, d_sig, _ = _composite(inp, S, noise_std, flags, "dense")
    _, _, mask = _composite(inp, S, noise_std, flags, "live")
    torch.cuda.synchronize()
    listed = _listed_mask(idx, count, n * S).view(b, n, S)
    mask = mask.bool().cpu()
    assert not bool((mask & ~listed).any()), "a sample the backward calls live is missing from the forward-time list"
    extra = listed & ~mask
    _, x = _rule(sig, noise, noise_std, flags)
    zero = ((d_feat == 0).all(-1) & (d_sig == 0)).cpu()
    assert bool((zero & torch.from_numpy(x > 0))[extra].all()), "list and mask differ at a sample that is not an underflow"
    print(f"list vs mask {H}x{W} S={S} noise {noise_std} flags {flags}: {int(extra.sum())} of {extra.numel()} samples listed only")
    assert int(extra.sum()) <= 0.01 * extra.numel()


# --------------------------------------------------------------------------------------
# 3. the compositing backward on the listed samples
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,S", SHAPES)
@pytest.mark.parametrize("noise_std,flags", CASES)
def test_listed_compositing_writes_the_listed_samples_only(H, W, S, noise_std, flags):
    """listed rows and dsigma are cips_composite_bwd's bit for bit; the others still hold the pre-fill"""
    inp = _inputs(H, W, S)
    feat, sig, z, noise, dfea = inp
    b, n = sig.shape[:2]
    idx, count = _list(sig, noise, noise_std, flags)
    d_feat, d_sig, _ = _composite(inp, S, noise_std, flags, "dense")
    l_feat, l_sig, _ = _composite(inp, S, noise_std, flags, "listed")
    torch.cuda.synchronize()
    listed = _listed_mask(idx, count, n * S).view(b, n, S).to(dev())
    assert torch.isfinite(d_feat).all() and torch.isfinite(d_sig).all()
    assert torch.equal(l_feat[listed], d_feat[listed]) and torch.equal(l_sig[listed], d_sig[listed])
    assert bool((l_feat[~listed] == SENTINEL).all()) and bool((l_sig[~listed] == SENTINEL).all()), "an unlisted sample was written"
    assert not bool((d_feat[listed] == SENTINEL).any())


def test_listed_compositing_softplus_is_the_dense_call():
    """a clamp without dead samples: every sample is written"""
    H, W, S = SHAPES[1]
    inp = _inputs(H, W, S)
    d_feat, d_sig, _ = _composite(inp, S, 0.3, 1, "dense", clamp="softplus")
    l_feat, l_sig, _ = _composite(inp, S, 0.3, 1, "listed", clamp="softplus")
    torch.cuda.synchronize()
    assert torch.equal(l_feat, d_feat) and torch.equal(l_sig, d_sig)


# --------------------------------------------------------------------------------------
# 4. the finalisation over segments
# --------------------------------------------------------------------------------------
def test_finalize_segments_is_reduce_plus_finalize_bit_for_bit():
    """random partials, rows per image 1, 30, 5, 16, 17, 3 (one row; most of the rows; the edges of the kernel's batches of 16
    rows), idle NaN rows behind them that nobody may read"""
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    ns = [1, 30, 5, 16, 17, 3]
    b = len(ns)
    std, t, g = _siren_setup(b, 27)
    tt = {k: v.detach().contiguous() for k, v in t.items()}
    rows = sum(ns)
    sw_, gw = lib.cips_siren_bwd_x3_sred(), lib.cips_siren_bwd_x3_gpart()
    sred = torch.full((rows + 4, sw_), float("nan"))
    gpart = torch.full((rows + 4, gw), float("nan"))
    sred[:rows] = torch.randn(rows, sw_, generator=g)
    gpart[:rows] = torch.randn(rows, gw, generator=g)
    sred, gpart = sred.to(dev()), gpart.to(dev())
    first = np.concatenate([[0], np.cumsum(ns)[:-1]])
    img = torch.tensor(np.stack([first, ns], 1), dtype=torch.int32).to(dev()).contiguous()
    sw = ops._siren_struct(tt)

    def outs():
        o = tuple(torch.full_like(tt[n], float("nan")) for n in ops._SIREN_NAMES)
        sg = _lib.SirenGrads()
        for n, v in zip(ops._SIREN_NAMES, o):
            setattr(sg, "d" + n, v.data_ptr())
        return o, sg
    ref, sg = outs()
    sr = torch.empty(b, sw_, device=dev()); gp = torch.empty(b, gw, device=dev())
    _lib.check(lib.cips_siren_bwd_x3_reduce_segments(P_(sred), P_(gpart), P_(img), b, P_(sr), P_(gp), ops._stream()), "reduce")
    _lib.check(lib.cips_siren_bwd_x3_finalize(C.byref(sw), P_(sr), P_(gp), b, 1, C.byref(sg), ops._stream()), "finalize")
    got, sg2 = outs()
    _lib.check(lib.cips_siren_bwd_x3_finalize_segments(C.byref(sw), P_(sred), P_(gpart), P_(img), b, C.byref(sg2), ops._stream()),
               "finalize_segments")
    torch.cuda.synchronize()
    for n, a, r in zip(ops._SIREN_NAMES, got, ref):
        assert torch.isfinite(r).all(), n
        assert torch.equal(a, r), (n, float((a - r).abs().max()))
    assert lib.cips_siren_bwd_x3_finalize_segments(C.byref(sw), P_(sred), P_(gpart), None, b, C.byref(sg2), ops._stream()) == 1


# --------------------------------------------------------------------------------------
# 5. RayMarchFunction, switch on / off / dense
# --------------------------------------------------------------------------------------
def _march_setup(H, W, S, b, noise_std, flags, seed, lists_in_forward=True):
    """test_gpu_siren_bwd_live._march_setup on H x W rays, the caller of RayMarchFunction promising to join the list stream
    (the tenth entry of geom); `std` is a static latent buffer the step reads"""
    from cips3d_amd import ops
    d = dev()
    n = H * W
    net = seeded_generator(seed).to(d).siren
    g = torch.Generator().manual_seed(seed + n)
    std = torch.randn(b, 128, generator=g).to(d).requires_grad_(True)
    xg = torch.linspace(-1, 1, W, device=d); yg = torch.linspace(1, -1, H, device=d); zg = torch.linspace(0.88, 1.12, S, device=d)
    zc = float(-1.0 / math.tan((2 * math.pi * 12 / 360) / 2))
    c2w = torch.eye(4).repeat(b, 1, 1)
    c2w[:, :3, 3] = torch.tensor([0.0, 0.0, 1.0])
    c2w = c2w.to(d).contiguous()
    jit = torch.rand(b, n, S, generator=g).to(d); noise = torch.randn(b, n, S, generator=g).to(d)
    up = torch.randn(b, n, 32, generator=g).to(d)
    geom = (b, H, W, S, zc, float(noise_std), ops._CLAMP["relu"], flags, True, lists_in_forward)
    params = list(net.parameters()) + [std]

    def step():
        fea, _ = net.march({"nerf_w0": std, "nerf_w1": std, "nerf_rgb": std}, geom, xg, yg, zg, c2w, jit, noise)
        ops.live_forward_join()
        (fea * up).sum().backward()
    return net, params, step, std


def _run(params, step):
    for p in params:
        p.grad = None
    step()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in params]


class _Spy:
    """records what a list-making function of ops returns (eager runs only)"""

    def __init__(self, monkeypatch, name):
        from cips3d_amd import ops
        self.calls, real = [], getattr(ops, name)

        def spy(*a, **k):
            out = real(*a, **k)
            self.calls.append(out)
            return out
        monkeypatch.setattr(ops, name, spy)

    def lists(self):
        idx, count = self.calls[-1][:2]
        torch.cuda.synchronize()
        return [idx[i, :int(count[i])].cpu() for i in range(idx.shape[0])]


@pytest.mark.parametrize("H,W,S,noise_std,flags", [(8, 8, 24, 0.0, 0), (8, 8, 24, 0.3, 2), (5, 8, 5, 0.3, 1), (5, 8, 5, 0.0, 3)])
def test_march_backward_live_forward_switch(H, W, S, noise_std, flags, monkeypatch):
    """RayMarchFunction forward + backward, b = 3: the lists of the forward pass (switch on) against those of the backward (off)
    and against the dense calls.  On and dense agree to the bar of test_march_backward_even_switch; on and off are equal bit for
    bit whenever their lists coincide, which they must without last_back."""
    from cips3d_amd import ops
    assert ops.SIREN_BWD_LIVE and ops.SIREN_BWD_EVEN
    net, params, step, _ = _march_setup(H, W, S, 3, noise_std, flags, 14)
    fwd, bwd = _Spy(monkeypatch, "live_plan_forward"), _Spy(monkeypatch, "live_points")
    monkeypatch.setattr(ops, "SIREN_LIVE_FWD", True)
    monkeypatch.setattr(ops, "SIREN_FIN_SEGMENTS", False)
    on = _run(params, step)
    assert len(fwd.calls) == 1 and not bwd.calls and not ops._LIVE_PENDING
    l_on = fwd.lists()
    monkeypatch.setattr(ops, "SIREN_FIN_SEGMENTS", True)            # the one-launch finalisation: the same bits
    for a, r in zip(_run(params, step), on):
        assert torch.equal(a, r)
    fwd.calls.pop()
    monkeypatch.setattr(ops, "SIREN_LIVE_FWD", False)
    off = _run(params, step)
    assert len(fwd.calls) == 1 and len(bwd.calls) == 1
    l_off = bwd.lists()
    monkeypatch.setattr(ops, "SIREN_BWD_LIVE", False)
    dense = _run(params, step)
    assert len(fwd.calls) == 1 and len(bwd.calls) == 1
    same = all(torch.equal(a, r) for a, r in zip(l_on, l_off))
    share = sum(len(a) for a in l_on) / (3 * H * W * S)
    worst = 0.0
    for a, r in zip(on, dense):
        assert torch.isfinite(a).all()
        worst = max(worst, rel_err(a, r))
    print(f"march {H}x{W} S={S} noise {noise_std} flags {flags}: live share {share:.3f}, lists coincide {same}, "
          f"on vs dense worst rel err {worst:.3e}")
    assert worst < TOL
    assert 0.05 < share < 0.95
    if not flags & 1:
        assert same
    if same:
        for a, r in zip(on, off):
            assert torch.equal(a, r)
    else:
        assert max(rel_err(a, r) for a, r in zip(on, off)) < TOL


def test_march_direct_call_without_the_promise_keeps_the_backward_time_lists(monkeypatch):
    """a geom of nine entries (no caller to join the list stream): the lists are made in the backward as before"""
    from cips3d_amd import ops
    net, params, step, _ = _march_setup(5, 8, 5, 3, 0.0, 0, 14, lists_in_forward=False)
    fwd, bwd = _Spy(monkeypatch, "live_plan_forward"), _Spy(monkeypatch, "live_points")
    _run(params, step)
    assert not fwd.calls and len(bwd.calls) == 1


# --------------------------------------------------------------------------------------
# 6. capture
# --------------------------------------------------------------------------------------
def test_march_live_forward_follows_the_data_in_a_replayed_graph(monkeypatch):
    """the captured forward + backward (8 x 8 rays, S = 24, b = 3) replayed on new latents with the density bias at +1, -1 and
    +0: the forward-time lists and their plan are launches of the graph, so every replay's gradients equal an eager run's bit
    for bit, and the eager runs' counts show that the replays covered both regimes"""
    from cips3d_amd import ops, graph
    monkeypatch.setattr(ops, "SIREN_LIVE_FWD", True)
    net, params, step, std = _march_setup(8, 8, 24, 3, 0.0, 0, 12)
    captured = graph.capture(step, params=params)
    assert not ops._LIVE_PENDING
    held = [p.grad for p in params]
    assert all(h is not None for h in held)
    fwd = _Spy(monkeypatch, "live_plan_forward")
    g = torch.Generator().manual_seed(5)
    shares = []
    for delta in (1.0, -2.0, 1.0):
        with torch.no_grad():
            net.final_layer.bias.add_(delta)
            std.copy_(torch.randn(std.shape, generator=g))
        captured.replay()
        torch.cuda.synchronize()
        got = [h.clone() for h in held]
        ref = _run(params, step)
        for a, r in zip(got, ref):
            assert torch.isfinite(a).all()
            assert torch.equal(a, r)
        shares.append(sum(len(x) for x in fwd.lists()) / (3 * 64 * 24))
    print("live shares at bias +1, -1, +0:", [round(s, 3) for s in shares])
    assert shares[0] > 0.9 and shares[1] < 0.1 and shares[1] < shares[2] < shares[0]


def _generator_fixture():
    fix = load_golden("g_r8_flat_noise")
    d = torch.device("cuda:0")
    G = seeded_generator(fix["seed"], freeze=fix["freeze"], device=d)
    zs = {k: v.to(d).clone() for k, v in fix["zs"].items()}
    rand = {k: v.to(d) for k, v in fix["rand"].items()}
    kw = dict(img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"], grad_points=None,
              forward_points=None, rand_override=rand, **fix["G_kwargs"])
    return fix, G, zs, kw


def test_generator_step_with_forward_lists_replays_on_new_latents(monkeypatch):
    """the whole generator (the lists' stream beside the INR head, joined behind it): forward + backward captured, replayed
    on new latents, against the eager step at the bar of test_captured_generator_step_replays_the_eager_gradients; and the
    eager gradients with the switch on against off"""
    from cips3d_amd import ops
    from cips3d_amd.graph import capture
    monkeypatch.setattr(ops, "SIREN_LIVE_FWD", True)
    fix, G, zs, kw = _generator_fixture()
    G0 = fix["G0"].to(zs["z_nerf"].device)
    params = [p for p in G.parameters() if p.requires_grad]

    def step():
        for p in params:
            p.grad = None
        imgs, _ = G(zs, **kw)
        (imgs * G0).sum().backward()

    cs = capture(step, warmup=1, params=params)
    assert not ops._LIVE_PENDING
    held = [p.grad for p in params]                  # the graph's own gradient tensors: every replay overwrites them
    fwd = _Spy(monkeypatch, "live_plan_forward")
    g = torch.Generator().manual_seed(9)
    counts = []
    for _ in range(2):
        for v in zs.values():
            v.copy_(torch.randn(v.shape, generator=g))
        cs()
        torch.cuda.synchronize()
        got = [None if h is None else h.clone() for h in held]
        step()
        torch.cuda.synchronize()
        assert len(fwd.calls) == len(counts) + 1, "the generator's march did not make its lists in the forward pass"
        counts.append(fwd.calls[-1][1].tolist())
        for p, a in zip(params, got):
            assert (p.grad is None) == (a is None)
            if a is not None:
                assert torch.allclose(a, p.grad, rtol=1e-6, atol=1e-9), float((a - p.grad).abs().max())
    print("live counts of the two latents:", counts)
    assert counts[0] != counts[1]
    on = [None if p.grad is None else p.grad.detach().clone() for p in params]
    monkeypatch.setattr(ops, "SIREN_LIVE_FWD", False)
    step()
    torch.cuda.synchronize()
    assert len(fwd.calls) == 2
    for p, a in zip(params, on):
        if a is not None:
            assert torch.allclose(a, p.grad, rtol=1e-6, atol=1e-9), float((a - p.grad).abs().max())


def test_captured_training_forward_without_a_backward_leaves_no_stream_unjoined(monkeypatch):
    """a training forward of the generator (grad mode on: the lists are made) with no backward, captured and replayed: the
    capture ends without an unjoined stream, and nothing is left pending"""
    from cips3d_amd import ops
    from cips3d_amd.graph import capture
    monkeypatch.setattr(ops, "SIREN_LIVE_FWD", True)
    fix, G, zs, kw = _generator_fixture()
    buf = torch.zeros_like(fix["imgs"], device=zs["z_nerf"].device)
    fwd = _Spy(monkeypatch, "live_plan_forward")

    def forward_only():
        imgs, _ = G(zs, **kw)
        assert imgs.requires_grad
        buf.copy_(imgs.detach())

    forward_only()
    torch.cuda.synchronize()
    eager = buf.clone()
    assert len(fwd.calls) == 1 and not ops._LIVE_PENDING
    cs = capture(forward_only, warmup=1)
    assert not ops._LIVE_PENDING
    buf.zero_()
    cs()
    torch.cuda.synchronize()
    assert torch.equal(buf, eager)
