"""GPU: the fused SIREN backward over the LIVE samples only (cips_composite_bwd_live -> cips_live_points ->
cips_siren_bwd_x3_live / cips_siren_bwd_x3_rays_live; ops.SIREN_BWD_LIVE).  A sample whose compositing weight and dsigma are
exactly zero adds +-0 to every SIREN gradient, so leaving it out changes nothing but the summation order: the mask and the
list are checked exactly, the list walk bit for bit where its partition is the dense one and to the tolerance of
test_siren_backward elsewhere, and a replayed graph must follow the data."""
import ctypes as C
import math

import pytest
import torch

from conftest import seeded_generator, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3          # TOL of tests/test_gpu_kernels.py (test_siren_backward)


def dev():
    return torch.device("cuda")


def P_(x):
    return C.c_void_p(x.data_ptr()) if x is not None else None


# --------------------------------------------------------------------------------------
# 1. the mask
# --------------------------------------------------------------------------------------
def _composite_inputs(R, S, seed):
    g = torch.Generator().manual_seed(seed)
    feat = torch.randn(R, S, 32, generator=g)
    sig = torch.randn(R, S, generator=g) + 0.43          # P(sigma < 0) = 0.33
    z = torch.linspace(0.88, 1.12, S).view(1, S) + (torch.rand(R, S, generator=g) - 0.5) * (0.1 / S)
    noise = torch.randn(R, S, generator=g)
    dfea = torch.randn(R, 32, generator=g)
    return [t.to(dev()).contiguous() for t in (feat, sig, z, noise, dfea)]


def _pinned_mask(sig, noise, noise_std):
    """what a pinned clamp mask is in use: the branches another evaluation of the same pre-activations took — the sign of
    sigma + noise, the other way round where that is within rounding of zero (here |x| < 0.05: ~4 % of the samples).  The
    last sample keeps its own branch when clamped: its interval is 1e10 long, and the linear extension of a negative
    density over it overflows in the reference arithmetic as well."""
    x = sig + noise * noise_std
    pin = x > 0
    near = x.abs() < 0.05
    near[:, -1] &= pin[:, -1]
    return (pin ^ near).to(torch.uint8).contiguous()


def _composite_bwd(inp, S, noise_std, clamp, flags, pinned, live):
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    feat, sig, z, noise, dfea = inp
    R = feat.shape[0]
    pin = _pinned_mask(sig, noise, noise_std) if pinned else None
    dfeat = torch.full((R, S, 32), float("nan"), device=dev())
    dsig = torch.full((R, S), float("nan"), device=dev())
    head = (P_(feat), P_(sig), P_(z), None, None, None, P_(noise) if noise_std else None, float(noise_std), None, P_(dfea),
            P_(dfeat), P_(dsig), None, None)
    tail = (R, S, ops._CLAMP[clamp], flags, P_(pin), ops._stream())
    if live:
        mask = torch.full((R, S), 7, dtype=torch.uint8, device=dev())
        _lib.check(lib.cips_composite_bwd_live(*head, P_(mask), None, *tail), "cips_composite_bwd_live")
        return dfeat, dsig, mask
    _lib.check(lib.cips_composite_bwd(*head, *tail), "cips_composite_bwd")
    return dfeat, dsig, None


_MASK_CASES = [("relu", f, ns, False) for f in (0, 1, 2, 3) for ns in (0.0, 0.3)] + [("softplus", 0, 0.3, False),
                                                                                     ("softplus", 3, 0.0, False),
                                                                                     ("relu", 0, 0.0, True), ("relu", 3, 0.3, True)]


@pytest.mark.parametrize("R,S", [(2 * 100, 5), (2 * 64, 24)])
@pytest.mark.parametrize("clamp,flags,noise_std,pinned", _MASK_CASES)
def test_live_mask_is_exact(R, S, clamp, flags, noise_std, pinned):
    """mask == (dfeat row != 0).any() | (dsigma != 0) of the dense call on the same inputs; the live call's dsigma equals the
    dense one everywhere and its dfeat on the live rows (the dead rows are not written); softplus is all live; under
    last_back the topped-up last sample is live."""
    inp = _composite_inputs(R, S, 5 + S)
    d_feat, d_sig, _ = _composite_bwd(inp, S, noise_std, clamp, flags, pinned, live=False)
    l_feat, l_sig, mask = _composite_bwd(inp, S, noise_std, clamp, flags, pinned, live=True)
    torch.cuda.synchronize()
    want = (d_feat != 0).any(-1) | (d_sig != 0)
    assert int(mask.max()) <= 1
    assert torch.isfinite(d_feat).all() and torch.isfinite(d_sig).all()
    assert torch.equal(mask.bool(), want)
    assert torch.equal(l_sig, d_sig)
    assert torch.equal(l_feat[want], d_feat[want])
    assert torch.isnan(l_feat[~want]).all(), "a dead row was written"
    share = want.float().mean().item()
    print(f"mask R={R} S={S} {clamp} flags {flags} noise {noise_std} pinned {pinned}: live share {share:.3f}")
    if clamp == "softplus":
        assert bool(want.all())
    else:
        assert 0.3 < share < 0.9
    if flags & 1:
        assert bool(want[:, -1].all())


def test_live_mask_with_a_fine_set():
    """the merged (hierarchical) form of the compositing backward: live_f / live_c in the order of dfeat_f / dfeat_c, through
    the merge order; and a mask for only one of the two sample sets is refused"""
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    R, S = 2 * 50, 6
    E = 2 * S
    d = dev()
    g = torch.Generator().manual_seed(31)
    fc, ff = (torch.randn(R, S, 32, generator=g).to(d) for _ in range(2))
    sc, sf = ((torch.randn(R, S, generator=g) + 0.43).to(d) for _ in range(2))
    zc = (torch.linspace(0.88, 1.12, S).view(1, S) + (torch.rand(R, S, generator=g) - 0.5) * 0.02).to(d).contiguous()
    zf = (0.88 + 0.24 * torch.rand(R, S, generator=g)).to(d)
    noise = torch.randn(R, E, generator=g).to(d)
    dfea = torch.randn(R, 32, generator=g).to(d)
    fea = torch.empty(R, 32, device=d); order = torch.empty(R, E, dtype=torch.int32, device=d)
    s = ops._stream()
    _lib.check(lib.cips_composite_fwd(P_(fc), P_(sc), P_(zc), P_(ff), P_(sf), P_(zf), P_(noise), 0.3, P_(fea), None, None, P_(order),
                                      None, R, S, ops._CLAMP["relu"], 1, None, None, s), "cips_composite_fwd")

    def bwd(live):
        o = [torch.full((R, S, 32), float("nan"), device=d), torch.full((R, S), float("nan"), device=d),
             torch.full((R, S, 32), float("nan"), device=d), torch.full((R, S), float("nan"), device=d)]
        m = [torch.full((R, S), 7, dtype=torch.uint8, device=d) for _ in range(2)] if live else [None, None]
        head = (P_(fc), P_(sc), P_(zc), P_(ff), P_(sf), P_(zf), P_(noise), 0.3, P_(order), P_(dfea), *[P_(x) for x in o])
        tail = (R, S, ops._CLAMP["relu"], 1, None, s)
        if live:
            assert lib.cips_composite_bwd_live(*head, P_(m[0]), None, *tail) == 1        # hipErrorInvalidValue
            assert lib.cips_composite_bwd_live(*head, None, P_(m[1]), *tail) == 1
            _lib.check(lib.cips_composite_bwd_live(*head, P_(m[0]), P_(m[1]), *tail), "cips_composite_bwd_live")
        else:
            _lib.check(lib.cips_composite_bwd(*head, *tail), "cips_composite_bwd")
        return o, m
    dense, _ = bwd(False)
    got, (m_c, m_f) = bwd(True)
    torch.cuda.synchronize()
    for df_d, ds_d, df_l, ds_l, m in ((dense[0], dense[1], got[0], got[1], m_c), (dense[2], dense[3], got[2], got[3], m_f)):
        assert torch.isfinite(df_d).all() and torch.isfinite(ds_d).all()
        want = (df_d != 0).any(-1) | (ds_d != 0)
        assert int(m.max()) <= 1 and torch.equal(m.bool(), want)
        assert torch.equal(ds_l, ds_d) and torch.equal(df_l[want], df_d[want])
        assert torch.isnan(df_l[~want]).all()
        assert 0.3 < want.float().mean().item() < 0.9


# --------------------------------------------------------------------------------------
# 2. the list
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [128 * 7 + 5, 2 * 16384 + 160])
def test_live_list_is_exact(P):
    """idx[b, :count[b]] == nonzero(mask[b]) ascending, for an all-dead, an all-live and two random images; P not a multiple
    of 128 (byte path) and P a multiple of 16 spanning three 16 384-byte tiles (vector path)."""
    from cips3d_amd import ops
    g = torch.Generator().manual_seed(P)
    mask = torch.zeros(4, P, dtype=torch.uint8)
    mask[1] = 1
    mask[2] = (torch.rand(P, generator=g) < 0.65).to(torch.uint8) * 255
    mask[3] = (torch.rand(P, generator=g) < 0.01).to(torch.uint8)
    md = mask.to(dev())
    idx, count = ops.live_points(md)
    idx2, count2 = ops.live_points(md)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and count.dtype == torch.int32
    assert count.tolist() == [int((mask[b] != 0).sum()) for b in range(4)]
    assert count.tolist()[:2] == [0, P]
    for b in range(4):
        nz = torch.nonzero(mask[b]).flatten().to(torch.int32)
        assert torch.equal(idx[b, :count[b]].cpu(), nz), b
        assert torch.equal(idx2[b, :count[b]], idx[b, :count[b]])
    assert torch.equal(count2, count)


# --------------------------------------------------------------------------------------
# 3 / 4. the list walk
# --------------------------------------------------------------------------------------
def _siren_setup(b, seed):
    G = seeded_generator(seed).to(dev())
    net = G.siren
    g = torch.Generator().manual_seed(seed)
    std = torch.randn(b, 128, generator=g).to(dev()).requires_grad_(True)
    t = {}
    t["g0"], t["p0"] = net.network[0].film(std); t["g1"], t["p1"] = net.network[1].film(std); t["gc"], t["pc"] = net.color_layer_sine.film(std)
    t.update(w0=net.network[0].linear.weight, b0=net.network[0].linear.bias, w1=net.network[1].linear.weight, b1=net.network[1].linear.bias,
             ws=net.final_layer.weight, bs=net.final_layer.bias, wc=net.color_layer_sine.linear.weight, bc=net.color_layer_sine.linear.bias,
             wf=net.color_layer_linear[0].weight, bf=net.color_layer_linear[0].bias)
    return std, t, g


def _points_or_rays(form, b, H, W, S, g):
    """-> (points (b,P,3), None) or (None, (RayParams, the tensors it points into: the caller keeps them alive))"""
    from cips3d_amd import ops
    d = dev()
    P = H * W * S
    if form == "points":
        pts = ((torch.rand(b, P, 3, generator=g) - 0.5) * 0.3).to(d)
        return pts, None
    xg = torch.linspace(-1, 1, W, device=d); yg = torch.linspace(1, -1, max(H, 2), device=d)[:H].contiguous()
    zg = torch.linspace(0.88, 1.12, S, device=d)
    zc = float(-1.0 / math.tan((2 * math.pi * 12 / 360) / 2))
    c2w = torch.eye(4).repeat(b, 1, 1)
    c2w[:, :3, 3] = torch.tensor([0.0, 0.0, 1.0])
    c2w = c2w.to(d).contiguous()
    jit = torch.rand(b, H * W, S, generator=g).to(d)
    keep = (xg, yg, zg, c2w, jit)
    return None, (ops._ray_params(xg, yg, zg, zc, c2w, jit, H, W, S), keep)


def _partials(tt, dfeat, dsigma, b, P, pts, rays, live):
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    sw = ops._siren_struct(tt)
    chunks = lib.cips_siren_bwd_x3_chunks(b, P)
    sred = torch.full((b * chunks, lib.cips_siren_bwd_x3_sred()), float("nan"), device=dev())
    gpart = torch.full((b * chunks, lib.cips_siren_bwd_x3_gpart()), float("nan"), device=dev())
    s = ops._stream()
    if live is None:
        if pts is not None:
            rc = lib.cips_siren_bwd_x3(C.byref(sw), P_(pts), P_(dfeat), P_(dsigma), P_(sred), P_(gpart), b, P, s)
        else:
            rc = lib.cips_siren_bwd_x3_rays(C.byref(sw), C.byref(rays), P_(dfeat), P_(dsigma), P_(sred), P_(gpart), b, s)
    else:
        idx, count = live
        if pts is not None:
            rc = lib.cips_siren_bwd_x3_live(C.byref(sw), P_(pts), P_(dfeat), P_(dsigma), P_(idx), P_(count), P_(sred), P_(gpart), b, P, s)
        else:
            rc = lib.cips_siren_bwd_x3_rays_live(C.byref(sw), C.byref(rays), P_(dfeat), P_(dsigma), P_(idx), P_(count), P_(sred),
                                                 P_(gpart), b, s)
    _lib.check(rc, "siren backward")
    return sred, gpart, chunks


@pytest.mark.parametrize("trig", [0, 1])
@pytest.mark.parametrize("form", ["points", "rays"])
def test_live_walk_of_every_point_is_bit_identical(trig, form, monkeypatch):
    """b = 2, P = 1024: the dense chunk is 512 (two workgroups per image), and the list of all points splits into
    roundup128(1024 / 2) = 512 slots per workgroup: the same points in the same rounds, so the partials are bit-identical"""
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    b, H, W, S = 2, 8, 8, 16
    P = H * W * S
    std, t, g = _siren_setup(b, 21)
    tt = {k: v.detach().contiguous() for k, v in t.items()}
    pts, rp = _points_or_rays(form, b, H, W, S, g)
    rays = rp[0] if rp else None
    dfeat = torch.randn(b, P, 32, generator=g).to(dev()); dsigma = torch.randn(b, P, generator=g).to(dev())
    idx = torch.arange(P, dtype=torch.int32, device=dev()).repeat(b, 1).contiguous()
    count = torch.full((b,), P, dtype=torch.int32, device=dev())
    sr_d, gp_d, chunks = _partials(tt, dfeat, dsigma, b, P, pts, rays, None)
    sr_l, gp_l, _ = _partials(tt, dfeat, dsigma, b, P, pts, rays, (idx, count))
    torch.cuda.synchronize()
    assert chunks == 2
    assert torch.isfinite(sr_d).all() and torch.isfinite(gp_d).all()
    assert torch.equal(sr_l, sr_d) and torch.equal(gp_l, gp_d)


def _grads(t, std, dfeat, dsigma, b, P, pts, rays, live):
    from cips3d_amd import ops
    tt = {k: v.detach().contiguous() for k, v in t.items()}
    gr = ops._siren_backward(tt, dfeat, dsigma, b, P, points=pts, rays=rays, live=live)
    film = ops._SIREN_NAMES[:6]
    gs, = torch.autograd.grad([t[n] for n in film], std, grad_outputs=list(gr[:6]), retain_graph=True)
    return dict(zip(ops._SIREN_NAMES, gr)), gs


@pytest.mark.parametrize("trig", [0, 1])
@pytest.mark.parametrize("form", ["points", "rays"])
@pytest.mark.parametrize("case", ["sparse", "empty_image"])
def test_live_walk_equals_dense(case, form, trig, monkeypatch):
    """b = 3, P = 128 * 7 + 5 (= 1 x 53 rays of 17 samples): two workgroups per image.  "sparse": image 0 all live, image 1
    ~35 % dead, image 2 five live rows (its second workgroup is empty).  "empty_image": image 1 has no live point at all
    and its FiLM gradients are exactly zero.  The dense call sees zeros in the dead rows, the live call NaNs: it must not
    read them."""
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    b, H, W, S = 3, 1, 53, 17
    P = H * W * S
    assert P == 128 * 7 + 5
    std, t, g = _siren_setup(b, 22)
    pts, rp = _points_or_rays(form, b, H, W, S, g)
    rays = rp[0] if rp else None
    live = torch.ones(b, P, dtype=torch.bool)
    if case == "sparse":
        live[1] = torch.rand(P, generator=g) >= 0.35
        live[2] = False
        live[2, torch.tensor([0, 130, 131, 640, P - 1])] = True
    else:
        live[0] = torch.rand(P, generator=g) >= 0.5
        live[1] = False
    live = live.to(dev())
    dfeat = torch.randn(b, P, 32, generator=g).to(dev()); dsigma = torch.randn(b, P, generator=g).to(dev())
    nan = torch.tensor(float("nan"), device=dev())
    df_dense, ds_dense = dfeat * live.unsqueeze(-1), dsigma * live
    df_live, ds_live = torch.where(live.unsqueeze(-1), dfeat, nan), torch.where(live, dsigma, nan)
    lp = ops.live_points(live.to(torch.uint8).contiguous())
    ref, ref_s = _grads(t, std, df_dense.contiguous(), ds_dense.contiguous(), b, P, pts, rays, None)
    got, got_s = _grads(t, std, df_live.contiguous(), ds_live.contiguous(), b, P, pts, rays, lp)
    torch.cuda.synchronize()
    worst = 0.0
    for n in ops._SIREN_NAMES:
        assert torch.isfinite(got[n]).all(), n
        e = rel_err(got[n], ref[n])
        worst = max(worst, e)
        assert e < TOL, (n, e)
    assert torch.isfinite(got_s).all()
    e = rel_err(got_s, ref_s)
    print(f"live walk {case} {form} trig={trig}: worst gradient rel err {max(worst, e):.3e}")
    assert e < TOL
    if case == "empty_image":
        for n in ops._SIREN_NAMES[:6]:
            assert bool((got[n][1] == 0).all()), n
        assert bool((got_s[1] == 0).all())


# --------------------------------------------------------------------------------------
# 5 / 6. RayMarchFunction
# --------------------------------------------------------------------------------------
def _march_setup(img, S, b, noise_std, flags, seed):
    from cips3d_amd import ops
    d = dev()
    n = img * img
    G = seeded_generator(seed).to(d)
    net = G.siren
    g = torch.Generator().manual_seed(seed + img)
    std = torch.randn(b, 128, generator=g).to(d).requires_grad_(True)
    xg = torch.linspace(-1, 1, img, device=d); yg = torch.linspace(1, -1, img, device=d); zg = torch.linspace(0.88, 1.12, S, device=d)
    zc = float(-1.0 / math.tan((2 * math.pi * 12 / 360) / 2))
    c2w = torch.eye(4).repeat(b, 1, 1)
    c2w[:, :3, 3] = torch.tensor([0.0, 0.0, 1.0])
    c2w = c2w.to(d).contiguous()
    jit = torch.rand(b, n, S, generator=g).to(d); noise = torch.randn(b, n, S, generator=g).to(d)
    up = torch.randn(b, n, 32, generator=g).to(d)
    geom = (b, img, img, S, zc, float(noise_std), ops._CLAMP["relu"], flags, True)
    params = list(net.parameters()) + [std]

    def step():
        fea, _ = net.march({"nerf_w0": std, "nerf_w1": std, "nerf_rgb": std}, geom, xg, yg, zg, c2w, jit, noise)
        (fea * up).sum().backward()
    return net, params, step


def _run(params, step):
    for p in params:
        p.grad = None
    step()
    torch.cuda.synchronize()
    return [p.grad.clone() for p in params]


@pytest.mark.parametrize("img,S,b,noise_std,flags", [(8, 24, 2, 0.0, 0), (10, 5, 3, 0.2, 3)])
def test_march_backward_live_switch(img, S, b, noise_std, flags, monkeypatch):
    """RayMarchFunction forward + backward with ops.SIREN_BWD_LIVE on vs off: every SIREN parameter gradient and the style
    gradient agree to the tolerance of test_siren_backward"""
    from cips3d_amd import ops
    net, params, step = _march_setup(img, S, b, noise_std, flags, 11)
    monkeypatch.setattr(ops, "SIREN_BWD_LIVE", False)
    off = _run(params, step)
    monkeypatch.setattr(ops, "SIREN_BWD_LIVE", True)
    on = _run(params, step)
    worst = 0.0
    for a, r in zip(on, off):
        assert torch.isfinite(a).all()
        worst = max(worst, rel_err(a, r))
    print(f"march backward live on vs off {img}x{img} S={S} b={b}: worst gradient rel err {worst:.3e}")
    assert worst < TOL


def test_march_backward_live_follows_the_data_in_a_replayed_graph(monkeypatch):
    """The captured forward + backward (r8, S = 24, b = 2) replayed after the density bias moved by +1 (nearly every sample
    live) and then to -1 (nearly none): each replay's gradients equal an eager run on the same weights bit for bit — the
    trip counts come from device memory, nothing is baked in at capture time, and nothing on the path synchronises with
    the host (the capture itself would fail).  The eager runs' counts show that the replays covered both regimes: the
    initial sigma has mean ~0.13 and standard deviation <= 0.35, so a shift by +-1 is three deviations or more."""
    from cips3d_amd import ops, graph
    monkeypatch.setattr(ops, "SIREN_BWD_LIVE", True)
    net, params, step = _march_setup(8, 24, 2, 0.0, 0, 12)
    captured = graph.capture(step, params=params)
    held = [p.grad for p in params]                  # the graph's own gradient tensors: every replay overwrites them
    assert all(h is not None for h in held)
    counts, real = [], ops.live_points

    def spy(mask):                                   # eager runs only: installed after the capture
        idx, count = real(mask)
        counts.append((count, mask.numel()))
        return idx, count
    monkeypatch.setattr(ops, "live_points", spy)
    shares = []
    for delta in (1.0, -2.0, 1.0):                   # bias + 1, bias - 1, the initial bias
        with torch.no_grad():
            net.final_layer.bias.add_(delta)
        captured.replay()
        torch.cuda.synchronize()
        got = [h.clone() for h in held]
        ref = _run(params, step)
        for a, r in zip(got, ref):
            assert torch.isfinite(a).all()
            assert torch.equal(a, r)
        count, total = counts[-1]
        shares.append(count.sum().item() / total)
    print("live shares at bias +1, -1, +0:", [round(s, 3) for s in shares])
    assert shares[0] > 0.9 and shares[1] < 0.1 and shares[1] < shares[2] < shares[0]
