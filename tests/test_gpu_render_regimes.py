"""GPU: the renderer kernels (render.hip, the compositing block of the fused march, the live-sample lists) on the ray classes
of tests/render_regimes.py — opaque surfaces with alpha == 1.0f in the middle of a ray, walls behind which (float)T == 0,
empty rays, exact +-0 at the relu gate, softplus at 25 and -110 — against oracle.integrate / oracle.fine_points in fp64.
tests/test_render_regimes_cpu.py shows on the CPU that the classes reach those regimes and that no unpinned gate lies within
1e-4 of 0, which is why nothing here pins a clamp branch.

Paths no test ran before: the compositing launchers with fewer than 32 rays per workgroup (hierarchical S = 48: E = 96, 16
rays per workgroup in the backward), the resampler's u == 0 and u > cdf[-1] edges, and its in-kernel ray form (rays=)."""
import ctypes as C
import functools
import math

import pytest
import torch

import render_regimes as rr
from conftest import max_rel, rel_err, seeded_generator
from test_gpu_siren_live_fwd import SENTINEL, _composite, _list, _listed_mask

pytestmark = pytest.mark.gpu

TOL = 1e-3          # TOL of tests/test_gpu_kernels.py
F32, F64 = torch.float32, torch.float64
R = rr.B * rr.N     # 134 rays: no multiple of 32, 16 or 8 rays per workgroup


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _set(S, soft, fine):
    """one draw of the classes (coarse or fine seed) with its features -> r, feat (b, n, S, 32)"""
    seed = {(False, False): rr.SEED_COARSE, (False, True): rr.SEED_FINE, (True, False): rr.SEED_SOFT, (True, True): rr.SEED_SOFT_FINE}
    r = (rr.build_softplus if soft else rr.build)(rr.B, rr.N, S, seed[(soft, fine)])
    feat, up = rr.features(rr.B, rr.N, S, 7 + S + (1000 if fine else 0))
    return r, feat, up


@functools.lru_cache(maxsize=None)
def _flat_ref(S, clamp, flags):
    r, feat, up = _set(S, clamp == "softplus", False)
    noise, noise_std = _noise(S, clamp)
    return rr.oracle_composite(feat, r["x"], r["z"], up, clamp, flags, F64, noise, noise_std)


def _noise(E, clamp):
    """softplus runs with a noise draw (x stays above 20 / below the underflow); relu has none: its gates are crafted"""
    if clamp != "softplus":
        return None, 0.0
    return torch.randn(rr.B, rr.N, E, generator=torch.Generator().manual_seed(90 + E)), 0.3


def _check_composite(got, ref, what):
    """got / ref: dicts of fea, depth, w and the input gradients; the bars of test_composite_forward_backward"""
    e = {k: (max_rel if k in ("fea", "depth", "w") else rel_err)(got[k], ref[k].reshape(got[k].shape)) for k in got}
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert torch.isfinite(got[k]).all(), k
        assert v < (1e-5 if k in ("fea", "depth", "w") else 1e-4), (k, v)


CLAMP_FLAGS = [("relu", 0), ("relu", 1), ("relu", 2), ("relu", 3), ("softplus", 0), ("softplus", 3)]


# --------------------------------------------------------------------------------------
# 2. compositing, forward and backward
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", rr.FLAT_S)
@pytest.mark.parametrize("clamp,flags", CLAMP_FLAGS)
def test_composite_flat(S, clamp, flags):
    """CompositeFunction without a fine set.  relu with flags 1 and 2 hands the class values in as noise (noise_std = 1) on a
    sigma of zeros, the other cases as sigma: the same pre-activation bits either way."""
    from cips3d_amd import ops
    d = dev()
    r, feat, up = _set(S, clamp == "softplus", False)
    ref = _flat_ref(S, clamp, flags)
    x = r["x"].view(R, S).to(d)
    noise, noise_std = _noise(S, clamp)
    as_noise = clamp == "relu" and flags in (1, 2)
    if as_noise:
        sc, nz, noise_std = torch.zeros_like(x).requires_grad_(True), x, 1.0
    else:
        sc, nz = x.clone().requires_grad_(True), (noise.view(R, S).to(d) if noise is not None else None)
    fc = feat.view(R, S, 32).to(d).requires_grad_(True)
    fea, dep, wts, order, zs = ops.CompositeFunction.apply(fc, sc, r["z"].view(R, S).to(d), None, None, None, nz, noise_std,
                                                           ops._CLAMP[clamp], flags)
    (fea * up.view(R, 32).to(d)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(zs.cpu(), r["z"].view(R, S))
    _check_composite(dict(fea=fea, depth=dep, w=wts, dfeat=fc.grad, dx=sc.grad), ref, f"flat S={S} {clamp} flags {flags}")


def _hier(S, clamp, flags, zf=None, what="hier"):
    """CompositeFunction with a fine set (a second draw of the classes; zf replaces its depths) against the fp64 oracle on the
    inputs gathered by the product's own merge order"""
    from cips3d_amd import ops
    d = dev()
    soft = clamp == "softplus"
    E = 2 * S
    (rc, featc, up), (rf, featf, _) = _set(S, soft, False), _set(S, soft, True)
    zf = rf["z"] if zf is None else zf
    noise, noise_std = _noise(E, clamp)
    fc, ff = (t.view(R, S, 32).to(d).requires_grad_(True) for t in (featc, featf))
    sc, sf = (t["x"].view(R, S).to(d).requires_grad_(True) for t in (rc, rf))
    fea, dep, wts, order, zs = ops.CompositeFunction.apply(fc, sc, rc["z"].view(R, S).to(d), ff, sf, zf.reshape(R, S).to(d),
                                                           noise.view(R, E).to(d) if noise is not None else None, noise_std,
                                                           ops._CLAMP[clamp], flags)
    (fea * up.view(R, 32).to(d)).sum().backward()
    torch.cuda.synchronize()
    # the merge: a permutation per ray, ascending depths, and the depths it reports are the inputs' bits
    order = order.cpu().long()
    all_z = torch.cat([zf.reshape(R, S), rc["z"].view(R, S)], -1)
    all_x = torch.cat([rf["x"].view(R, S), rc["x"].view(R, S)], -1)
    all_f = torch.cat([featf.view(R, S, 32), featc.view(R, S, 32)], -2)
    assert torch.equal(order.sort(-1).values, torch.arange(E).expand(R, E))
    assert torch.equal(zs.cpu(), all_z.gather(-1, order))
    assert bool((zs[:, 1:] >= zs[:, :-1]).all())
    zsort, idx = torch.sort(all_z, -1)
    ties = int((zsort[:, 1:] == zsort[:, :-1]).sum())
    if ties == 0:
        assert torch.equal(order, idx), "merge order must be bit-exact on depths without ties"
    g = lambda t: t.gather(-1, order).view(rr.B, rr.N, E)
    ref = rr.oracle_composite(all_f.gather(-2, order.unsqueeze(-1).expand(R, E, 32)).view(rr.B, rr.N, E, 32), g(all_x), g(all_z), up,
                              clamp, flags, F64, noise, noise_std)
    # the oracle's gradients back from compositing order to [fine, coarse]
    dfeat = torch.zeros(R, E, 32, dtype=F64).scatter_(-2, order.unsqueeze(-1).expand(R, E, 32), ref["dfeat"].view(R, E, 32))
    dx = torch.zeros(R, E, dtype=F64).scatter_(-1, order, ref["dx"].view(R, E))
    ref = dict(fea=ref["fea"], depth=ref["depth"], w=ref["w"], dfeat_f=dfeat[:, :S], dfeat_c=dfeat[:, S:], dx_f=dx[:, :S], dx_c=dx[:, S:])
    got = dict(fea=fea, depth=dep, w=wts, dfeat_f=ff.grad, dfeat_c=fc.grad, dx_f=sf.grad, dx_c=sc.grad)
    _check_composite(got, ref, f"{what} S={S} {clamp} flags {flags} ({ties} ties)")
    return ties


@pytest.mark.parametrize("S", rr.HIER_S)
@pytest.mark.parametrize("clamp,flags", CLAMP_FLAGS)
def test_composite_hierarchical(S, clamp, flags):
    """E = 2 S = 18, 48, 96: 32 rays per workgroup, then 32 forward / 16 backward at E = 96 (more than 80 entries)"""
    _hier(S, clamp, flags)


def test_composite_hierarchical_with_tied_depths():
    """every third ray's fine depths are its coarse depths bit for bit, and the rays after them repeat one fine depth:
    torch.sort promises no order for ties, so the oracle is evaluated in the product's"""
    S = 24
    zc, zf = _set(S, False, False)[0]["z"], _set(S, False, True)[0]["z"].clone()
    zf[:, 0::3] = zc[:, 0::3]
    zf[:, 1::3, 5] = zf[:, 1::3, 4]
    ties = _hier(S, "relu", 1, zf=zf, what="hier ties")
    assert ties >= (rr.N // 3) * S


@pytest.mark.parametrize("S", rr.FLAT_S)
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_liveness_loses_nothing(S, flags):
    """flat relu: dense, masked (cips_composite_bwd_live) and listed (cips_composite_bwd_listed) backward on outputs pre-filled
    with a sentinel.  What the masked and the listed call write is the dense call's bit for bit; the mask lies inside the list
    of cips_live_points_clamp; outside the list the dense row and dsigma compare equal to 0.  New here: wall samples (x > 0,
    w == 0: listed, and masked out) and the +-0 gates (not listed)."""
    d = dev()
    r, feat, up = _set(S, False, False)
    x = r["x"].to(d)
    inp = [feat.to(d).contiguous(), x.contiguous(), r["z"].to(d).contiguous(), None, up.to(d).contiguous()]
    idx, count = _list(x, None, 0.0, flags)
    d_feat, d_sig, _ = _composite(inp, S, 0.0, flags, "dense")
    m_feat, m_sig, mask = _composite(inp, S, 0.0, flags, "live")
    l_feat, l_sig, _ = _composite(inp, S, 0.0, flags, "listed")
    torch.cuda.synchronize()
    listed = _listed_mask(idx, count, rr.N * S).view(rr.B, rr.N, S).to(d)
    assert int(mask.max()) <= 1
    mask = mask.bool()
    assert torch.isfinite(d_feat).all() and torch.isfinite(d_sig).all()
    assert not bool((d_feat == SENTINEL).any()) and not bool((d_sig == SENTINEL).any())
    # masked: every dsigma and the live rows are the dense ones, the other rows untouched
    assert torch.equal(m_sig, d_sig) and torch.equal(m_feat[mask], d_feat[mask])
    assert bool((m_feat[~mask] == SENTINEL).all())
    # listed: the listed rows and dsigmas are the dense ones, the others untouched
    assert torch.equal(l_feat[listed], d_feat[listed]) and torch.equal(l_sig[listed], d_sig[listed])
    assert bool((l_feat[~listed] == SENTINEL).all()) and bool((l_sig[~listed] == SENTINEL).all())
    # skipping loses nothing
    assert not bool((mask & ~listed).any()), "a sample the backward calls live is missing from the list"
    assert bool((d_feat[~listed] == 0).all()) and bool((d_sig[~listed] == 0).all())
    assert bool((d_feat[~mask] == 0).all()) and bool((d_sig[~mask] == 0).all())
    # the two new cases
    last = torch.zeros_like(listed)
    last[..., -1] = bool(flags & 1)
    zero_gate = (x == 0) & rr.is_class(r, "zeros").to(d).unsqueeze(-1) & ~last
    assert bool(zero_gate.any()) and not bool((listed & zero_gate).any()) and not bool((mask & zero_gate).any())
    dark = listed & ~mask & rr.is_class(r, "wall").to(d).unsqueeze(-1) & (x > 0)
    print(f"liveness S={S} flags {flags}: listed {int(listed.sum())}, masked {int(mask.sum())}, dark wall samples {int(dark.sum())}")
    if S - S // 2 >= 6:
        assert bool(dark.any())


# --------------------------------------------------------------------------------------
# 3. the resampler
# --------------------------------------------------------------------------------------
def _resample(r, S, u, cdf_in=None, rays=None, with_dirs=True):
    from cips3d_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(17)
    orig = torch.randn(rr.B, 3, generator=g).to(d)
    dirs = torch.randn(R, 3, generator=g).to(d)
    return ops.resample_fwd(r["x"].view(R, S).to(d), r["z"].view(R, S).to(d), None, 0.0, u.to(d), orig if with_dirs else None,
                            dirs if with_dirs else None, rr.B, rr.N, S, 0, debug=True, cdf_in=cdf_in.to(d) if cdf_in is not None else None,
                            rays=rays)


def _edge_draws(cdf, S):
    """u (R, S) for a cdf (R, S - 1): slot 0 is exactly 0, slot 1 is 1 - 2^-24 (the two ends of torch.rand's range), the others
    are cdf entries bit for bit or their neighbours in fp32, entry and direction walking with the ray and the slot.  The cdf's
    first entry (0) has no lower neighbour in torch.rand's range and is copied instead."""
    Rn = cdf.shape[0]
    u = torch.empty(Rn, S)
    u[:, 0] = 0.0
    u[:, 1] = 1 - 2.0 ** -24
    ray = torch.arange(Rn)
    for i in range(2, S):
        j = (ray + i) % (S - 1)
        c = cdf[ray, j]
        mode = (ray // (S - 1) + i) % 3
        up, down = torch.nextafter(c, torch.full_like(c, 2.0)), torch.nextafter(c, torch.full_like(c, -1.0))
        u[:, i] = torch.where(mode == 1, up, torch.where((mode == 2) & (c > 0), down, c))
    return u


@pytest.mark.parametrize("S", rr.FLAT_S)
def test_resample_bookkeeping_on_the_edges(S):
    """on the fp32 oracle's cdf (cdf_in) and draws that sit on, just above and just below its entries, at 0 and at 1 - 2^-24: the
    indices are torch.searchsorted's bit for bit and fine_z follows; both ends of the index range are reached"""
    r, _, _ = _set(S, False, False)
    _, book = rr.oracle_resample(r["x"], r["z"], rr.uniform_draws(R, S, rr.SEED_U), F32)
    cdf = book["cdf"]
    u = _edge_draws(cdf, S)
    fz, book = rr.oracle_resample(r["x"], r["z"], u, F32)
    assert torch.equal(book["cdf"], cdf)
    inds = book["inds"]
    assert bool((inds == 0).any()) and bool((inds == S - 1).any()), "the draws miss an end of the index range"
    assert bool((inds[:, 0] == 0).all())
    on_entry = (u.unsqueeze(-1) == cdf.unsqueeze(1)).any(-1)
    assert bool(on_entry[:, 2:].any()) and bool((~on_entry[:, 2:]).any())
    fz_x, _, _, cdf_x, inds_x = _resample(r, S, u, cdf_in=cdf)
    torch.cuda.synchronize()
    assert torch.equal(cdf_x.cpu(), cdf)
    assert torch.equal(inds_x.cpu(), inds), "searchsorted indices differ on identical float inputs"
    e = max_rel(fz_x, fz)
    print(f"resample edges S={S}: ind == 0 at {int((inds == 0).sum())}, ind == S - 1 at {int((inds == S - 1).sum())} of {inds.numel()} "
          f"draws; fine_z {e:.2e}")
    assert e < 1e-6


@pytest.mark.parametrize("S", rr.FLAT_S)
def test_resample_end_to_end_on_the_step_cdf(S):
    """the kernel's own weights and cdf, random draws.  Weights and cdf at the existing 1e-5 of the fp32 oracle; at most 1e-3 of
    the indices off the fp64 oracle's; fine_z at the agreeing indices no further from the fp64 oracle than four times the fp32
    oracle's own distance plus 1e-6 (on a step cdf (u - c0) / denom divides a one-ulp cdf difference by a bin of ~2e-5, so the
    reference itself is that far off; a sample in a wrong bin moves by ~1e-2).
    Measured on an MI355X host, reference distance / product distance: S = 3: 1.12e-07 / 1.05e-07, S = 9: 1.25e-07 / 1.10e-07,
    S = 24: 8.28e-06 / 1.58e-05, no index off at any S.  The reference distance depends on the host's
    expf: another CPU gave 3.84e-06 at S = 24."""
    r, _, _ = _set(S, False, False)
    u = rr.uniform_draws(R, S, rr.SEED_U)
    fz32, b32 = rr.oracle_resample(r["x"], r["z"], u, F32)
    fz64, b64 = rr.oracle_resample(r["x"], r["z"], u, F64)
    mism32, dist32 = rr.resample_distance(fz32, b32["inds"], fz64, b64["inds"])
    fz_d, _, w_d, cdf_d, inds_d = _resample(r, S, u)
    torch.cuda.synchronize()
    mism, dist = rr.resample_distance(fz_d, inds_d, fz64, b64["inds"])
    print(f"resample end to end S={S}: index mismatch vs fp64 {mism:.2e} (fp32 oracle {mism32:.2e}); fine_z distance from fp64: "
          f"reference {dist32:.3e} product {dist:.3e}")
    assert max_rel(w_d, b32["weights"]) < 1e-5
    assert max_rel(cdf_d, b32["cdf"]) < 1e-5
    assert mism <= 1e-3
    assert dist <= 4 * dist32 + 1e-6


def _ray_grids(H, W, S, d):
    xg = torch.linspace(-1, 1, W, device=d); yg = torch.linspace(1, -1, H, device=d); zg = torch.linspace(rr.Z0, rr.Z1, S, device=d)
    zc = float(-1.0 / math.tan((2 * math.pi * rr.FOV / 360) / 2))
    return xg, yg, zg, zc


@pytest.mark.parametrize("S", rr.FLAT_S)
def test_resample_in_kernel_rays_give_the_same_depths(S):
    """rays= (directions and origins formed in the kernel, what the generator uses) on a 1 x 67 image per batch entry: fine_z is
    the origins / dirs form's bit for bit on the same sigma, z and u, and no fine points are returned"""
    from cips3d_amd import ops
    d = dev()
    r, _, _ = _set(S, False, False)
    u = rr.uniform_draws(R, S, rr.SEED_U)
    xg, yg, zg, zc = _ray_grids(1, rr.N, S, d)
    c2w = torch.eye(4).repeat(rr.B, 1, 1)
    c2w[:, :3, 3] = torch.tensor([[0.1, -0.2, 1.0], [-0.3, 0.05, 0.9]])
    c2w = c2w.to(d).contiguous()
    rp = ops._ray_params(xg, yg, zg, zc, c2w, None, 1, rr.N, S)
    fz_a, fp_a, w_a, cdf_a, inds_a = _resample(r, S, u)
    fz_b, fp_b, w_b, cdf_b, inds_b = _resample(r, S, u, rays=rp, with_dirs=False)
    torch.cuda.synchronize()
    assert fp_b is None and fp_a is not None and torch.isfinite(fz_a).all()
    assert torch.equal(fz_b, fz_a) and torch.equal(inds_b, inds_a) and torch.equal(w_b, w_a) and torch.equal(cdf_b, cdf_a)


@pytest.mark.parametrize("flags", [0, 3])
def test_resampled_depths_composite(flags):
    """the chain: the kernel's own fine_z on the step-cdf rays (samples crowd into one bin, deltas down to ~1e-7) merged with
    the coarse samples and composited, against the fp64 oracle on that same fine_z, at the compositing bars"""
    S = 24
    r, _, _ = _set(S, False, False)
    fz = _resample(r, S, rr.uniform_draws(R, S, rr.SEED_U))[0]
    torch.cuda.synchronize()
    fz = fz.cpu().view(rr.B, rr.N, S)
    allz = torch.cat([fz, r["z"]], -1).sort(-1).values
    gaps = allz[..., 1:] - allz[..., :-1]
    print(f"chain: smallest positive gap of the merged depths {float(gaps[gaps > 0].min()):.2e}")
    assert float(gaps[gaps > 0].min()) < 1e-5
    _hier(S, "relu", flags, zf=fz, what="chain")


# --------------------------------------------------------------------------------------
# 4. the fused march and its backward
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _march_ref(H, W, S, flags, seed):
    G = seeded_generator(11)
    m = rr.build_march(H, W, S, flags, seed)
    return G, m, rr.oracle_march64(G, m, H, W, S, flags)


@pytest.mark.parametrize("H,W,S,flags,seed", rr.MARCH_CASES)
def test_march_on_the_ray_classes(H, W, S, flags, seed, monkeypatch):
    """cips_march_fwd_x3 with every optional output, then net.march forward + backward on three paths (the live lists made in
    the forward pass, in the backward pass, and the dense backward), b = 3, the class values on the noise input with
    noise_std = 1, against rays -> siren -> integrate in fp64.  In the flags-0 case image 0 is all empty: its style gradient is
    exactly 0 on every path."""
    from cips3d_amd import ops, _lib
    from cips3d_amd._lib import check
    d = dev()
    b, n = rr.MARCH_B, H * W
    G, m, o = _march_ref(H, W, S, flags, seed)
    net = seeded_generator(11).to(d).siren
    lib = _lib.load()
    xg, yg, zg, zc = _ray_grids(H, W, S, d)
    c2w = o["cam2world"].float().to(d).contiguous()
    std = m["style"].to(d).requires_grad_(True)
    sdict = {"nerf_w0": std, "nerf_w1": std, "nerf_rgb": std}
    t = {}
    t["g0"], t["p0"] = net.network[0].film(std); t["g1"], t["p1"] = net.network[1].film(std); t["gc"], t["pc"] = net.color_layer_sine.film(std)
    t.update(w0=net.network[0].linear.weight, b0=net.network[0].linear.bias, w1=net.network[1].linear.weight, b1=net.network[1].linear.bias,
             ws=net.final_layer.weight, bs=net.final_layer.bias, wc=net.color_layer_sine.linear.weight, bc=net.color_layer_sine.linear.bias,
             wf=net.color_layer_linear[0].weight, bf=net.color_layer_linear[0].bias)
    tt = {k: v.detach().contiguous() for k, v in t.items()}
    sw = ops._siren_struct(tt)
    jd, nd = m["jitter"].to(d).contiguous(), m["noise"].to(d).contiguous()
    rp = ops._ray_params(xg, yg, zg, zc, c2w, jd, H, W, S)
    o_fea = torch.empty(b, n, 32, device=d); o_depth = torch.empty(b, n, device=d); o_w = torch.full((b, n, S), float("nan"), device=d)
    o_feat = torch.empty(b, n * S, 32, device=d); o_sig = torch.empty(b, n * S, device=d); o_z = torch.empty(b, n * S, device=d)
    P = lambda v: C.c_void_p(v.data_ptr())
    check(lib.cips_march_fwd_x3(C.byref(sw), C.byref(rp), P(nd), 1.0, ops._CLAMP["relu"], flags, P(o_fea), P(o_depth), P(o_w),
                                P(o_feat), P(o_sig), P(o_z), b, None, None, ops._stream()), "march")
    torch.cuda.synchronize()
    # the gates first: the kernel's sigma + noise has the fp64 oracle's sign at every sample
    gate = (o_sig.view(b, n, S) + nd) > 0
    assert torch.equal(gate.cpu(), o["x"] > 0), "a relu gate differs from the fp64 oracle's"
    e = [max_rel(o_z.view(b, n, S), o["z"]), max_rel(o_feat.view(b, n, S, 32), o["out"][..., :32]),
         max_rel(o_sig.view(b, n, S), o["out"][..., 32]), max_rel(o_w, o["w"]), max_rel(o_fea, o["fea"]), max_rel(o_depth, o["depth"])]
    print(f"march {H}x{W} S={S} flags {flags}: z {e[0]:.2e} feat {e[1]:.2e} sigma {e[2]:.2e} weights {e[3]:.2e} fea {e[4]:.2e} "
          f"depth {e[5]:.2e}; open gates {float(gate.float().mean()):.3f}")
    assert e[0] < 1e-6 and max(e[1:]) < 2e-4
    # ---- backward through net.march on the three paths ----
    params = dict(net.named_parameters())
    up = m["up"].to(d)

    def run(lists_in_forward):
        geom = (b, H, W, S, zc, 1.0, ops._CLAMP["relu"], flags, True, lists_in_forward)
        for p in list(params.values()) + [std]:
            p.grad = None
        fea, _ = net.march(sdict, geom, xg, yg, zg, c2w, jd, nd)
        ops.live_forward_join()
        (fea * up).sum().backward()
        torch.cuda.synchronize()
        assert not ops._LIVE_PENDING
        return {**{k: p.grad.clone() for k, p in params.items()}, "style": std.grad.clone()}

    calls = []
    real = ops.live_plan_forward
    monkeypatch.setattr(ops, "live_plan_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(ops, "SIREN_BWD_LIVE", True)
    monkeypatch.setattr(ops, "SIREN_BWD_EVEN", True)
    monkeypatch.setattr(ops, "SIREN_LIVE_FWD", True)
    got = {"lists in forward": run(True)}
    assert len(calls) == 1
    monkeypatch.setattr(ops, "SIREN_LIVE_FWD", False)
    got["lists in backward"] = run(True)
    assert len(calls) == 1
    monkeypatch.setattr(ops, "SIREN_BWD_LIVE", False)
    got["dense"] = run(True)
    want = {**o["grads"], "style": o["dstyle"]}
    for path, gr in got.items():
        errs = {k: rel_err(gr[k], want[k]) for k in want}
        worst = max(errs, key=errs.get)
        print(f"march backward, {path}: worst gradient rel err {errs[worst]:.3e} ({worst})")
        for k, v in errs.items():
            assert torch.isfinite(gr[k]).all(), (path, k)
            assert v < TOL, (path, k, v)
        if flags == 0:
            assert bool((gr["style"][0] == 0).all()), path
            assert bool((gr["style"][1:] != 0).any())
    for a, c in (("lists in forward", "lists in backward"), ("lists in forward", "dense"), ("lists in backward", "dense")):
        for k in want:
            assert rel_err(got[a][k], got[c][k]) < TOL, (a, c, k)
