"""GPU: differentiable depth and opacity maps — ops.CompositeGeoFunction / ops.RayMarchGeoFunction, the `_geo` entry points of
render.hip and the fused march, and G.render — against oracle.integrate / oracle.generator_forward in fp64 on the inputs of
tests/render_regimes.py.  tests/test_depth_gradient_cpu.py holds the reference and shows on the CPU that the fp32 oracle is
more than 200 times inside the bars used here.

The loss is  sum(fea * up) + sum(depth * ud) + sum(opacity * uo)  and its depth-only and opacity-only parts; opacity is the sum
of the ray's weights before the last_back top-up."""
import ctypes as C
import functools
import math

import pytest
import torch

import render_regimes as rr
from conftest import max_rel, rel_err, seeded_generator
from oracle import cips3d_oracle as orc
from test_depth_gradient_cpu import CLAMP_FLAGS, F64, LOSSES, flat_ref, flat_set, geo_upstreams, noise_draw, oracle_composite_geo
from test_gpu_kernels import TOL, dev
from test_gpu_points_gradient import B_, FOV, IMG, KW, LOOK, POS, RAY_END, RAY_START, S_, _gen_inputs
from test_gpu_render_regimes import _ray_grids
from test_gpu_siren_live_fwd import SENTINEL, _list, _listed_mask

pytestmark = pytest.mark.gpu
R = rr.B * rr.N     # 134 rays: no multiple of 32, 16 or 8 rays per workgroup
FWD_KEYS = ("fea", "depth", "opacity", "w")


def P_(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _check(got, ref, what):
    """the bars of _check_composite in tests/test_gpu_render_regimes.py: max_rel < 1e-5 forward, rel_err < 1e-4 for the gradients"""
    e = {k: (max_rel if k in FWD_KEYS else rel_err)(got[k], ref[k].reshape(got[k].shape)) for k in got}
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k, v in e.items():
        assert torch.isfinite(got[k]).all(), k
        assert v < (1e-5 if k in FWD_KEYS else 1e-4), (what, k, v)


def _loss(terms, fea, dep, opa, up, ud, uo):
    """only the terms the loss holds, so that the Function sees None for the others"""
    parts = [(fea * up).sum(), (dep * ud).sum(), (opa * uo).sum()]
    return sum(p for p, t in zip(parts, terms) if t)


# --------------------------------------------------------------------------------------
# 1. compositing, flat and hierarchical
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", rr.FLAT_S)
@pytest.mark.parametrize("clamp,flags", CLAMP_FLAGS)
def test_composite_geo_flat(S, clamp, flags):
    """CompositeGeoFunction without a fine set, three losses.  relu with flags 1 and 2 hands the class values in as noise
    (noise_std = 1) on a sigma of zeros, the other cases as sigma: the same pre-activation bits either way."""
    from cips3d_amd import ops
    d = dev()
    r, feat, up, ud, uo = flat_set(S, clamp == "softplus")
    x = r["x"].view(R, S).to(d)
    noise, noise_std = noise_draw(S, clamp)
    as_noise = clamp == "relu" and flags in (1, 2)
    for loss, terms in LOSSES.items():
        if as_noise:
            sc, nz, std = torch.zeros_like(x).requires_grad_(True), x, 1.0
        else:
            sc, nz, std = x.clone().requires_grad_(True), (noise.view(R, S).to(d) if noise is not None else None), noise_std
        fc = feat.view(R, S, 32).to(d).requires_grad_(True)
        fea, dep, opa, wts, order, zs = ops.CompositeGeoFunction.apply(fc, sc, r["z"].view(R, S).to(d), None, None, None, nz, std,
                                                                       ops._CLAMP[clamp], flags)
        assert dep.grad_fn is not None and opa.grad_fn is not None and wts.grad_fn is None
        _loss(terms, fea, dep, opa, up.view(R, 32).to(d), ud.view(R).to(d), uo.view(R).to(d)).backward()
        torch.cuda.synchronize()
        assert torch.equal(zs.cpu(), r["z"].view(R, S))
        _check(dict(fea=fea, depth=dep, opacity=opa, w=wts, dfeat=fc.grad, dx=sc.grad), flat_ref(S, clamp, flags, loss),
               f"flat S={S} {clamp} flags {flags} loss {loss}")
        if loss != "all":
            assert bool((fc.grad == 0).all()) and float(sc.grad.abs().max()) > 0


@functools.lru_cache(maxsize=None)
def _fine_set(S, soft):
    r = (rr.build_softplus if soft else rr.build)(rr.B, rr.N, S, rr.SEED_SOFT_FINE if soft else rr.SEED_FINE)
    return r, rr.features(rr.B, rr.N, S, 7 + S + 1000)[0]


@pytest.mark.parametrize("S", rr.HIER_S)
@pytest.mark.parametrize("clamp,flags", CLAMP_FLAGS)
def test_composite_geo_hierarchical(S, clamp, flags):
    """with a fine set, E = 2 S = 18, 48, 96 (E = 96: 16 rays per workgroup in the backward), against the fp64 oracle on the
    inputs gathered by the product's own merge order, as _hier of tests/test_gpu_render_regimes.py does"""
    from cips3d_amd import ops
    d = dev()
    soft = clamp == "softplus"
    E = 2 * S
    rc, featc, up, ud, uo = flat_set(S, soft)
    rf, featf = _fine_set(S, soft)
    noise, noise_std = noise_draw(E, clamp)
    all_z = torch.cat([rf["z"].view(R, S), rc["z"].view(R, S)], -1)
    all_x = torch.cat([rf["x"].view(R, S), rc["x"].view(R, S)], -1)
    all_f = torch.cat([featf.view(R, S, 32), featc.view(R, S, 32)], -2)
    for loss, terms in LOSSES.items():
        fc, ff = (t.view(R, S, 32).to(d).requires_grad_(True) for t in (featc, featf))
        sc, sf = (t["x"].view(R, S).to(d).requires_grad_(True) for t in (rc, rf))
        fea, dep, opa, wts, order, zs = ops.CompositeGeoFunction.apply(
            fc, sc, rc["z"].view(R, S).to(d), ff, sf, rf["z"].view(R, S).to(d), noise.view(R, E).to(d) if noise is not None else None,
            noise_std, ops._CLAMP[clamp], flags)
        _loss(terms, fea, dep, opa, up.view(R, 32).to(d), ud.view(R).to(d), uo.view(R).to(d)).backward()
        torch.cuda.synchronize()
        order = order.cpu().long()
        assert torch.equal(order.sort(-1).values, torch.arange(E).expand(R, E))
        assert torch.equal(zs.cpu(), all_z.gather(-1, order))
        g = lambda t: t.gather(-1, order).view(rr.B, rr.N, E)
        ref = oracle_composite_geo(all_f.gather(-2, order.unsqueeze(-1).expand(R, E, 32)).view(rr.B, rr.N, E, 32), g(all_x), g(all_z),
                                   up, ud, uo, clamp, flags, F64, noise, noise_std, terms)
        # the oracle's gradients back from compositing order to [fine, coarse]
        dfeat = torch.zeros(R, E, 32, dtype=F64).scatter_(-2, order.unsqueeze(-1).expand(R, E, 32), ref["dfeat"].view(R, E, 32))
        dx = torch.zeros(R, E, dtype=F64).scatter_(-1, order, ref["dx"].view(R, E))
        ref = dict(fea=ref["fea"], depth=ref["depth"], opacity=ref["opacity"], w=ref["w"], dfeat_f=dfeat[:, :S], dfeat_c=dfeat[:, S:],
                   dx_f=dx[:, :S], dx_c=dx[:, S:])
        got = dict(fea=fea, depth=dep, opacity=opa, w=wts, dfeat_f=ff.grad, dfeat_c=fc.grad, dx_f=sf.grad, dx_c=sc.grad)
        _check(got, ref, f"hier S={S} {clamp} flags {flags} loss {loss}")


# --------------------------------------------------------------------------------------
# 2. NULL upstreams / a NULL opacity change nothing
# --------------------------------------------------------------------------------------
def _bwd(name, inp, S, hier, noise_std, clamp, flags, order, geo):
    """one compositing backward (`name`: "" dense, "_live", "_listed") through the old entry point (geo None) or its `_geo`
    form (geo = (ddepth, dopacity), either may be None) on SENTINEL-prefilled outputs
    -> [dfeat_c, dsig_c, dfeat_f, dsig_f, live_c, live_f] (None where the form has none)"""
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    fc, sc, zc, ff, sf, zf, noise, dfea = inp
    full = lambda *s, dt=torch.float32, v=SENTINEL: torch.full(s, v, dtype=dt, device=dev())
    out = [full(R, S, 32), full(R, S), full(R, S, 32) if hier else None, full(R, S) if hier else None, None, None]
    nz = P_(noise) if noise_std else None
    cm = ops._CLAMP[clamp]
    tail = () if geo is None else (P_(geo[0]), P_(geo[1]))
    fn = getattr(lib, "cips_composite_bwd" + name + ("" if geo is None else "_geo"))
    if name == "_listed":
        assert not hier
        args = (P_(fc), P_(sc), P_(zc), nz, float(noise_std), P_(dfea), P_(out[0]), P_(out[1]), R, S, cm, flags)
    else:
        args = (P_(fc), P_(sc), P_(zc), P_(ff), P_(sf), P_(zf), nz, float(noise_std), P_(order), P_(dfea), P_(out[0]), P_(out[1]),
                P_(out[2]), P_(out[3]))
        if name == "_live":
            out[4] = full(R, S, dt=torch.uint8, v=7)
            out[5] = full(R, S, dt=torch.uint8, v=7) if hier else None
            args += (P_(out[4]), P_(out[5]))
        args += (R, S, cm, flags, None)
    _lib.check(fn(*args, *tail, ops._stream()), fn.__name__)
    return out


def _fwd(inp, S, hier, noise_std, clamp, flags, opacity):
    """cips_composite_fwd (opacity None) or cips_composite_fwd_geo (opacity False: NULL, True: an output)
    -> [fea, depth, weights, order, zsorted, opacity or None]"""
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    fc, sc, zc, ff, sf, zf, noise, _ = inp
    E = 2 * S if hier else S
    d = dev()
    out = [torch.full((R, 32), SENTINEL, device=d), torch.full((R,), SENTINEL, device=d), torch.full((R, E), SENTINEL, device=d),
           torch.full((R, E), -7, dtype=torch.int32, device=d), torch.full((R, E), SENTINEL, device=d),
           torch.full((R,), SENTINEL, device=d) if opacity else None]
    args = (P_(fc), P_(sc), P_(zc), P_(ff), P_(sf), P_(zf), P_(noise) if noise_std else None, float(noise_std), P_(out[0]), P_(out[1]),
            P_(out[2]), P_(out[3]), P_(out[4]), R, S, ops._CLAMP[clamp], flags, None, None)
    if opacity is None:
        _lib.check(lib.cips_composite_fwd(*args, ops._stream()), "cips_composite_fwd")
    else:
        _lib.check(lib.cips_composite_fwd_geo(*args, P_(out[5]), ops._stream()), "cips_composite_fwd_geo")
    return out


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _raw_inputs(S, hier, clamp):
    d = dev()
    soft = clamp == "softplus"
    rc, featc, up, ud, uo = flat_set(S, soft)
    noise, noise_std = noise_draw(2 * S if hier else S, clamp)
    fin = [None, None, None]
    if hier:
        rf, featf = _fine_set(S, soft)
        fin = [featf.view(R, S, 32).to(d).contiguous(), rf["x"].view(R, S).to(d).contiguous(), rf["z"].view(R, S).to(d).contiguous()]
    inp = [featc.view(R, S, 32).to(d).contiguous(), rc["x"].view(R, S).to(d).contiguous(), rc["z"].view(R, S).to(d).contiguous(), *fin,
           noise.reshape(R, -1).to(d).contiguous() if noise is not None else None, up.view(R, 32).to(d).contiguous()]
    return inp, noise_std, ud.view(R).to(d).contiguous(), uo.view(R).to(d).contiguous()


@pytest.mark.parametrize("S,hier,clamp,flags", [(9, False, "relu", 3), (24, False, "softplus", 1), (9, True, "relu", 1),
                                                 (48, True, "softplus", 2)])
def test_null_upstreams_and_null_opacity_store_the_old_bits(S, hier, clamp, flags):
    """ddepth = dopacity = NULL: the `_geo` backwards store torch.equal results to cips_composite_bwd / _live / _listed on
    sentinel-prefilled buffers — rows, dsigmas, masks and the untouched sentinels.  opacity = NULL: cips_composite_fwd_geo equals
    cips_composite_fwd in every output, and so does the call that stores an opacity."""
    inp, noise_std, ud, uo = _raw_inputs(S, hier, clamp)
    old = _fwd(inp, S, hier, noise_std, clamp, flags, None)
    new = _fwd(inp, S, hier, noise_std, clamp, flags, False)
    opa = _fwd(inp, S, hier, noise_std, clamp, flags, True)
    torch.cuda.synchronize()
    assert _same(old, new) and _same(old[:5], opa[:5])
    assert not bool((opa[5] == SENTINEL).any()) and torch.isfinite(opa[5]).all()
    order = old[3] if hier else None
    for name in ("", "_live") + (() if hier else ("_listed",)):
        a = _bwd(name, inp, S, hier, noise_std, clamp, flags, order, None)
        b = _bwd(name, inp, S, hier, noise_std, clamp, flags, order, (None, None))
        c = _bwd(name, inp, S, hier, noise_std, clamp, flags, order, (ud, uo))
        torch.cuda.synchronize()
        assert _same(a, b), name
        # the upstreams do reach dsigma, and never the rows that were written
        assert not torch.equal(a[1], c[1]), name
        assert torch.equal(a[0], c[0]) or name == "_live", name


# --------------------------------------------------------------------------------------
# 3. liveness with the new upstreams
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", rr.FLAT_S)
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_liveness_holds_with_geometric_upstreams(S, flags):
    """flat relu, non-zero ddepth and dopacity, dfea = 0: dense, masked and listed `_geo` backwards on sentinel-prefilled
    outputs.  What the masked and the listed call write is the dense call's bit for bit; the mask lies inside the list of
    cips_live_points_clamp; outside the list the dense dsigma (and row) equals 0."""
    d = dev()
    inp, noise_std, ud, uo = _raw_inputs(S, False, "relu")
    inp[-1] = torch.zeros_like(inp[-1])
    assert float(ud.abs().min()) > 0 and float(uo.abs().min()) > 0
    r = flat_set(S, False)[0]
    x = r["x"].to(d).contiguous()
    idx, count = _list(x, None, 0.0, flags)
    dense = _bwd("", inp, S, False, 0.0, "relu", flags, None, (ud, uo))
    live = _bwd("_live", inp, S, False, 0.0, "relu", flags, None, (ud, uo))
    lst = _bwd("_listed", inp, S, False, 0.0, "relu", flags, None, (ud, uo))
    torch.cuda.synchronize()
    listed = _listed_mask(idx, count, rr.N * S).view(R, S).to(d)
    (d_feat, d_sig), (m_feat, m_sig, mask), (l_feat, l_sig) = dense[:2], (live[0], live[1], live[4]), lst[:2]
    assert int(mask.max()) <= 1
    mask = mask.bool()
    assert torch.isfinite(d_feat).all() and torch.isfinite(d_sig).all()
    assert not bool((d_feat == SENTINEL).any()) and not bool((d_sig == SENTINEL).any())
    assert bool((d_feat == 0).all()) and float(d_sig.abs().max()) > 0          # dfea = 0: only dsigma carries the gradient
    assert torch.equal(m_sig, d_sig) and torch.equal(m_feat[mask], d_feat[mask])
    assert bool((m_feat[~mask] == SENTINEL).all())
    assert torch.equal(l_feat[listed], d_feat[listed]) and torch.equal(l_sig[listed], d_sig[listed])
    assert bool((l_feat[~listed] == SENTINEL).all()) and bool((l_sig[~listed] == SENTINEL).all())
    assert not bool((mask & ~listed).any()), "a sample the backward calls live is missing from the list"
    assert bool((d_sig[~listed] == 0).all()) and bool((d_sig[~mask] == 0).all())
    # an empty ray has no gradient at all, whatever the upstreams are
    empty = rr.is_class(r, "empty").view(R).to(d)
    assert bool((d_sig[empty] == 0).all())
    print(f"liveness S={S} flags {flags}: listed {int(listed.sum())}, masked {int(mask.sum())}, non-zero dsigma {int((d_sig != 0).sum())}")


# --------------------------------------------------------------------------------------
# 4. the fused march
# --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _march_ref(H, W, S, flags, seed, loss):
    """rr.oracle_march64's setting with the three-term loss -> dict(fea, depth, opacity, grads, dstyle, dout (b, n, S, 33): the
    gradient at the SIREN's outputs, cam2world)"""
    terms = LOSSES[loss]
    G = seeded_generator(11)
    m = rr.build_march(H, W, S, flags, seed)
    b, n = rr.MARCH_B, H * W
    ud, uo = geo_upstreams(b, n, seed + 2)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in G.named_parameters() if k.startswith("siren.")}
    style = m["style"].double().clone().requires_grad_(True)
    torch.set_default_dtype(torch.float64)
    try:
        r = rr._rays64(orc, b, H, W, S, m)
        out = orc.siren(sd, r["points"].reshape(b, n * S, 3), style).reshape(b, n, S, 33)
        out.retain_grad()
        noise = m["noise"].double().unsqueeze(-1)
        fea, depth, w = orc.integrate(out, r["z"], noise, 1.0, clamp_mode="relu", last_back=bool(flags & 1), white_back=bool(flags & 2))
        opacity = orc.integrate(out, r["z"], noise, 1.0, clamp_mode="relu", last_back=False)[2].sum(2).squeeze(-1)
        depth = depth.squeeze(-1)
        _loss(terms, fea, depth, opacity, m["up"].double(), ud.double(), uo.double()).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return dict(fea=fea.detach(), depth=depth.detach(), opacity=opacity.detach(), cam2world=r["cam2world"], dout=out.grad,
                grads={k[len("siren."):]: v.grad for k, v in sd.items()}, dstyle=style.grad, m=m, ud=ud, uo=uo)


def _march_setup(H, W, S, flags, seed):
    """the generator's SIREN on the device with build_march's inputs, as test_march_on_the_ray_classes sets them up"""
    from cips3d_amd import ops
    d = dev()
    o = _march_ref(H, W, S, flags, seed, "all")
    m = o["m"]
    net = seeded_generator(11).to(d).siren
    xg, yg, zg, zc = _ray_grids(H, W, S, d)
    c2w = o["cam2world"].float().to(d).contiguous()
    std = m["style"].to(d).requires_grad_(True)
    sdict = {"nerf_w0": std, "nerf_w1": std, "nerf_rgb": std}
    jd, nd = m["jitter"].to(d).contiguous(), m["noise"].to(d).contiguous()
    return ops, net, sdict, std, (xg, yg, zg, zc), c2w, jd, nd


@pytest.mark.parametrize("H,W,S,flags,seed", rr.MARCH_CASES)
def test_march_entry_point_with_a_null_opacity_is_the_old_one(H, W, S, flags, seed, x3):
    """cips_march_fwd_x3_geo with opacity = NULL equals cips_march_fwd_x3 in every output; with an opacity the other outputs
    are still the same bits, and the opacity is the sum of the weights (before the top-up)"""
    from cips3d_amd import _lib
    lib = _lib.load()
    ops, net, sdict, std, (xg, yg, zg, zc), c2w, jd, nd = _march_setup(H, W, S, flags, seed)
    d = dev()
    b, n = rr.MARCH_B, H * W
    tt = {k: v.detach().contiguous() for k, v in zip(ops._SIREN_NAMES, net._siren_args(sdict))}     # (kept alive: sw holds pointers)
    sw = ops._siren_struct(tt)
    rp = ops._ray_params(xg, yg, zg, zc, c2w, jd, H, W, S)

    def run(opacity):
        out = [torch.full(s, SENTINEL, device=d) for s in ((b, n, 32), (b, n), (b, n, S), (b, n * S, 32), (b, n * S), (b, n * S))]
        opa = torch.full((b, n), SENTINEL, device=d) if opacity else None
        args = (C.byref(sw), C.byref(rp), P_(nd), 1.0, ops._CLAMP["relu"], flags, *(P_(t) for t in out), b, None, None)
        if opacity is None:
            _lib.check(lib.cips_march_fwd_x3(*args, ops._stream()), "cips_march_fwd_x3")
        else:
            _lib.check(lib.cips_march_fwd_x3_geo(*args, P_(opa), ops._stream()), "cips_march_fwd_x3_geo")
        return out, opa

    old, _ = run(None)
    new, _ = run(False)
    geo, opa = run(True)
    torch.cuda.synchronize()
    assert _same(old, new) and _same(old, geo)
    wsum = old[2].double().sum(-1)
    if flags & 1:           # the stored last weight is topped up: the weights sum to 1, the opacity does not
        assert max_rel(wsum, torch.ones_like(wsum)) < 1e-6 and float((opa - 1).abs().max()) > 0.5
    else:
        assert max_rel(opa, wsum) < 1e-6
    assert not bool((opa == SENTINEL).any()) and max_rel(opa, _march_ref(H, W, S, flags, seed, "all")["opacity"]) < 1e-5


@pytest.mark.parametrize("H,W,S,flags,seed", rr.MARCH_CASES)
def test_march_geo_on_the_ray_classes(H, W, S, flags, seed, x3, monkeypatch):
    """net.march(geo=True) forward + backward of the three losses on the three backward routes (lists made in the forward, lists
    made in the backward, dense), b = 3, against rays -> siren -> integrate in fp64: depth and opacity at max_rel 1e-5, the
    reduced SIREN parameter gradients and dstyle at TOL = 1e-3, the routes with each other at TOL.  Next to each error: the same
    gradients from the oracle's own fp64 upstream at the SIREN's outputs, rounded to fp32 and fed to the SIREN backward — the
    existing chain's share of the error.  In the flags-0 case image 0 is all empty: its style gradient is exactly 0."""
    ops, net, sdict, std, (xg, yg, zg, zc), c2w, jd, nd = _march_setup(H, W, S, flags, seed)
    d = dev()
    b, n = rr.MARCH_B, H * W
    params = dict(net.named_parameters())

    def grads():
        return {**{k: p.grad.clone() for k, p in params.items()}, "style": std.grad.clone()}

    def clear():
        for p in list(params.values()) + [std]:
            p.grad = None

    def run(o, terms):
        geom = (b, H, W, S, zc, 1.0, ops._CLAMP["relu"], flags, True, True)
        clear()
        fea, dep, opa = net.march(sdict, geom, xg, yg, zg, c2w, jd, nd, geo=True)
        ops.live_forward_join()
        assert dep.grad_fn is not None and opa.grad_fn is not None
        _loss(terms, fea, dep, opa, o["m"]["up"].to(d), o["ud"].to(d), o["uo"].to(d)).backward()
        torch.cuda.synchronize()
        assert not ops._LIVE_PENDING
        return grads(), dep.detach(), opa.detach()

    for loss, terms in LOSSES.items():
        o = _march_ref(H, W, S, flags, seed, loss)
        want = {**o["grads"], "style": o["dstyle"]}
        monkeypatch.setattr(ops, "SIREN_BWD_LIVE", True)
        monkeypatch.setattr(ops, "SIREN_BWD_EVEN", True)
        monkeypatch.setattr(ops, "SIREN_LIVE_FWD", True)
        got = {}
        got["lists in forward"], dep, opa = run(o, terms)
        monkeypatch.setattr(ops, "SIREN_LIVE_FWD", False)
        got["lists in backward"] = run(o, terms)[0]
        monkeypatch.setattr(ops, "SIREN_BWD_LIVE", False)
        got["dense"] = run(o, terms)[0]
        e = (max_rel(dep, o["depth"]), max_rel(opa, o["opacity"]))
        print(f"march geo {H}x{W} S={S} flags {flags} loss {loss}: depth {e[0]:.2e} opacity {e[1]:.2e}")
        # the chain alone: the oracle's gradient at the SIREN's outputs through SirenRaysFunction's backward
        clear()
        feat, sigma, _ = net.evaluate_rays(sdict, (b, H, W, S, zc), xg, yg, zg, c2w, jitter=jd)
        dout = o["dout"].float().to(d)
        torch.autograd.backward([feat, sigma], [dout[..., :32].reshape(feat.shape).contiguous(), dout[..., 32].reshape(sigma.shape).contiguous()])
        torch.cuda.synchronize()
        chain = grads()
        for path, gr in got.items():
            errs = {k: rel_err(gr[k], want[k]) for k in want}
            worst = max(errs, key=errs.get)
            print(f"march geo backward, loss {loss}, {path}: worst gradient rel err {errs[worst]:.3e} ({worst}); the SIREN backward "
                  f"on the oracle's fp64 upstream: {rel_err(chain[worst], want[worst]):.3e} there, "
                  f"{max(rel_err(chain[k], want[k]) for k in want):.3e} at its worst")
        assert e[0] < 1e-5 and e[1] < 1e-5, (loss, e)
        for path, gr in got.items():
            for k in want:
                assert torch.isfinite(gr[k]).all(), (loss, path, k)
                assert rel_err(gr[k], want[k]) < TOL, (loss, path, k, rel_err(gr[k], want[k]))
            if flags == 0:
                assert bool((gr["style"][0] == 0).all()), (loss, path)
                assert bool((gr["style"][1:] != 0).any())
        for a, c in (("lists in forward", "lists in backward"), ("lists in forward", "dense"), ("lists in backward", "dense")):
            for k in want:
                assert rel_err(got[a][k], got[c][k]) < TOL, (loss, a, c, k)


# --------------------------------------------------------------------------------------
# 5. generator level
# --------------------------------------------------------------------------------------
def _maps(d):
    g = torch.Generator().manual_seed(501)
    return torch.randn(B_, 1, IMG, IMG, generator=g).to(d), torch.randn(B_, 1, IMG, IMG, generator=g).to(d)


def _pinned(ops, fz):
    return ops.resample_debug(pin=[fz] if fz is not None else None)


def _fine_depths(G, ops, zs, rand, hier, **cam):
    """the fine depths of this render, recorded once (None without resampling)"""
    if not hier:
        return None
    rec = []
    with torch.no_grad(), ops.resample_debug(rec=rec):
        G.render(zs, hierarchical_sample=True, rand_override=rand, **KW, **cam)
    return rec[0]


def _param_grads(G):
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in G.named_parameters()}


@pytest.mark.parametrize("hier", [False, True])
def test_render_is_forward_plus_the_geometry(hier, x3):
    """(a) render().imgs is forward()'s image bit for bit and an image-only loss gives the same parameter gradients bit for bit;
    (b) render().depth is geometry().depth bit for bit; depth and opacity keep batch b under return_aux_img"""
    ops = x3
    d = dev()
    G = seeded_generator(21, device=d)
    zs, rand, G0 = _gen_inputs(d, hier)
    fz = _fine_depths(G, ops, zs, rand, hier)
    G.zero_grad(set_to_none=True)
    with _pinned(ops, fz):
        imgs, py = G(zs, hierarchical_sample=hier, rand_override=rand, **KW)
    (imgs * G0).sum().backward()
    torch.cuda.synchronize()
    want = _param_grads(G)
    G.zero_grad(set_to_none=True)
    with _pinned(ops, fz):
        r = G.render(zs, hierarchical_sample=hier, rand_override=rand, **KW)
    assert r.depth.shape == r.opacity.shape == (B_, 1, IMG, IMG)
    assert r.imgs.grad_fn is not None and r.depth.grad_fn is not None and r.opacity.grad_fn is not None
    (r.imgs * G0).sum().backward()
    torch.cuda.synchronize()
    got = _param_grads(G)
    assert torch.equal(r.imgs, imgs) and torch.equal(r.pitch_yaw, py)
    for k in want:
        assert (want[k] is None and got[k] is None) or torch.equal(want[k], got[k]), k
    with _pinned(ops, fz):
        geo = G.geometry(zs, hierarchical_sample=hier, rand_override=rand, **KW)
    assert torch.equal(r.depth.detach(), geo.depth)
    opa = r.opacity.detach()
    assert float(opa.min()) >= 0 and float(opa.max()) <= 1 + 1e-5 and float(opa.std()) > 0
    with torch.no_grad(), _pinned(ops, fz):
        ra = G.render(zs, hierarchical_sample=hier, rand_override=rand, return_aux_img=True, **KW)
    assert ra.imgs.shape[0] == 2 * B_ and ra.pitch_yaw.shape[0] == 2 * B_ and ra.depth.shape[0] == B_ and ra.opacity.shape[0] == B_
    assert torch.equal(ra.depth, geo.depth) and torch.equal(ra.imgs[:B_], imgs.detach())


@pytest.mark.parametrize("hier", [False, True])
def test_render_geometry_gradients_against_the_oracle(hier, x3):
    """(c) the loss sum(depth * D0) + sum(opacity * O0) (no image term: no LeakyReLU gate is involved): the gradients of every
    siren.* and mapping_network_nerf.* parameter and of z_nerf against oracle.generator_forward(keep=True) in fp64 on the same
    fine depths, at TOL; the head's and the INR mapping network's parameters get None or exact zeros"""
    ops = x3
    d = dev()
    G = seeded_generator(21, device=d)
    zs, rand, _ = _gen_inputs(d, hier)
    D0, O0 = _maps(d)
    fz = _fine_depths(G, ops, zs, rand, hier)
    zs = {"z_nerf": zs["z_nerf"].clone().requires_grad_(True), "z_inr": zs["z_inr"]}
    G.zero_grad(set_to_none=True)
    with _pinned(ops, fz):
        r = G.render(zs, hierarchical_sample=hier, rand_override=rand, **KW)
    ((r.depth * D0).sum() + (r.opacity * O0).sum()).backward()
    torch.cuda.synchronize()
    got = _param_grads(G)
    got["z_nerf"] = zs["z_nerf"].grad
    # ---- the oracle, fp64 ----
    G64 = seeded_generator(21).double()
    sd = dict(G64.named_parameters())
    z64 = {"z_nerf": zs["z_nerf"].detach().cpu().double().requires_grad_(True), "z_inr": zs["z_inr"].cpu().double()}
    torch.set_default_dtype(torch.float64)
    try:
        with orc.fine_z_pin(fz.cpu().double() if hier else None):
            o = orc.generator_forward(sd, z64, {k: v.cpu().double() for k, v in rand.items()}, IMG, FOV, RAY_START, RAY_END, S_,
                                      KW["h_stddev"], KW["v_stddev"], hier, nerf_noise=0., clamp_mode=KW["clamp_mode"], keep=True)
        depth, opacity = o["depth"].reshape(B_, 1, IMG, IMG), o["weights"].sum(2).reshape(B_, 1, IMG, IMG)    # no last_back here
        ((depth * D0.cpu().double()).sum() + (opacity * O0.cpu().double()).sum()).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    e = (max_rel(r.depth, depth), max_rel(r.opacity, opacity))
    print(f"render hier={hier}: depth {e[0]:.2e} opacity {e[1]:.2e} against the fp64 oracle")
    want = {k: p.grad for k, p in sd.items()}
    want["z_nerf"] = z64["z_nerf"].grad
    errs, zeros = {}, 0
    for k in want:
        if k.startswith(("siren.", "mapping_network_nerf.")) or k == "z_nerf":
            assert got[k] is not None and torch.isfinite(got[k]).all(), k
            errs[k] = rel_err(got[k], want[k])
            if float(want[k].abs().max()) == 0:
                # sigma leaves the SIREN in front of the colour branch: its parameters get exact zeros from this loss
                assert "color_layer" in k and bool((got[k] == 0).all()), k
                zeros += 1
        else:
            assert got[k] is None or bool((got[k] == 0).all()), (k, "a gradient outside the NeRF path")
            assert want[k] is None or bool((want[k] == 0).all()), k
    worst = max(errs, key=errs.get)
    print(f"render hier={hier}: {len(errs)} gradients ({zeros} of the colour branch exactly zero), worst rel err {errs[worst]:.3e} "
          f"({worst}), z_nerf {errs['z_nerf']:.3e}")
    assert zeros < len(errs) // 2 and float(want["z_nerf"].abs().max()) > 0
    for k, v in errs.items():
        assert v < TOL, (k, v)


@pytest.mark.parametrize("hier", [False, True])
def test_render_geometry_gradients_reach_the_camera(hier, x3, monkeypatch):
    """(d) camera_pos / camera_lookup requiring grad, the same loss: both gradients finite, non-zero, and those of the same call
    under MARCH_FUSED = False (the "points" form, an independent route) to TOL"""
    ops = x3
    d = dev()
    G = seeded_generator(21, device=d)
    zs, rand, _ = _gen_inputs(d, hier)
    D0, O0 = _maps(d)
    fz = _fine_depths(G, ops, zs, rand, hier, camera_pos=POS.to(d), camera_lookup=LOOK.to(d))

    def run():
        c, l = POS.clone().to(d).requires_grad_(True), LOOK.clone().to(d).requires_grad_(True)
        G.zero_grad(set_to_none=True)
        with _pinned(ops, fz):
            r = G.render(zs, hierarchical_sample=hier, rand_override=rand, camera_pos=c, camera_lookup=l, **KW)
        ((r.depth * D0).sum() + (r.opacity * O0).sum()).backward()
        torch.cuda.synchronize()
        return r.depth.detach(), r.opacity.detach(), c.grad, l.grad

    dep, opa, gc, gl = run()
    monkeypatch.setattr(ops, "MARCH_FUSED", False)
    dep_p, opa_p, gc_p, gl_p = run()
    e = (max_rel(dep, dep_p), max_rel(opa, opa_p), rel_err(gc, gc_p), rel_err(gl, gl_p))
    print(f"render camera hier={hier}: fused vs points form: depth {e[0]:.2e} opacity {e[1]:.2e} camera_pos.grad {e[2]:.2e} "
          f"camera_lookup.grad {e[3]:.2e}")
    for v in (gc, gl, gc_p, gl_p):
        assert v.shape == (B_, 3) and torch.isfinite(v).all() and float(v.abs().max()) > 0
    assert max(e) < TOL


def test_render_on_the_frozen_nerf_has_no_geometry_gradient(x3):
    """(e) GeneratorNerfINR_freeze_NeRF: the NeRF path runs under no_grad — depth and opacity carry no grad_fn, imgs does"""
    d = dev()
    G = seeded_generator(21, freeze=True, device=d)
    zs, rand, _ = _gen_inputs(d, False)
    r = G.render(zs, hierarchical_sample=False, rand_override=rand, **KW)
    torch.cuda.synchronize()
    assert r.depth.grad_fn is None and r.opacity.grad_fn is None and r.imgs.grad_fn is not None
    assert not r.depth.requires_grad and torch.isfinite(r.depth).all() and torch.isfinite(r.opacity).all()
