"""CPU: the reference of tests/test_gpu_depth_gradient.py.  oracle.integrate returns depth as an autograd tensor, and the opacity
is the sum of its weights before the last_back top-up (integrate(..., last_back=False)[2].sum(2): those weights do not depend
on last_back).  On the inputs of tests/render_regimes.py the loss  sum(fea * up) + sum(depth * ud) + sum(opacity * uo)  and its
depth-only and opacity-only parts are differentiated in fp32 and in fp64:
  * the fp32 oracle stays within the GPU file's bars of the fp64 oracle (max_rel < 1e-5 for depth / opacity, rel_err < 1e-4 for
    the gradients) — measured: depth / opacity <= 1.8e-7, dx <= 4.1e-7 for all three losses;
  * the depth-only and the opacity-only gradients are finite and non-zero in every case, last_back included (opacity is not
    the constant 1 there);
  * a ray of class `empty` gets exactly zero dx from both upstreams under relu (what the live-sample lists rely on)."""
import functools

import pytest
import torch

import render_regimes as rr
from conftest import max_rel, rel_err

F32, F64 = torch.float32, torch.float64
CLAMP_FLAGS = [("relu", 0), ("relu", 1), ("relu", 2), ("relu", 3), ("softplus", 0), ("softplus", 3)]
LOSSES = {"all": (1, 1, 1), "depth": (0, 1, 0), "opacity": (0, 0, 1)}      # which of (fea, depth, opacity) the loss holds
ALL_S = (3, 9, 24, 48)


def geo_upstreams(b, n, seed):
    """-> ud, uo (b, n): the upstream gradients of depth and opacity"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, n, generator=g), torch.randn(b, n, generator=g)


def noise_draw(E, clamp):
    """tests/test_gpu_render_regimes.py's _noise: softplus runs with a noise draw, relu has none"""
    if clamp != "softplus":
        return None, 0.0
    return torch.randn(rr.B, rr.N, E, generator=torch.Generator().manual_seed(90 + E)), 0.3


@functools.lru_cache(maxsize=None)
def flat_set(S, soft):
    """tests/test_gpu_render_regimes.py's _set for the coarse draw, with the two geometric upstreams
    -> r, feat (b, n, S, 32), up (b, n, 32), ud, uo (b, n)"""
    r = (rr.build_softplus if soft else rr.build)(rr.B, rr.N, S, rr.SEED_SOFT if soft else rr.SEED_COARSE)
    feat, up = rr.features(rr.B, rr.N, S, 7 + S)
    return (r, feat, up) + geo_upstreams(rr.B, rr.N, 70 + S)


def oracle_composite_geo(feat, x, z, up, ud, uo, clamp, flags, dtype, noise=None, noise_std=0.0, terms=(1, 1, 1)):
    """rr.oracle_composite for the loss  terms[0] sum(fea * up) + terms[1] sum(depth * ud) + terms[2] sum(opacity * uo),
    opacity = integrate(..., last_back=False)[2].sum(2), on inputs in compositing order
    -> dict(fea, depth, opacity, w, dfeat, dx) in `dtype`"""
    from oracle import cips3d_oracle as orc
    f = feat.to(dtype).clone().requires_grad_(True)
    s = x.to(dtype).clone().requires_grad_(True)
    nz = (noise if noise is not None else torch.zeros_like(x)).to(dtype).unsqueeze(-1)
    rs, zz = torch.cat([f, s.unsqueeze(-1)], -1), z.to(dtype).unsqueeze(-1)
    fea, depth, w = orc.integrate(rs, zz, nz, noise_std, clamp_mode=clamp, last_back=bool(flags & 1), white_back=bool(flags & 2))
    opacity = orc.integrate(rs, zz, nz, noise_std, clamp_mode=clamp, last_back=False)[2].sum(2).squeeze(-1)
    depth = depth.squeeze(-1)
    loss = terms[0] * (fea * up.to(dtype)).sum() + terms[1] * (depth * ud.to(dtype)).sum() + terms[2] * (opacity * uo.to(dtype)).sum()
    loss.backward()
    return dict(fea=fea.detach(), depth=depth.detach(), opacity=opacity.detach(), w=w.detach().squeeze(-1), dfeat=f.grad, dx=s.grad)


@functools.lru_cache(maxsize=None)
def flat_ref(S, clamp, flags, loss, dtype=F64):
    r, feat, up, ud, uo = flat_set(S, clamp == "softplus")
    noise, noise_std = noise_draw(S, clamp)
    return oracle_composite_geo(feat, r["x"], r["z"], up, ud, uo, clamp, flags, dtype, noise, noise_std, LOSSES[loss])


@pytest.mark.parametrize("S", ALL_S)
@pytest.mark.parametrize("clamp,flags", CLAMP_FLAGS)
def test_oracle_depth_and_opacity_gradients(S, clamp, flags):
    r = flat_set(S, clamp == "softplus")[0]
    for loss in LOSSES:
        a, b = flat_ref(S, clamp, flags, loss, F32), flat_ref(S, clamp, flags, loss, F64)
        e = dict(depth=max_rel(a["depth"], b["depth"]), opacity=max_rel(a["opacity"], b["opacity"]), dx=rel_err(a["dx"], b["dx"]))
        print(f"oracle fp32 vs fp64 S={S} {clamp} flags {flags} loss {loss}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
        assert e["depth"] < 1e-5 and e["opacity"] < 1e-5 and e["dx"] < 1e-4, (loss, e)
        for ref in (a, b):
            assert torch.isfinite(ref["dx"]).all() and torch.isfinite(ref["dfeat"]).all(), loss
            assert float(ref["dx"].abs().max()) > 0, (loss, "a zero gradient")
            if loss != "all":
                assert bool((ref["dfeat"] == 0).all()), (loss, "the features do not enter this loss")
            if clamp == "relu":
                empty = rr.is_class(r, "empty")
                assert bool(empty.any()) and bool((ref["dx"][empty] == 0).all()), (loss, "an empty ray with a gradient")
    # opacity is the sum of the weights before the top-up: the same numbers with and without last_back, and not the constant 1
    b = flat_ref(S, clamp, flags, "all", F64)
    assert torch.equal(b["opacity"], flat_ref(S, clamp, flags & 2, "all", F64)["opacity"])
    assert float((b["opacity"] - 1).abs().max()) > 0.5
    if flags & 1:
        assert max_rel(b["w"].sum(-1), torch.ones_like(b["opacity"])) < 1e-12
