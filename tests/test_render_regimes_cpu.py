"""CPU: the ray classes of tests/render_regimes.py do on the oracle what their names say, and the fp32 oracle is a usable
reference on them (finite gradients, within the compositing bars of the fp64 oracle, the resampler's indices equal to the fp64
ones).  What holds here is what tests/test_gpu_render_regimes.py relies on when it feeds these tensors to the kernels."""
import functools

import pytest
import torch

import render_regimes as rr
from conftest import max_rel, rel_err, seeded_generator

F32, F64 = torch.float32, torch.float64


@functools.lru_cache(maxsize=None)
def _flat(S, soft=False):
    r = rr.build_softplus(rr.B, rr.N, S, rr.SEED_SOFT) if soft else rr.build(rr.B, rr.N, S, rr.SEED_COARSE)
    feat, up = rr.features(rr.B, rr.N, S, 7 + S)
    return r, feat, up


def _alpha_T(r):
    """alpha (b, n, S) and the transmittance in front of every sample plus the one behind the last (b, n, S + 1), as
    oracle.integrate forms them in fp32"""
    x, z = r["x"], r["z"]
    d = torch.cat([z[..., 1:] - z[..., :-1], 1e10 * torch.ones_like(z[..., :1])], -1)
    a = 1 - torch.exp(-d * torch.relu(x))
    T = torch.cumprod(torch.cat([torch.ones_like(a[..., :1]), 1 - a + 1e-10], -1), -1)
    return a, T


@pytest.mark.parametrize("S", rr.FLAT_S)
def test_every_class_does_what_the_table_says(S):
    r, feat, up = _flat(S)
    x, z, k = r["x"], r["z"], S // 2
    assert x.dtype == F32 and z.dtype == F32
    assert bool((z[..., 1:] - z[..., :-1] >= rr.min_delta(S) * (1 - 1e-4)).all())
    for name in rr.CLASSES:
        assert float(rr.is_class(r, name).float().mean()) >= 0.1, name
    assert rr.min_gate_margin(r) >= 1e-4
    a, T = _alpha_T(r)
    o = {fl: rr.oracle_composite(feat, x, z, up, "relu", fl, F32) for fl in (0, 1, 2, 3)}
    w = o[0]["w"]
    for fl in o:
        assert torch.isfinite(o[fl]["dfeat"]).all() and torch.isfinite(o[fl]["dx"]).all(), fl
    # surface: alpha_k == 1.0f, and with nothing in front of it that is the weight
    m = rr.is_class(r, "surface")
    assert bool((x[m][:, :k] <= -1).all())
    assert bool((a[m][:, k] == 1).all()) and bool((w[m][:, k] == 1).all())
    assert bool((w[m][:, :k] == 0).all())
    assert bool((w[m][:, k + 1:] <= 1.5e-10).all())           # T = 1e-10 behind the surface
    # wall: alpha == 1.0f from k on; the running T is 0 at the end where five samples have cut it
    m = rr.is_class(r, "wall")
    assert bool((a[m][:, k:] == 1).all())
    if S - k >= 5:
        assert bool((T[m][:, -1] == 0).all())
    if S - k >= 6:
        assert bool((x[m][:, k + 5:] > 0).all()) and bool((w[m][:, k + 5:] == 0).all())      # open gate, no weight
    # empty
    m = rr.is_class(r, "empty")
    assert bool((x[m] <= -1).all()) and bool((w[m] == 0).all()) and bool((w[m].sum(-1) == 0).all())
    assert bool((o[1]["w"][m][:, -1] == 1).all()) and bool((o[1]["w"][m][:, :-1] == 0).all())
    assert torch.equal(o[1]["fea"][m], feat[m][:, -1]) and torch.equal(o[1]["depth"][m], z[m][:, -1])
    assert bool((o[2]["fea"][m] == 1).all())
    # last only
    m = rr.is_class(r, "last_only")
    assert bool((a[m][:, -1] == 1).all()) and bool((w[m][:, -1] == 1).all()) and bool((w[m][:, :-1] == 0).all())
    # zeros: both signs present, the gate closed at both
    m = rr.is_class(r, "zeros")
    zero = (x[m] == 0)
    neg = zero & torch.signbit(x[m])
    assert bool(neg[:, 0].all()) and bool((zero & ~neg)[:, 2].all()) and not bool(zero[:, 1].any())
    for fl in (0, 2):
        assert bool((o[fl]["w"][m][zero] == 0).all()) and bool((o[fl]["dx"][m][zero] == 0).all())
    assert bool((o[0]["dfeat"][m][zero] == 0).all())


@pytest.mark.parametrize("S", rr.FLAT_S)
def test_softplus_builder_reaches_both_ends(S):
    r, feat, up = _flat(S, soft=True)
    x, void = r["x"], r["void"]
    assert bool((x == rr.SOFT_HI).any()) and bool((x == rr.SOFT_LO).any()) and bool(((x != rr.SOFT_HI) & (x != rr.SOFT_LO)).any())
    assert float(void.float().mean()) >= 0.1
    assert float(torch.nn.functional.softplus(torch.tensor(rr.SOFT_LO))) == 0.0
    for fl in (0, 3):
        o = rr.oracle_composite(feat, x, r["z"], up, "softplus", fl, F32)
        assert torch.isfinite(o["dfeat"]).all() and torch.isfinite(o["dx"]).all()
        assert bool((o["dx"][x == rr.SOFT_LO] == 0).all())
        wv = o["w"][void]
        assert bool((wv[:, :-1] == 0).all()) and bool((wv[:, -1] == (1.0 if fl & 1 else 0.0)).all())


@pytest.mark.parametrize("S", rr.FLAT_S)
@pytest.mark.parametrize("clamp,flags", [("relu", 0), ("relu", 1), ("relu", 2), ("relu", 3), ("softplus", 0), ("softplus", 3)])
def test_fp32_oracle_is_within_the_composite_bars_of_fp64(S, clamp, flags):
    r, feat, up = _flat(S, soft=clamp == "softplus")
    o32 = rr.oracle_composite(feat, r["x"], r["z"], up, clamp, flags, F32)
    o64 = rr.oracle_composite(feat, r["x"], r["z"], up, clamp, flags, F64)
    e = {k: (rel_err if k in ("dfeat", "dx") else max_rel)(o32[k], o64[k]) for k in o32}
    print(f"fp32 vs fp64 oracle S={S} {clamp} flags {flags}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert max(e["fea"], e["depth"], e["w"]) < 1e-5
    assert max(e["dfeat"], e["dx"]) < 1e-4


@pytest.mark.parametrize("S", rr.HIER_S)
def test_fine_set_seed_keeps_the_gates_clear(S):
    """the hierarchical cases draw the same classes a second time: that draw, too, keeps every unpinned gate 1e-4 from 0"""
    assert rr.min_gate_margin(rr.build(rr.B, rr.N, S, rr.SEED_COARSE)) >= 1e-4
    assert rr.min_gate_margin(rr.build(rr.B, rr.N, S, rr.SEED_FINE)) >= 1e-4


@pytest.mark.parametrize("S", rr.FLAT_S)
def test_resampler_reference_on_the_step_cdf(S):
    """random draws on the class rays: the fp32 oracle's indices are the fp64 oracle's at every draw; its fine_z at those
    indices lies as far from the fp64 one as a one-ulp cdf difference divided by a small bin makes it (printed: the GPU test
    measures the same figure and holds the kernel to four times it)."""
    r, _, _ = _flat(S)
    u = rr.uniform_draws(rr.B * rr.N, S, rr.SEED_U)
    fz32, b32 = rr.oracle_resample(r["x"], r["z"], u, F32)
    fz64, b64 = rr.oracle_resample(r["x"], r["z"], u, F64)
    mism, dist = rr.resample_distance(fz32, b32["inds"], fz64, b64["inds"])
    last = b32["cdf"][:, -1]
    print(f"resampler reference S={S}: index mismatch {mism:.2e}, fine_z distance {dist:.2e}, "
          f"cdf[-1] < 1 - 2^-24 in {int((last < 1 - 2.0 ** -24).sum())} of {last.numel()} rays")
    assert mism == 0.0
    assert max_rel(b32["weights"], b64["weights"]) < 1e-5 and max_rel(b32["cdf"], b64["cdf"]) < 1e-5
    assert dist < 1e-3          # far below a bin width (~1e-2): a sample in a wrong bin would show


@pytest.mark.parametrize("H,W,S,flags,seed", rr.MARCH_CASES)
def test_march_inputs_keep_the_gates_clear(H, W, S, flags, seed):
    """the march cases add the class values to the network's own sigma: no fp64 sigma + noise lies within 1e-4 of 0 (the fp32
    kernels then take the oracle's branch everywhere), every class keeps its share, and image 0 of the flags-0 case is empty"""
    G = seeded_generator(11)
    m = rr.build_march(H, W, S, flags, seed)
    o = rr.oracle_march64(G, m, H, W, S, flags)
    assert float(o["x"].abs().min()) >= 1e-4
    for i, name in enumerate(rr.CLASSES):
        assert float((m["cls"][1:] == i).float().mean()) >= 0.1, name
    if flags == 0:
        assert bool((o["x"][0] < 0).all()) and bool((o["w"][0] == 0).all()) and bool((o["dstyle"][0] == 0).all())
        assert float(o["dstyle"][1:].abs().min()) > 0
    assert all(torch.isfinite(g).all() for g in o["grads"].values()) and torch.isfinite(o["dstyle"]).all()
    assert all(p.grad is None for p in G.parameters())


def test_rectangular_rays_are_the_oracles_on_a_square():
    """render_regimes._rays64 (H x W images) against oracle.rays on 8 x 8"""
    from oracle import cips3d_oracle as orc
    H = W = 8
    S = 9
    m = rr.build_march(H, W, S, 3, 5)
    torch.set_default_dtype(F64)
    try:
        mine = rr._rays64(orc, rr.MARCH_B, H, W, S, m)
        ref = orc.rays(rr.MARCH_B, H, rr.FOV, rr.Z0, rr.Z1, S, m["jitter"].double().unsqueeze(-1), m["theta"].double(),
                       m["phi"].double(), 0.3, 0.155)
    finally:
        torch.set_default_dtype(F32)
    assert max_rel(mine["points"], ref["points"]) < 1e-12 and max_rel(mine["z"], ref["z"]) < 1e-14
    assert torch.equal(mine["cam2world"], ref["cam2world"])
