"""The references of tests/siren_refs.py checked against the project's oracle and against themselves, on the CPU: what
tests/test_gpu_siren_fp64.py holds the SIREN kernels to has to be right, and its yardsticks have to be steady, before a kernel
is measured with them."""
import math

import pytest
import torch

import siren_refs as sr
from oracle import cips3d_oracle as orc

SEEDS = range(5)
B, P = 2, 513
# the sparse upstreams and the smallest shapes of the GPU tests, on the regimes they run there: (B, P, upstream pattern)
SPARSE = [(2, 513, "dsigma"), (2, 513, "dfeat"), (2, 1029, "dsigma"), (2, 1029, "dfeat")]
FEW = [(2, 513, ("onehot", 1, 511)), (2, 513, ("onehot", 1, 512)), (2, 1029, ("onehot", 1, 511)), (2, 1029, ("onehot", 1, 512)),
       (2, 1029, ("onehot", 1, 1028)), (1, 1, "dense"), (1, 31, "dense"), (2, 129, "dense")]


def _rel_rms(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def test_siren_ref_fp32_is_the_oracle_forward_and_gradients():
    """plain fp32 siren_ref == orc.siren on the init regime, outputs and autograd gradients (through gain_fc / bias_fc down to
    the generator's parameters and the style), to 1e-6 of each tensor's rms"""
    G = sr._generator(0)
    G.zero_grad()
    pts, up = sr.make_points("box", B, P, 0), sr.make_upstream(B, P, 0)
    style = sr.make_style(B, 0).requires_grad_(True)
    ref = orc.siren(dict(G.named_parameters()), pts, style)
    (ref * up).sum().backward()
    gref = {n: p.grad.clone() for n, p in G.siren.named_parameters()}
    sref = style.grad.clone()
    G.zero_grad(); style.grad = None
    out = sr.siren_ref(pts, sr.generator_tensors(G, style))
    (out * up).sum().backward()
    assert _rel_rms(out, ref) <= 1e-6
    assert len(gref) == 22
    for n, p in G.siren.named_parameters():
        assert _rel_rms(p.grad, gref[n]) <= 1e-6, n
    assert _rel_rms(style.grad, sref) <= 1e-6
    G.zero_grad()
    # make_tensors hands out the same values, detached
    with torch.no_grad():
        assert torch.equal(sr.siren_ref(pts, sr.make_tensors("init", B, 0)), out)


@pytest.fixture(scope="module")
def sweep():
    """{(regime, seed): {name: all_distances}} for the plain fp32 reference and the "bf16x2" / "fp16x2" emulations in fp32 and
    the "bf16x2" one in fp64, all against exact fp64"""
    res = {}
    for regime, (b, p, pattern) in [(r, (B, P, "dense")) for r in sr.REGIMES] + [(r, c) for r in ("init", "wide") for c in SPARSE + FEW]:
        for seed in SEEDS:
            t, pts = sr.make_tensors(regime, b, seed), sr.make_points("box", b, p, seed)
            up = sr.make_upstream(b, p, seed, pattern)
            truth = sr.evaluate(pts, t, up, torch.float64)
            res[regime, (b, p, pattern), seed] = {name: sr.all_distances(sr.evaluate(pts, t, up, dt, planes), truth)
                                 for name, dt, planes in (("f32", torch.float32, None), ("bf32", torch.float32, "bf16x2"),
                                                          ("bf64", torch.float64, "bf16x2"), ("h32", torch.float32, "fp16x2"))}
    return res


def test_yardstick_spread_sets_the_multipliers(sweep):
    """The "bf16x2" yardstick evaluated in fp32 and in fp64 are two realisations of one set of roundings; the ratio of their
    distances from exact fp64 (either way round) is the spread a kernel that applies the same roundings in its own order is
    allowed on top, and the multipliers of the GPU tests keep a factor 1.5 above the largest seen."""
    worst = {}
    for (regime, case, seed), d in sweep.items():
        if case != (B, P, "dense"):
            regime = "few-rows" if case in FEW else "part-zero"
        for q in sr.QUANTITIES:
            if q == "dbs":
                continue            # a plain sum in every realisation: exact in fp64
            for m in ("rms", "peak"):
                a, b = d["bf32"][q][m], d["bf64"][q][m]
                if a == 0 and b == 0:
                    continue        # identically zero in every realisation
                r, k = max(a / b, b / a), (regime, "fwd" if q in ("feat", "sigma") else "grad", m)
                if r > worst.get(k, (0, ""))[0]:
                    worst[k] = (r, f"{q} seed {seed}")
    print("\nyardstick spread, bf16x2 in fp32 vs in fp64: largest ratio of the distances from fp64 (and where)")
    for regime in list(sr.REGIMES) + ["part-zero", "few-rows"]:
        print(f"  {regime:10s} " + "  ".join(f"{c} {m} {worst[regime, c, m][0]:4.2f} ({worst[regime, c, m][1]})"
                                             for c in ("fwd", "grad") for m in ("rms", "peak")))
    for regime in sr.REGIMES:
        # (the forward's rms multiplier is not chosen here: 2 x yardstick + 2e-7 is the rule the forward already holds)
        assert worst[regime, "fwd", "peak"][0] <= sr.M_FWD_PEAK / 1.5, regime
        m_rms, m_peak = sr.M_GRAD[regime]
        assert worst[regime, "grad", "rms"][0] <= m_rms / 1.5 and worst[regime, "grad", "peak"][0] <= m_peak / 1.5, regime
        assert m_rms in (2, 3, 4, 6, 8) and m_peak in (3, 4, 6, 8)
    # the sparse upstream patterns run on the init and wide regimes: dsigma / dfeat alone under those regimes' multipliers
    assert worst["part-zero", "grad", "rms"][0] <= 2 / 1.5 and worst["part-zero", "grad", "peak"][0] <= 3 / 1.5
    m_rms, m_peak = sr.M_GRAD_FEW
    for b, p, pattern in FEW:
        assert sr.grad_multipliers("init", pattern, b * p) == sr.grad_multipliers("wide", pattern, b * p) == (m_rms, m_peak)
    for b, p, pattern in SPARSE + [(B, P, "dense")]:
        assert sr.grad_multipliers("init", pattern, b * p) == sr.M_GRAD["init"]
    assert worst["few-rows", "grad", "rms"][0] <= m_rms / 1.5 and worst["few-rows", "grad", "peak"][0] <= m_peak / 1.5


def test_classes_of_the_realisations(sweep):
    """the table of the issue, per regime: plain fp32 and the two emulations against fp64; bf16 planes really cost accuracy,
    fp16 planes stay in fp32's class (the bar of the forward kernel that runs on them); dbs / dbf stay under their floor's
    condition in plain fp32"""
    print("\ndistance from fp64, largest over seeds: forward rms / peak, gradient rms / peak")
    for regime in sr.REGIMES:
        for name in ("f32", "h32", "bf32"):
            col = []
            for qs in (("feat", "sigma"), [q for q in sr.QUANTITIES[2:] if q not in sr.NO_PRODUCT]):
                for m in ("rms", "peak"):
                    col.append(max(sweep[regime, (B, P, "dense"), s][name][q][m] for s in SEEDS for q in qs))
            print(f"  {regime:10s} {name:5s} " + " ".join(f"{v:9.2e}" for v in col))
        for s in SEEDS:
            d = sweep[regime, (B, P, "dense"), s]
            if regime != "spike":                # the hand-written backward of the emulation is the function's gradient
                assert all(d["bf64"][q]["rms"] < 1e-4 for q in sr.QUANTITIES), (regime, s)
            for q in ("feat", "sigma"):
                assert d["h32"][q]["rms"] <= 2 * d["f32"][q]["rms"] + 2e-7, (regime, s, q)
            assert d["bf32"]["dw1"]["rms"] > 1.5 * d["f32"]["dw1"]["rms"], (regime, s)
            for q in sr.NO_PRODUCT:             # the condition of their 1e-6 floor
                assert d["f32"][q]["rms"] < 2e-7, (regime, s, q, d["f32"][q])
            assert d["bf32"]["dbs"]["rms"] < 2e-7


def test_coarse_sine_yardstick():
    """sine_error: the kernels' documented sine accuracy (ops.py:165-166) as a yardstick of its own.  It is a draw fixed by the
    seed, it keeps what is exactly zero exactly zero, it costs accuracy where a sine's argument is amplified (spike) and
    stays in plain fp32's class elsewhere — the bars of the all-fp32 backward stay tight in every other regime."""
    print("\nfp32 yardstick with sines of 1.2e-6 over the plain one: largest ratio of the gradients' distances from fp64 (rms, peak)")
    for regime in sr.REGIMES:
        t, pts, up = sr.make_tensors(regime, B, 3), sr.make_points("box", B, P, 3), sr.make_upstream(B, P, 3)
        truth = sr.evaluate(pts, t, up, torch.float64)
        plain = sr.all_distances(sr.evaluate(pts, t, up, torch.float32), truth)
        res = sr.evaluate(pts, t, up, torch.float32, sine_error=sr.SINE_ERROR)
        again = sr.evaluate(pts, t, up, torch.float32, sine_error=sr.SINE_ERROR)
        assert all(torch.equal(res[q], again[q]) for q in res)
        coarse = sr.all_distances(res, truth)
        qs = [q for q in sr.QUANTITIES[2:] if q not in sr.NO_PRODUCT]
        r = {m: max((coarse[q][m] / plain[q][m], q) for q in qs) for m in ("rms", "peak")}
        print(f"  {regime:10s} rms {r['rms'][0]:5.1f} ({r['rms'][1]})  peak {r['peak'][0]:5.1f} ({r['peak'][1]})")
        assert all(coarse[q]["rms"] < 1e-3 for q in sr.QUANTITIES)
        assert (r["rms"][0] > 4) == (regime == "spike")
        for q in sr.NO_PRODUCT:
            assert coarse[q] == plain[q]                  # no sine in them
    # the zero-FiLM image: its sines are sin(0), and stay 0
    t, pts, up = sr.make_tensors("wide", B, 3), sr.make_points("box", B, P, 3), sr.make_upstream(B, P, 3)
    res = sr.evaluate(pts, t, up, torch.float32, sine_error=sr.SINE_ERROR)
    assert not res["dg0"][1].any() and not res["dp0"][1].any() and res["dg0"][0].any()
    assert float(sr.SINE_ERROR) == 1.2e-6


def test_every_regime_keeps_the_sine_arguments_finite():
    print("\nlargest |sine argument| / 2 pi")
    for regime in sr.REGIMES:
        big = 0.0
        for kind in ("box", "edge"):
            for seed in SEEDS:
                t, pts = sr.make_tensors(regime, B, seed), sr.make_points(kind, B, P, seed)
                assert all(bool(torch.isfinite(v).all()) for v in t)
                with torch.no_grad():
                    out, args = sr.siren_ref(pts, t, return_args=True)
                assert bool(torch.isfinite(out).all())
                for a in args:
                    assert bool(torch.isfinite(a).all())
                    big = max(big, float(a.abs().max()) / (2 * math.pi))
        print(f"  {regime:10s} {big:8.1f} revolutions")
        assert big < 1e4


def test_inputs_are_what_they_say():
    t = dict(zip(sr.NAMES, sr.make_tensors("wide", 3, 1)))
    assert all(not t[n][1].any() and t[n][0].any() and t[n][2].any() for n in sr.FILM)
    assert bool((t["g0"] < 0).any()) and float(t["g1"].abs().min()) < 1.0
    assert not sr.make_tensors("wc0", 2, 0)[sr.NAMES.index("wc")].any()
    w = sr.make_tensors("spike", 2, 0)[sr.NAMES.index("w1")]
    assert float(w.abs().max()) > 500 * float(w.abs().median())
    e = sr.make_points("edge", 2, 129, 0)
    assert bool((e == 0).all(-1).any()) and float(e.abs().max()) > 0.3 and bool((e[:, 32:40] == e[:, 24:32]).all())
    assert bool((e[:, 16:24].abs() == 0.12).all())
    assert float(sr.make_points("box", 2, 129, 0).abs().max()) <= 0.15
    up = sr.make_upstream(2, 513, 0, ("onehot", 1, 512))
    assert not up[0].any() and bool(up[1, 512].all()) and int((up != 0).sum()) == 33


def test_distances_measures():
    q64 = torch.tensor([[3.0, 4.0], [0.0, 0.0]], dtype=torch.float64)
    q = torch.tensor([[3.0, 4.5], [0.0, 0.0]])
    d = sr.distances(q, q64)
    assert d["rms"] == pytest.approx(0.1) and d["peak"] == pytest.approx(0.5 / math.sqrt(25 / 4))
    assert sr.distances(q, q64, per_image=True)["rms"] == pytest.approx(0.1)
    q[1, 0] = 1e-30                                   # a zero row must stay exactly zero
    assert sr.distances(q, q64, per_image=True)["rms"] == math.inf
    assert sr.distances(torch.zeros(3), torch.zeros(3, dtype=torch.float64)) == {"rms": 0.0, "peak": 0.0}
    # one wrong image among many shows in the per-image measure, not in the global one
    big = torch.ones(300, 8, dtype=torch.float64)
    bad = big.clone().float(); bad[7] *= 1.01
    assert sr.distances(bad, big, per_image=True)["rms"] == pytest.approx(0.01, rel=1e-3)
    assert sr.distances(bad, big)["rms"] < 1e-3
