"""The FiLM-SIREN kernels against fp64, each held to the class of its own arithmetic.

ops.SirenFunction is called directly, in every forward form (exact fp32 `f32`; split-operand `x3` on fp16 planes, and on bf16
planes with TRIG_MODE bit 1) and every backward form (fused `x3`, `staged`, `staged_f32`).  The truth is tests/siren_refs.py's
plain-torch SIREN in fp64 (on the CPU; from 400k points on in fp64 on the device, 64 images at a time).  The bar of a quantity —
feat, sigma and each of the 16 gradients — is a small multiple of the distance from that truth of a YARDSTICK: the same reference
evaluated in fp32, plain for the forward forms that compute in fp32 or on fp16 planes, with "bf16x2" operands for the forms on
split bf16, and with the kernels' sine accuracy (siren_refs.SINE_ERROR, ops.py:165-166) for the all-fp32 backward, which has no
operand rounding above its sines.  rms = |q - q64| / |q64| (the FiLM gradients: the worst image's own), peak = max |q - q64| /
rms value of q64.

  forward            rms <= 2 x yardstick + 2e-7           peak <= 3 x yardstick + 2e-6
  gradients, fp32    rms, peak <= 4 x yardstick (fp32 with coarse sines)
  gradients, bf16x2  rms <= m_rms x yardstick              peak <= m_peak x yardstick      (dbs, dbf: + 1e-6)

m_rms, m_peak = siren_refs.grad_multipliers, chosen from the spread of the yardstick itself: the largest ratio, over seeds 0..4,
between the distances from fp64 of the "bf16x2" yardstick evaluated in fp32 and in fp64, times 1.5, rounded up to a step of
2, 3, 4, 6, 8 and to (2, 3) at the least (tests/test_siren_refs_cpu.py prints this table and asserts the choice):

  regime / case   fwd rms  fwd peak  grad rms  grad peak
  init              1.04     1.16      1.11      1.28      -> (2, 3)
  wide              1.04     1.23      1.11      1.32      -> (2, 3)
  scaled37          1.03     1.15      1.11      1.28      -> (2, 3)
  scaled3e-4        1.32     1.31      1.11      1.28      -> (2, 3)
  spike             1.04     1.19      3.23      4.95      -> (6, 8)   ill-conditioned: a few elements carry the error
  wc0               1.04     1.16      1.11      1.28      -> (2, 3)
  part-zero           -        -       1.24      1.53      -> (2, 3)   dsigma or dfeat alone, init and wide
  few-rows          4.94     4.94      1.47      2.46      -> (3, 4)   one-hot upstreams and B * P < 512, init and wide

The few-rows line is why a case of fewer than 512 points takes its forward yardstick, and the rms value its feat and sigma are
measured against, over 512 points (the case's own, then more of the kind), and why a quantity of fewer than 32 numbers is held
to its peak bar alone: a single sigma can be a hundredth of sigma's rms value, and the "rms" of one number is one draw.

What has an fp64 value of exactly zero has to come out as exact zeros: the zero-FiLM image of the wide regime, everything
outside a one-hot upstream's image, the colour branch under a dsigma-only upstream.  Shapes: the chunk-512 edges, and the
smallest batches that select the 1024-, 2048- and 4096-point walks of x3_chunk (asserted through cips_siren_bwd_x3_chunks).
The full 32-round walk of a 4096-point chunk needs about 3.1M points and stays with the end-to-end tests.

Against the plain fp32 yardstick the all-fp32 backward missed 4 x in two places, both the sines': the spike regime (dp1 18.6 x,
db0 peak 25.6 x: one feature's argument carries 150 times its input's error) and dbc summed over the 384 to 768 images of the
wide regime (5.0 x to 7.0 x).  The second is the hardware cosine's systematic part, which adds coherently over all B * P points
against the upstream's mean of 0.5: measured at 768 x 600, dbc sits at 2.9e-6 with hardware sines, at 6.4e-7 with the polynomial
(TRIG_MODE 0), the per-image dpc being the same 6.7e-7 in both, and at 1.4 x the plain yardstick once the upstream's mean is removed.

Recorded on an MI355X, not bars: the largest product-to-yardstick ratio per form and regime, and where (dbs, dbf and
identically zero quantities left out; a sigma of fewer than 32 numbers is held to its peak bar alone).

  form                     regime                    rms x                                 peak x
  bwd staged trig 1        init                       0.41 dw1 1x1                          0.60 dw1 1x1
  bwd staged trig 1        init, sparse upstream      0.50 dwc 2x513 onehot-1-511           1.00 dw1 2x513 onehot-1-511
  bwd staged trig 1        scaled37                   0.18 dw1 2x513                        0.18 dw1 2x513
  bwd staged trig 1        scaled3e-4                 0.29 dw1 2x513                        0.40 dg1 2x513
  bwd staged trig 1        spike                      0.25 dws 2x513                        0.89 dws 2x513
  bwd staged trig 1        wc0                        1.00 dwf 2x513                        0.96 dwf 2x513
  bwd staged trig 1        wide                       0.67 dbc 768x600                      0.57 dbc 768x600
  bwd staged trig 1        wide, sparse upstream      0.38 dw1 2x513 dsigma                 0.43 dw0 2x1029 dsigma
  bwd staged_f32 trig 1    init                       2.93 dbc 384x2049                     2.79 dbc 384x2049
  bwd staged_f32 trig 1    init, sparse upstream      1.25 dw1 2x1029 dsigma                2.17 dwc 2x1029 dfeat
  bwd staged_f32 trig 1    scaled37                   0.74 dgc 2x513                        1.04 dw1 2x513
  bwd staged_f32 trig 1    scaled3e-4                 0.93 db1 2x513                        1.31 dw1 2x513
  bwd staged_f32 trig 1    spike                      1.22 dg1 2x513                        2.61 dws 2x513
  bwd staged_f32 trig 1    wc0                        1.12 dwc 2x513                        1.39 dwc 2x513
  bwd staged_f32 trig 1    wide                       3.90 dbc 384x2049                     3.40 dbc 384x2049
  bwd staged_f32 trig 1    wide, sparse upstream      1.69 dp1 2x1029 dsigma                2.57 dp0 2x1029 dsigma
  bwd x3 trig 0            init                       1.54 dgc 1x1                          2.03 dg0 1x31
  bwd x3 trig 0            init, sparse upstream      2.04 dgc 2x513 onehot-1-511           2.44 dgc 2x513 onehot-1-511
  bwd x3 trig 0            scaled37                   1.06 dw0 2x513                        1.12 dw0 2x513
  bwd x3 trig 0            scaled3e-4                 1.09 dp0 2x513                        1.09 dg0 2x513
  bwd x3 trig 0            spike                      1.45 dwf 2x513                        1.35 dw1 2x513
  bwd x3 trig 0            wc0                        1.15 dgc 2x513                        1.52 dgc 2x513
  bwd x3 trig 0            wide                       1.52 dg1 2x129 edge                   2.06 db0 2x129
  bwd x3 trig 0            wide, sparse upstream      1.90 dgc 2x1029 onehot-1-511          3.07 dgc 2x1029 onehot-1-511
  bwd x3 trig 1            init                       2.04 dgc 1x1                          2.49 dgc 1x1
  bwd x3 trig 1            init, sparse upstream      1.88 dgc 2x513 onehot-1-512           2.38 dgc 2x513 onehot-1-512
  bwd x3 trig 1            scaled37                   1.21 dg0 2x513                        1.30 dgc 2x513
  bwd x3 trig 1            scaled3e-4                 1.16 dbc 2x513                        1.36 dg1 2x513
  bwd x3 trig 1            spike                      1.95 dwf 2x513                        2.68 dws 2x513
  bwd x3 trig 1            wc0                        1.18 dw1 2x513                        1.65 dp0 2x513
  bwd x3 trig 1            wide                       1.74 dgc 1x1                          3.09 dgc 1x31
  bwd x3 trig 1            wide, sparse upstream      1.90 dgc 2x1029 onehot-1-511          3.07 dgc 2x1029 onehot-1-511
  fwd f32 trig 0           init                       1.18 sigma 2x129                      1.25 sigma 384x2049
  fwd f32 trig 0           scaled37                   1.09 feat 2x513                       1.05 feat 2x513
  fwd f32 trig 0           scaled3e-4                 1.11 sigma 2x513                      1.14 sigma 2x513
  fwd f32 trig 0           spike                      1.05 feat 2x513                       0.93 feat 2x513
  fwd f32 trig 0           wc0                        1.12 sigma 2x513                      0.99 sigma 2x513
  fwd f32 trig 0           wide                       1.39 sigma 2x129                      1.76 sigma 2x513
  fwd f32 trig 1           init                       1.58 feat 1x1                         1.33 sigma 2x129
  fwd f32 trig 1           scaled37                   1.11 feat 2x513                       1.08 sigma 2x513
  fwd f32 trig 1           scaled3e-4                 1.13 sigma 2x513                      0.99 feat 2x513
  fwd f32 trig 1           spike                      1.30 feat 2x513                       0.96 feat 2x513
  fwd f32 trig 1           wc0                        1.14 sigma 2x513                      1.16 sigma 2x513
  fwd f32 trig 1           wide                       1.37 sigma 2x129                      1.78 sigma 2x513
  fwd x3 trig 0            init                       1.19 feat 1x1                         1.19 sigma 384x1025
  fwd x3 trig 0            scaled37                   1.03 sigma 2x513                      0.93 feat 2x513
  fwd x3 trig 0            scaled3e-4                 1.06 sigma 2x513                      1.02 sigma 2x513
  fwd x3 trig 0            spike                      0.93 sigma 2x513                      0.62 sigma 2x513
  fwd x3 trig 0            wc0                        1.04 sigma 2x513                      1.01 sigma 2x513
  fwd x3 trig 0            wide                       1.38 sigma 2x129                      1.93 sigma 2x513
  fwd x3 trig 1            init                       1.71 sigma 1x1                        1.84 sigma 2x129 edge
  fwd x3 trig 1            scaled37                   1.36 sigma 2x513                      1.18 sigma 2x513
  fwd x3 trig 1            scaled3e-4                 1.43 sigma 2x513                      1.17 sigma 2x513
  fwd x3 trig 1            spike                      1.55 sigma 2x513                      1.13 sigma 2x513
  fwd x3 trig 1            wc0                        1.45 sigma 2x513                      1.30 sigma 2x513
  fwd x3 trig 1            wide                       2.68 sigma 1x1                        1.96 feat 2x129
  fwd x3 trig 3            init                       1.59 sigma 1x1                        1.71 sigma 2x1029 edge
  fwd x3 trig 3            scaled37                   1.19 feat 2x513                       1.30 sigma 2x513
  fwd x3 trig 3            scaled3e-4                 1.12 feat 2x513                       1.13 feat 2x513
  fwd x3 trig 3            spike                      1.19 sigma 2x513                      1.39 sigma 2x513
  fwd x3 trig 3            wc0                        1.30 sigma 2x513                      1.13 sigma 2x513
  fwd x3 trig 3            wide                       1.44 sigma 2x1029 edge                1.69 sigma 2x1029 edge
"""
import functools
import statistics

import pytest
import torch

import siren_refs as sr

pytestmark = pytest.mark.gpu

SEED = 3
SMALL = [(1, 1), (1, 31), (2, 129), (3, 512), (2, 513), (2, 1029)]
LONG = {(384, 1025): 1024, (384, 2049): 2048, (768, 600): 4096}       # (B, P): the chunk x3_chunk picks
PATTERN_SHAPES = [(2, 513), (2, 1029)]
FWD_MODES = [("f32", 0), ("f32", 1), ("x3", 0), ("x3", 1), ("x3", 3)]
BWD_MODES = [("x3", 0), ("x3", 1), ("staged", 1), ("staged_f32", 1)]


def _cases():
    """(regime, points, B, P): every regime at (2, 513); init and wide at every shape; edge points at (2, 129) and (2, 1029)"""
    c = [(r, "box", 2, 513) for r in sr.REGIMES]
    c += [(r, "box", B, P) for B, P in SMALL + list(LONG) if (B, P) != (2, 513) for r in ("init", "wide")]
    c += [(r, "edge", B, P) for B, P in [(2, 129), (2, 1029)] for r in ("init", "wide")]
    return c


def _patterns(P):
    """one part of the upstream alone; one live row: the last point of the ragged tail, point 511, point 512 of image 1"""
    return ["dsigma", "dfeat"] + [("onehot", 1, p) for p in sorted({P - 1, 511, 512})]


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# known misses, strict: (test, mode, trig, regime, points, B, P) -> {quantity: reason with the measured ratio}.  Every other
# quantity of the case is asserted; a listed one that comes inside its bar fails the test, so a fix shows.
EXPECTED = {}


def _params(test, modes, cases):
    out = []
    for case in cases:
        for mode in modes:
            out.append(pytest.param(*mode, *case, id="-".join(_id(v) for v in mode + case)))
    return out


@functools.lru_cache(maxsize=None)
def _case(regime, kind, B, P, pattern):
    """inputs on the device, the fp64 truth, and the two yardsticks' distances from it — computed once per case and left alone"""
    dev = torch.device("cuda")
    t, pts = sr.make_tensors(regime, B, SEED), sr.make_points(kind, B, P, SEED)
    up = sr.make_upstream(B, P, SEED, pattern)
    where, images = ("cuda", 64) if B * P >= 400_000 else ("cpu", None)
    truth = sr.evaluate(pts, t, up, torch.float64, None, where, images)
    kinds = {"f32": None, "bf16x2": "bf16x2"}
    yard = {k: sr.all_distances(sr.evaluate(pts, t, up, torch.float32, pl, where, images), truth) for k, pl in kinds.items()}
    yard["f32 coarse sines"] = sr.all_distances(sr.evaluate(pts, t, up, torch.float32, None, where, images, sr.SINE_ERROR), truth)
    value_rms = {}
    if P < 512:
        # feat and sigma are per-point quantities: on a handful of points the yardstick's distance is one draw of its error, not
        # its size, and the values' own rms is no scale (a single sigma: two realisations of the yardstick 4.9 x apart,
        # tests/test_siren_refs_cpu.py).  Both are taken over 512 points: the case's own, then more of the kind
        more = torch.cat([pts, sr.make_points(kind, B, 512 - P, SEED + 1)], 1)
        t512 = sr.evaluate(more, t, None, torch.float64)
        for k, pl in kinds.items():
            yard[k].update(sr.all_distances(sr.evaluate(more, t, None, torch.float32, pl), t512))
        value_rms = {q: float(v.pow(2).mean().sqrt()) for q, v in t512.items()}
    return dict(t=[v.to(dev) for v in t], pts=pts.to(dev), up=up.to(dev), truth=truth, yard=yard, value_rms=value_rms)


def _run(ops, monkeypatch, c, fwd, bwd, trig, backward):
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", fwd)
    monkeypatch.setattr(ops, "SIREN_BWD_MODE", bwd)
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    leaves = [v.clone().requires_grad_(backward) for v in c["t"]]
    feat, sigma = ops.SirenFunction.apply(c["pts"], *leaves)
    res = {"feat": feat.detach(), "sigma": sigma.detach()}
    if backward:
        torch.autograd.backward([feat, sigma], [c["up"][..., :32].contiguous(), c["up"][..., 32].contiguous()])
        res.update({"d" + n: v.grad for n, v in zip(sr.NAMES, leaves)})
    torch.cuda.synchronize()
    return res


def _check(tag, res, c, quantities, yardstick, bars, expected=None):
    """every quantity against its bars(q, yardstick distances) -> (rms bar, peak bar); prints each figure, then asserts all.
    expected: {quantity: reason} of EXPECTED — those have to miss, and the test then ends as an expected failure"""
    expected = expected or {}
    bad, missed = [], set()
    for q in quantities:
        n_bad = len(bad)
        truth = c["truth"][q]
        got = res[q].to(truth.device)
        zero = (truth == 0).all(-1) if q[1:] in sr.FILM else (truth == 0).all()
        if bool(zero.any()) and bool((got[zero] != 0).any() if zero.dim() else (got != 0).any()):
            bad.append(f"{q}: not exactly zero where the fp64 value is")
        d = sr.distances(got, truth, per_image=q[1:] in sr.FILM, value_rms=c["value_rms"].get(q))
        y = c["yard"][yardstick][q]
        b_rms, b_peak = bars(q, y)
        if truth.numel() < 32 and q in ("feat", "sigma"):
            b_rms = float("inf")        # the rms of a few sigmas is their peak: held to the peak bar alone
        print(f"RATIO {tag} {q} rms {d['rms']:.3e} yard {y['rms']:.3e} x{d['rms'] / max(y['rms'], 1e-300):.2f} bar {b_rms:.3e} | "
              f"peak {d['peak']:.3e} yard {y['peak']:.3e} x{d['peak'] / max(y['peak'], 1e-300):.2f} bar {b_peak:.3e}")
        if not d["rms"] <= b_rms:
            bad.append(f"{q}: rms {d['rms']:.3e} > {b_rms:.3e} ({d['rms'] / max(y['rms'], 1e-300):.2f} x the {yardstick} yardstick)")
        if not d["peak"] <= b_peak:
            bad.append(f"{q}: peak {d['peak']:.3e} > {b_peak:.3e} ({d['peak'] / max(y['peak'], 1e-300):.2f} x the {yardstick} yardstick)")
        if q in expected and len(bad) > n_bad:
            missed.add(q)
            del bad[n_bad:]
    bad += [f"{q}: expected to miss its bar ({expected[q]}) and did not" for q in expected if q not in missed]
    assert not bad, tag + "\n  " + "\n  ".join(bad)
    if missed:
        pytest.xfail("; ".join(f"{q}: {expected[q]}" for q in sorted(missed)))


def _fwd_bars(q, y):
    return 2 * y["rms"] + 2e-7, sr.M_FWD_PEAK * y["peak"] + 2e-6


def _grad_bars(mode, regime, rows, pattern="dense"):
    m_rms, m_peak = (4, 4) if mode == "staged_f32" else sr.grad_multipliers(regime, pattern, rows)

    def bars(q, y):
        floor = 1e-6 if q in sr.NO_PRODUCT else 0.0
        return m_rms * y["rms"] + floor, m_peak * y["peak"] + floor
    return bars


GRADS = sr.QUANTITIES[2:]


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """the cases' device tensors (the fp64 truths of the 400k-point cases among them) go when the module is done"""
    yield
    _case.cache_clear()
    torch.cuda.empty_cache()


def _assert_chunk(B, P):
    """the case walks the chunk it is there for (x3_chunk, siren_x3_common.h)"""
    from cips3d_amd import _lib
    chunk = LONG.get((B, P), 512)
    assert _lib.load().cips_siren_bwd_x3_chunks(B, P) == -(-P // chunk)
    assert chunk == 4096 or B * -(-P // (2 * chunk)) < 768          # the next larger chunk was not eligible
    assert chunk == 512 or B * -(-P // chunk) >= 768


@pytest.mark.parametrize("fwd,trig,regime,kind,B,P", _params("forward", FWD_MODES, _cases()))
def test_siren_forward_fp64(fwd, trig, regime, kind, B, P, monkeypatch):
    from cips3d_amd import ops
    _assert_chunk(B, P)
    c = _case(regime, kind, B, P, "dense")
    res = _run(ops, monkeypatch, c, fwd, "x3", trig, backward=False)
    yardstick = "bf16x2" if (fwd == "x3" and trig & 2) else "f32"
    _check(f"fwd {fwd} trig{trig} {regime} {kind} {B}x{P}", res, c, ("feat", "sigma"), yardstick, _fwd_bars)


@pytest.mark.parametrize("bwd,trig,regime,kind,B,P", _params("backward", BWD_MODES, _cases()))
def test_siren_backward_fp64(bwd, trig, regime, kind, B, P, monkeypatch):
    from cips3d_amd import ops
    _assert_chunk(B, P)
    c = _case(regime, kind, B, P, "dense")
    res = _run(ops, monkeypatch, c, "x3", bwd, trig, backward=True)
    yardstick = "f32 coarse sines" if bwd == "staged_f32" else "bf16x2"
    _check(f"bwd {bwd} trig{trig} {regime} {kind} {B}x{P} dense", res, c, GRADS, yardstick, _grad_bars(bwd, regime, B * P),
           EXPECTED.get(("backward", bwd, trig, regime, kind, B, P)))


@pytest.mark.parametrize("bwd,trig,regime,kind,B,P,pattern", _params(
    "pattern", BWD_MODES, [(r, "box", B, P, pat) for B, P in PATTERN_SHAPES for r in ("init", "wide") for pat in _patterns(P)]))
def test_siren_backward_fp64_upstream_patterns(bwd, trig, regime, kind, B, P, pattern, monkeypatch):
    """one part of the upstream zero, or one live row: a tail row read twice, a chunk's last point lost or a sum taken over the
    wrong image moves these by far more than a bar"""
    from cips3d_amd import ops
    c = _case(regime, kind, B, P, pattern)
    res = _run(ops, monkeypatch, c, "x3", bwd, trig, backward=True)
    yardstick = "f32 coarse sines" if bwd == "staged_f32" else "bf16x2"
    _check(f"bwd {bwd} trig{trig} {regime} {kind} {B}x{P} {_id(pattern)}", res, c, GRADS, yardstick, _grad_bars(bwd, regime, B * P, pattern))


@pytest.mark.parametrize("trig", [0, 1])
@pytest.mark.parametrize("B,P", [(2, 513), (3, 512)])
def test_siren_backward_x3_runs_on_split_bf16(trig, B, P, monkeypatch):
    """mode in effect: the fused backward's gradients sit at the "bf16x2" yardstick's distance, not several times below it
    where an fp32 leg wired in by mistake would (the plain fp32 yardstick is 5 to 10 times closer to fp64)"""
    from cips3d_amd import ops
    c = _case("init", "box", B, P, "dense")
    res = _run(ops, monkeypatch, c, "x3", "x3", trig, backward=True)
    qs = [q for q in GRADS if q not in sr.NO_PRODUCT]
    got = statistics.median(sr.distances(res[q].cpu(), c["truth"][q], per_image=q[1:] in sr.FILM)["rms"] for q in qs)
    yard = statistics.median(c["yard"]["bf16x2"][q]["rms"] for q in qs)
    print(f"median gradient rms: fused backward {got:.3e}, bf16x2 yardstick {yard:.3e}, "
          f"fp32 yardstick {statistics.median(c['yard']['f32'][q]['rms'] for q in qs):.3e}")
    assert got >= 0.25 * yard
