"""Point-colour microbench: the colour of the SIREN's radiance field on an N^3 lattice (GeneratorNerfINR.color_grid's kernel) and
at a mesh-sized set of points (extract_mesh(colors='aux')), against the path composed of what existed before the colour kernel,
device-event timings, legs alternated inside every repeat of one process:

  lattice, N^3 points per image
  (a) cips_siren_rgb_x3_grid     the three coordinate arrays in, 12 B per point out (rgb only)
  (a+) the same with sigma       16 B per point out
  (b) composed                   the points materialised as (B, P, 3) (outside the timing), then per chunk that fits memory:
                                 cips_siren_fwd_x3 (12 B in, 132 B out), _ToRGBFunction (128 B in, 12 B out), torch.tanh
                                 (12 B in, 12 B out) — three launches per chunk
  (s) cips_siren_sigma_x3_grid   the sigma-only lattice kernel, for scale: 16 896 of the 27 136 MAC per point, 4 B out
  points, P per image
  (p) cips_siren_rgb_x3          12 B in, 12 B out
  (q) composed                   cips_siren_fwd_x3 + _ToRGBFunction + torch.tanh on the same points, one chunk

The outputs of (a) and (p) are compared with (b) and (q) where they are timed: the composed path rounds the 32-term sum in
another order, so the comparison is a bar on the absolute difference, not bits.  Real initialiser weights (bench.G_CFG under seed
0), random styles.  The table goes to stdout and to --out."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import G_CFG
from cips3d_amd import _lib, ops
from cips3d_amd._lib import GridParams
from cips3d_amd.evaluation import density_lattice
from cips3d_amd.generator import GeneratorNerfINR, _ToRGBFunction

MAC_COLOR = 128 * 3 + 128 * 128 + 128 + 64 * 128 + 32 * 64 + 3 * 32       # the chain's 27 136 and the projection's 96
MAC_SIGMA = 128 * 3 + 128 * 128 + 128
ROOF_3PASS = 2516.8e12 / 3                            # dense bf16 / fp16 MFMA peak over the three passes of a split product
BYTES = {"a": 12, "a+": 16, "b": 12 + 132 + 128 + 12 + 12 + 12, "s": 4, "p": 24, "q": 12 + 132 + 128 + 12 + 12 + 12}
MAC = {"a": MAC_COLOR, "a+": MAC_COLOR, "b": MAC_COLOR, "s": MAC_SIGMA, "p": MAC_COLOR, "q": MAC_COLOR}
BAR = 1e-5            # |rgb difference| of two fp32 evaluations of tanh(W f + b), |W f + b| of order 1: a few 1e-7 expected


def timed(legs, repeats):
    times = {k: [] for k, _ in legs}
    for rep in range(repeats + 2):                      # two warm-up rounds of every leg, then the timed ones, alternated
        for k, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[k].append(e0.elapsed_time(e1))
    return {k: sorted(v) for k, v in times.items()}


def rows(times, B, P):
    out = []
    for k, ts in times.items():
        med = ts[len(ts) // 2]
        rate = B * P / (med * 1e-3)
        out.append(f"({k + ')':<4} {B:<3} {P:<9} {med:10.3f}  {ts[0]:8.3f}  {ts[-1]:8.3f}  {rate / 1e9:8.3f}  "
                   f"{rate * 2 * MAC[k] / ROOF_3PASS:13.3f}  {BYTES[k]:11d}  {rate * BYTES[k] / 1e12:.3f}")
    return out


def verdict(times, new, old, what):
    tn, to = times[new], times[old]
    gain, spread = to[len(to) // 2] - tn[len(tn) // 2], max(to[-1] - to[0], tn[-1] - tn[0])
    word = "faster by more than the spread" if gain > spread else ("NOT faster by more than the spread" if gain >= 0 else "SLOWER")
    return (f"     {what}: ({old}) - ({new}) = {gain:.3f} ms (medians), largest min-max spread of the two = {spread:.3f} ms -> "
            f"({new}) is {word}; ratio {to[len(to) // 2] / tn[len(tn) // 2]:.2f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--points", type=int, default=300000, help="P of the points legs: the vertices of a 256^3 mesh")
    ap.add_argument("--batches", default="1,2")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="points per image and call of leg (b)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("at least 5 timed repeats per leg")
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_colors needs the GPU: there is nothing to time without one")
    d = torch.device("cuda:0")
    lib = _lib.load()
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=d).to(d)
    G.device = d
    W, bias = G.aux_to_rbg[0].weight.detach().contiguous(), G.aux_to_rbg[0].bias.detach().contiguous()
    N, Pm = a.n, a.points
    P = N ** 3
    gx, gy, gz = (g.to(d) for g in density_lattice(N, 0.3, (0., 0., 0.)))
    lines = [f"point colours: lattice N={N} ({P} points per image) and P={Pm} points per image, {a.repeats} timed repeats per leg "
             f"after 2 warm-up rounds, legs alternated",
             f"roof: {2 * MAC_COLOR} useful FLOP per point on 3-pass split MFMAs = {ROOF_3PASS / (2 * MAC_COLOR) / 1e9:.2f} Gpoint/s "
             f"(sigma only: {ROOF_3PASS / (2 * MAC_SIGMA) / 1e9:.2f})",
             "leg   B   P         ms(median)   ms(min)   ms(max)  Gpoint/s  of_3pass_roof  HBM_B/point  TB/s"]
    st = ops._stream
    for B in (int(v) for v in a.batches.split(",")):
        with torch.no_grad():
            style = {k: torch.randn(B, 128, device=d) for k in G.siren.style_dim_dict}
            t = ops._siren_prep(G.siren._siren_args(style))
        sw = ops._siren_struct(t)
        gp = GridParams(ops._p(gx), ops._p(gy), ops._p(gz), N, N, N)
        pts = ops.lattice_points(gx, gy, gz, B).contiguous()
        chunks = [pts[:, p0:p0 + a.chunk].contiguous() for p0 in range(0, P, a.chunk)]     # leg (b)'s inputs, made outside its timing
        del pts
        cmax = max(c.shape[1] for c in chunks)
        feat, sig_c = torch.empty(B, cmax, 32, device=d), torch.empty(B, cmax, device=d)
        rgb_a, rgb_ap, rgb_b = (torch.empty(B, P, 3, device=d) for _ in range(3))
        sig_ap, sig_s = torch.empty(B, P, device=d), torch.empty(B, P, device=d)

        def leg_a():
            _lib.check(lib.cips_siren_rgb_x3_grid(C.byref(sw), C.byref(gp), ops._p(W), ops._p(bias), 1, ops._p(rgb_a), None, B, st()),
                       "rgb_x3_grid")

        def leg_ap():
            _lib.check(lib.cips_siren_rgb_x3_grid(C.byref(sw), C.byref(gp), ops._p(W), ops._p(bias), 1, ops._p(rgb_ap), ops._p(sig_ap),
                                                  B, st()), "rgb_x3_grid")

        def leg_b():
            with torch.no_grad():
                p0 = 0
                for c in chunks:
                    n = c.shape[1]
                    f = feat.view(-1)[:B * n * 32].view(B, n, 32)
                    _lib.check(lib.cips_siren_fwd_x3(C.byref(sw), ops._p(c), ops._p(f), ops._p(sig_c), B, n, st()), "fwd_x3")
                    torch.tanh(_ToRGBFunction.apply(f, W, bias), out=rgb_b[:, p0:p0 + n])
                    p0 += n

        def leg_s():
            _lib.check(lib.cips_siren_sigma_x3_grid(C.byref(sw), C.byref(gp), ops._p(sig_s), B, st()), "sigma_x3_grid")

        times = timed([("a", leg_a), ("a+", leg_ap), ("b", leg_b), ("s", leg_s)], a.repeats)
        assert torch.equal(rgb_a, rgb_ap) and torch.equal(sig_ap, sig_s)
        diff = float((rgb_a - rgb_b).abs().max())
        assert diff <= BAR, diff
        lines += rows(times, B, P)
        lines.append(verdict(times, "a", "b", f"lattice B={B}") + f"; max |rgb (a) - rgb (b)| = {diff:.1e}")
        del chunks, feat, sig_c, rgb_a, rgb_ap, rgb_b, sig_ap, sig_s
        torch.cuda.empty_cache()

        ptm = ((torch.rand(B, Pm, 3, device=d) - 0.5) * 0.3).contiguous()
        feat, sig_c = torch.empty(B, Pm, 32, device=d), torch.empty(B, Pm, device=d)
        rgb_p = torch.empty(B, Pm, 3, device=d)
        res = {}

        def leg_p():
            _lib.check(lib.cips_siren_rgb_x3(C.byref(sw), ops._p(ptm), ops._p(W), ops._p(bias), 1, ops._p(rgb_p), None, B, Pm, st()),
                       "rgb_x3")

        def leg_q():
            with torch.no_grad():
                _lib.check(lib.cips_siren_fwd_x3(C.byref(sw), ops._p(ptm), ops._p(feat), ops._p(sig_c), B, Pm, st()), "fwd_x3")
                res["q"] = torch.tanh(_ToRGBFunction.apply(feat, W, bias))

        times = timed([("p", leg_p), ("q", leg_q)], a.repeats)
        diff = float((rgb_p - res["q"]).abs().max())
        assert diff <= BAR, diff
        lines += rows(times, B, Pm)
        lines.append(verdict(times, "p", "q", f"points B={B}") + f"; max |rgb (p) - rgb (q)| = {diff:.1e}")
        del ptm, feat, sig_c, rgb_p, res
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
