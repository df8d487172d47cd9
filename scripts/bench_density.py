"""Density-volume microbench: sigma on an N^3 lattice (GeneratorNerfINR.density_grid's kernel) three ways, device-event timings,
legs alternated inside every repeat of one process:

  (a) cips_siren_sigma_x3_grid   the lattice's three coordinate arrays in, 4 B per point out
  (b) cips_siren_sigma_x3        the same points materialised as a (B, P, 3) tensor: 12 B in, 4 B out
  (c) cips_siren_fwd_x3          the full forward on those points in chunks that fit memory (what there was before the
                                 sigma-only kernel): 12 B in, 132 B out, sigma picked from its output

--alt NAME=PATH (repeatable) names another build of the library; its (a) runs next to the product's as leg (a'), (a''), ...
The occupancy A/B of profiles/density_grid.txt was made this way: its partner was the library built into another build.LIBDIR
from siren_sigma_x3_kernel with __launch_bounds__(512, 2) and 96 KiB asked for at the launch (one workgroup resident per CU).
Real initialiser weights (bench.G_CFG under seed 0), random styles.  The table goes to stdout and to --out."""
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
from cips3d_amd.generator import GeneratorNerfINR

FLOP_PER_POINT = 2 * (128 * 3 + 128 * 128 + 128)      # 33 792: layer 0, W1, the sigma dot
ROOF_3PASS = 2516.8e12 / 3                            # dense bf16 / fp16 MFMA peak over the three passes of a split product
BYTES = {"a": 4, "b": 16, "c": 144}                   # HBM bytes per point, algorithmic (every (a') is an (a))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--chunk", type=int, default=1 << 21, help="points per image and call of leg (c)")
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("at least 5 timed repeats per leg")
    d = torch.device("cuda:0")
    lib = _lib.load()
    alts = []                                            # (leg, name, library)
    for i, spec in enumerate(a.alt):
        name, path = spec.rsplit("=", 1)
        alt = C.CDLL(os.path.abspath(path))
        alt.cips_siren_sigma_x3_grid.restype, alt.cips_siren_sigma_x3_grid.argtypes = _lib.SIGNATURES["cips_siren_sigma_x3_grid"]
        alts.append(("a" + "'" * (i + 1), name, alt))
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=d).to(d)
    G.device = d
    N = a.n
    P = N ** 3
    gx, gy, gz = (g.to(d) for g in density_lattice(N, 0.3, (0., 0., 0.)))
    lines = [f"density lattice N={N} ({P} points per image), {a.repeats} timed repeats per leg after 2 warm-up rounds, legs alternated",
             f"roof: {FLOP_PER_POINT} useful FLOP per point on 3-pass split MFMAs = {ROOF_3PASS / FLOP_PER_POINT / 1e9:.2f} Gpoint/s",
             "leg   B   ms(median)  ms(min)  ms(max)  Gpoint/s  of_3pass_roof  HBM_B/point  TB/s"]
    ok = True
    for B in (int(v) for v in a.batches.split(",")):
        with torch.no_grad():
            style = {k: torch.randn(B, 128, device=d) for k in G.siren.style_dim_dict}
            t = ops._siren_prep(G.siren._siren_args(style))
        sw = ops._siren_struct(t)
        gp = GridParams(ops._p(gx), ops._p(gy), ops._p(gz), N, N, N)
        pts = torch.stack([gx.view(N, 1, 1).expand(N, N, N), gy.view(1, N, 1).expand(N, N, N), gz.view(1, 1, N).expand(N, N, N)],
                          -1).reshape(1, P, 3).expand(B, P, 3).contiguous()
        chunks = [pts[:, p0:p0 + a.chunk].contiguous() for p0 in range(0, P, a.chunk)]     # leg (c)'s inputs, made outside its timing
        cmax = max(c.shape[1] for c in chunks)
        feat = torch.empty(B, cmax, 32, device=d)
        sig_c = torch.empty(B, cmax, device=d)
        vol = {k: torch.empty(B, P, device=d) for k in ["a", "b"] + [k for k, _, _ in alts]}
        st = ops._stream

        def leg_a():
            _lib.check(lib.cips_siren_sigma_x3_grid(C.byref(sw), C.byref(gp), ops._p(vol["a"]), B, st()), "sigma_x3_grid")

        def leg_alt(k, alt):
            return lambda: _lib.check(alt.cips_siren_sigma_x3_grid(C.byref(sw), C.byref(gp), ops._p(vol[k]), B, st()), "sigma_x3_grid " + k)

        def leg_b():
            _lib.check(lib.cips_siren_sigma_x3(C.byref(sw), ops._p(pts), ops._p(vol["b"]), B, P, st()), "sigma_x3")

        def leg_c():
            for c in chunks:
                _lib.check(lib.cips_siren_fwd_x3(C.byref(sw), ops._p(c), ops._p(feat), ops._p(sig_c), B, c.shape[1], st()), "fwd_x3")

        legs = [("a", leg_a)] + [(k, leg_alt(k, alt)) for k, _, alt in alts] + [("b", leg_b), ("c", leg_c)]
        times = {k: [] for k, _ in legs}
        for rep in range(a.repeats + 2):
            for k, fn in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 2:
                    times[k].append(e0.elapsed_time(e1))
        # the timed outputs are the same volume: (a), (a') and (b) bit for bit, and (c)'s last chunk too
        assert all(torch.equal(vol["a"], v) for v in vol.values())
        p0 = (len(chunks) - 1) * a.chunk
        assert torch.equal(sig_c[:, :P - p0], vol["a"][:, p0:])
        for k, _ in legs:
            ts = sorted(times[k])
            med = ts[len(ts) // 2]
            rate = B * P / (med * 1e-3)
            lines.append(f"({k + ')':<4} {B:<3} {med:10.3f}  {ts[0]:7.3f}  {ts[-1]:7.3f}  {rate / 1e9:8.3f}  {rate * FLOP_PER_POINT / ROOF_3PASS:13.3f}"
                         f"  {BYTES[k[0]]:11d}  {rate * BYTES[k[0]] / 1e12:.3f}")
        ta, tc = sorted(times["a"]), sorted(times["c"])
        gain, spread = tc[len(tc) // 2] - ta[len(ta) // 2], tc[-1] - tc[0]
        verdict = gain > spread
        ok = ok and verdict
        lines.append(f"     B={B}: (c) - (a) = {gain:.3f} ms (medians), min-max spread of (c) = {spread:.3f} ms -> "
                     f"{'(a) is faster by more than the spread' if verdict else '(a) is NOT faster by more than the spread'}; "
                     f"speed-up {tc[len(tc) // 2] / ta[len(ta) // 2]:.2f}x")
        del pts, chunks, feat, sig_c, vol
        torch.cuda.empty_cache()
    for k, name, _ in alts:
        lines.append(f"({k}) = (a) from another build of the library: {name}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not ok:
        raise SystemExit(2)


if __name__ == "__main__":
    main()
