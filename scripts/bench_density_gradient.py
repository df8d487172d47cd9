"""Density-gradient microbench: sigma and grad sigma on an N^3 lattice (GeneratorNerfINR.density_grid(return_gradient=True)'s
kernel) against its floor and against what there was before it; device-event timings, legs alternated inside every repeat of
one process:

  (a) cips_siren_sigma_grad_x3_grid   the lattice's three coordinate arrays in, sigma + gradient out (16 B per point)
  (b) cips_siren_sigma_x3_grid        sigma alone: the same chain without the transposed layer — the floor
  (c) cips_siren_sigma_x3 six times   central differences on points shifted by +-h along each axis, the six (B, P, 3) tensors
                                      built outside the timing and the differences not taken: less than a user has to do

--alt NAME=PATH (repeatable) names another build of the library; its (a) runs next to the product's as leg (a'), (a''), ...
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

MAC_SIGMA = 128 * 3 + 128 * 128 + 128                 # 16 896: layer 0, W1, the sigma dot
MAC_GRAD = 128 * 128                                  # 16 384: the transposed layer (the layer-0 sums ride on the VALU)
BYTES = {"a": 16, "b": 4, "c": 6 * 16}                # HBM bytes per point, algorithmic


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--h", type=float, default=1e-4, help="step of leg (c)'s central differences")
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
        alt.cips_siren_sigma_grad_x3_grid.restype, alt.cips_siren_sigma_grad_x3_grid.argtypes = _lib.SIGNATURES["cips_siren_sigma_grad_x3_grid"]
        alts.append(("a" + "'" * (i + 1), name, alt))
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=d).to(d)
    G.device = d
    N = a.n
    P = N ** 3
    gx, gy, gz = (g.to(d) for g in density_lattice(N, 0.3, (0., 0., 0.)))
    lines = [f"density-gradient lattice N={N} ({P} points per image), {a.repeats} timed repeats per leg after 2 warm-up rounds, legs alternated",
             f"MAC per point: (a) {MAC_SIGMA + MAC_GRAD}, (b) {MAC_SIGMA}, (c) {6 * MAC_SIGMA}; trigonometric evaluations: 512, 256, 1536",
             "leg   B   ms(median)  ms(min)  ms(max)  Gpoint/s  HBM_B/point  TB/s"]
    ok = True
    for B in (int(v) for v in a.batches.split(",")):
        with torch.no_grad():
            style = {k: torch.randn(B, 128, device=d) for k in G.siren.style_dim_dict}
            t = ops._siren_prep(G.siren._siren_args(style))
        sw = ops._siren_struct(t)
        gp = GridParams(ops._p(gx), ops._p(gy), ops._p(gz), N, N, N)
        pts = torch.stack([gx.view(N, 1, 1).expand(N, N, N), gy.view(1, N, 1).expand(N, N, N), gz.view(1, 1, N).expand(N, N, N)],
                          -1).reshape(1, P, 3).expand(B, P, 3)
        shifted = []
        for ax in range(3):
            for sgn in (1.0, -1.0):
                e = torch.zeros(3, device=d)
                e[ax] = sgn * a.h
                shifted.append((pts + e).contiguous())
        sig_fd = [torch.empty(B, P, device=d) for _ in shifted]
        sig = {k: torch.empty(B, P, device=d) for k in ["a", "b"] + [k for k, _, _ in alts]}
        grad = {k: torch.empty(B, P, 3, device=d) for k in ["a"] + [k for k, _, _ in alts]}
        st = ops._stream

        def leg_a():
            _lib.check(lib.cips_siren_sigma_grad_x3_grid(C.byref(sw), C.byref(gp), ops._p(sig["a"]), ops._p(grad["a"]), B, st()), "sigma_grad_x3_grid")

        def leg_alt(k, alt):
            return lambda: _lib.check(alt.cips_siren_sigma_grad_x3_grid(C.byref(sw), C.byref(gp), ops._p(sig[k]), ops._p(grad[k]), B, st()),
                                      "sigma_grad_x3_grid " + k)

        def leg_b():
            _lib.check(lib.cips_siren_sigma_x3_grid(C.byref(sw), C.byref(gp), ops._p(sig["b"]), B, st()), "sigma_x3_grid")

        def leg_c():
            for p_, o_ in zip(shifted, sig_fd):
                _lib.check(lib.cips_siren_sigma_x3(C.byref(sw), ops._p(p_), ops._p(o_), B, P, st()), "sigma_x3")

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
        # the timed outputs describe the same volume: sigma bit for bit, and the gradient agrees with leg (c)'s differences
        assert all(torch.equal(sig["a"], v) for v in sig.values()) and all(torch.equal(grad["a"], v) for v in grad.values())
        fd = torch.stack([(sig_fd[2 * ax] - sig_fd[2 * ax + 1]) / (2 * a.h) for ax in range(3)], -1)
        dev_fd = float((fd - grad["a"]).abs().max() / grad["a"].abs().max())
        for k, _ in legs:
            ts = sorted(times[k])
            med = ts[len(ts) // 2]
            rate = B * P / (med * 1e-3)
            lines.append(f"({k + ')':<4} {B:<3} {med:10.3f}  {ts[0]:7.3f}  {ts[-1]:7.3f}  {rate / 1e9:8.3f}  {BYTES[k[0]]:11d}  {rate * BYTES[k[0]] / 1e12:.3f}")
        ta, tb, tc = sorted(times["a"]), sorted(times["b"]), sorted(times["c"])
        ma, mb, mc = ta[len(ta) // 2], tb[len(tb) // 2], tc[len(tc) // 2]
        gain, spread = mc - ma, tc[-1] - tc[0]
        verdict = gain > spread
        ok = ok and verdict
        lines.append(f"     B={B}: (a) / (b) = {ma / mb:.2f}; (c) - (a) = {gain:.3f} ms (medians), min-max spread of (c) = {spread:.3f} ms -> "
                     f"{'(a) is faster by more than the spread' if verdict else '(a) is NOT faster by more than the spread'}; "
                     f"speed-up {mc / ma:.2f}x; fp32 central differences at h = {a.h:g} are {dev_fd:.1e} of max |grad| away from (a)")
        del pts, shifted, sig_fd, sig, grad, fd
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
