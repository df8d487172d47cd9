"""Surface ray-cast microbench: first-hit depth of the iso-surface sigma = level for every pixel of an img x img view
(GeneratorNerfINR.surface's kernel) against the same search composed from the sigma kernel and against the sigma kernel's own
rate; device-event timings, legs alternated inside every repeat of one process:

  (a) cips_siren_surface_x3          one launch: coarse walk with early exit, bisection, secant, final evaluation
  (b) ops.siren_surface_composed     cips_rays_fwd + one cips_siren_sigma_x3 launch over all (ray, sample) points + torch tensor
                                     operations + one launch per bisection step + one for the final point
  (c) cips_siren_sigma_x3            on n * (S + refine + 1) random points: the evaluations (a) makes at most, with no search

The level is the 0.7 quantile of the densities at the coarse samples, so the view has misses, hits and rays that start inside.
Real initialiser weights (bench.G_CFG under seed 0), random styles, a seeded gaussian camera per image.  The table goes to stdout
and to --out."""
import argparse
import ctypes as C
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bench import G_CFG
from cips3d_amd import _lib, ops
from cips3d_amd.generator import GeneratorNerfINR


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--refine", type=int, default=8)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("at least 5 timed repeats per leg")
    d = torch.device("cuda:0")
    lib = _lib.load()
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=d).to(d)
    G.device = d
    img, S, refine = a.img, a.steps, a.refine
    n = img * img
    fov, t0, t1 = 12, 0.88, 1.12
    zc = float((-torch.ones(1) / np.tan((2 * math.pi * fov / 360) / 2)).item())
    xg, yg, zg = ops.pixel_grids(img, img, S, t0, t1, d)
    lines = [f"surface ray cast {img} x {img}, S = {S} coarse steps, refine = {refine} ({n} rays per image, at most {S + refine + 1} "
             f"evaluations per ray), {a.repeats} timed repeats per leg after 2 warm-up rounds, legs alternated",
             "leg   B   ms(median)  ms(min)  ms(max)  Mray/s   Geval/s (evaluations made or, for (c), points)"]
    for B in (int(v) for v in a.batches.split(",")):
        with torch.no_grad():
            style = {k: torch.randn(B, 128, device=d) for k in G.siren.style_dim_dict}
            args = G.siren._siren_args(style)
            t = ops._siren_prep(args)
        _, _, c2w = ops.camera_pose(torch.randn(B, 1, device=d), torch.randn(B, 1, device=d), False, 0.3, math.pi / 2, 0.155, math.pi / 2)
        geom = (B, img, img, S, zc)
        # the level: from the coarse samples of these rays
        dirs = ops.rays_fwd(xg, yg, zg, zc, c2w, None, B, img, img, S)[2]
        pts = (c2w[:, None, None, :3, 3] + dirs.unsqueeze(2) * zg.view(1, 1, S, 1)).reshape(B, n * S, 3).contiguous()
        coarse = ops.siren_sigma(pts, *args)
        level = float(np.float32(torch.quantile(coarse.flatten()[:: max(1, coarse.numel() // (1 << 22))], 0.7).item()))
        del pts, coarse
        sw = ops._siren_struct(t)
        rp = ops._ray_params(xg, yg, zg, zc, c2w, None, img, img, S)
        depth = torch.empty(B, n, device=d)
        hit = torch.empty(B, n, dtype=torch.uint8, device=d)
        sigma = torch.empty(B, n, device=d)
        points = torch.empty(B, n, 3, device=d)
        P = n * (S + refine + 1)
        rnd = ((torch.rand(B, P, 3, device=d) - 0.5) * 0.24).contiguous()
        sig_c = torch.empty(B, P, device=d)
        res = {}

        def leg_a():
            _lib.check(lib.cips_siren_surface_x3(C.byref(sw), C.byref(rp), level, refine, ops._p(depth), ops._p(hit), ops._p(sigma),
                                                 ops._p(points), None, B, ops._stream()), "cips_siren_surface_x3")

        def leg_b():
            res["b"] = ops.siren_surface_composed(level, refine, geom, xg, yg, zg, c2w, *args)

        def leg_c():
            _lib.check(lib.cips_siren_sigma_x3(C.byref(sw), ops._p(rnd), ops._p(sig_c), B, P, ops._stream()), "cips_siren_sigma_x3")

        legs = [("a", leg_a), ("b", leg_b), ("c", leg_c)]
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
        # outside the timing: what the early exit skipped (the debug trace's NaN slots) and how the two searches agree
        trace = ops.siren_surface(level, refine, geom, xg, yg, zg, c2w, *args, trace=True)[4]
        seen = ~torch.isnan(trace[..., 0])
        skipped = 1.0 - float(seen[:, :, :S].float().mean())
        evals = float(seen.sum()) + B * n                                   # + the final evaluation of every ray
        del trace
        bd, bh = res["b"][0], res["b"][1]
        same = bh == hit
        frac = [float((hit == k).float().mean()) for k in (0, 1, 2)]
        work = {"a": evals, "b": float(B * n * (S + refine + 1)), "c": float(B * P)}
        for k, _ in legs:
            ts = sorted(times[k])
            med = ts[len(ts) // 2]
            lines.append(f"({k})   {B:<3} {med:10.3f}  {ts[0]:7.3f}  {ts[-1]:7.3f}  {B * n / (med * 1e-3) / 1e6:7.2f}  {work[k] / (med * 1e-3) / 1e9:7.3f}")
        ta, tb, tc = sorted(times["a"]), sorted(times["b"]), sorted(times["c"])
        ma, mb, mc = ta[len(ta) // 2], tb[len(tb) // 2], tc[len(tc) // 2]
        spread = max(tb[-1] - tb[0], ta[-1] - ta[0])
        lines.append(f"     B={B}: level {level:.4f}; miss / hit / inside {frac[0]:.2f} / {frac[1]:.2f} / {frac[2]:.2f}; the early exit skipped "
                     f"{100 * skipped:.1f} % of the coarse steps ({evals / (B * n):.1f} evaluations per ray of at most {S + refine + 1}); "
                     f"(b) - (a) = {mb - ma:.3f} ms (medians), largest min-max spread of the two = {spread:.3f} ms -> "
                     f"{'(a) is faster by more than the spread' if mb - ma > spread else '(a) is NOT faster by more than the spread'}; "
                     f"(b) / (a) = {mb / ma:.2f}, (a) / (c) = {ma / mc:.2f}; the composed search gives the same mask on "
                     f"{100 * float(same.float().mean()):.3f} % of the rays, max |depth difference| there {float((bd - depth).abs()[same].max()):.2e}")
        del rnd, sig_c, res
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
