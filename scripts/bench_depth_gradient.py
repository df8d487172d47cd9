"""Differentiable depth / opacity microbench at C2 (r64, batch 32; S = 24 flat and 12 + 12 hierarchical), one process, device-event
timings, legs alternated inside every repeat:

  a. forward() + backward of an image loss
  b. render()  + backward of the same image loss                     (the same kernels as a, plus the opacity store)
  c. render()  + backward of image + depth + opacity losses          (the `_geo` compositing backward)
  and the compositing backward alone at the flat shape, with and without the two upstream gradients

  --legs a runs leg a only: that is what a checkout without G.render can run, for the comparison with the commit before.

Real initialiser weights (bench.G_CFG under seed 0), fixed latents, eager launches.  The run-to-run spread of a leg is its
(max - min) over the alternated repeats; two legs agree when their medians differ by less than that.  The table goes to stdout
and is appended to --out."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import G_CFG, G_KW
from cips3d_amd import _lib, ops
from cips3d_amd.generator import GeneratorNerfINR


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def _timed(legs, repeats):
    times = {k: [] for k, _ in legs}
    for rep in range(repeats + 2):
        for k, fn in legs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 2:
                times[k].append(e0.elapsed_time(e1))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--img", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--legs", default="abc", choices=["a", "abc"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("at least 5 timed repeats per leg")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=d).to(d)
    G.device = d
    B, img = a.batch, a.img
    n = img * img
    zs = G.get_zs(B)
    params = list(G.parameters())
    G0 = torch.randn(B, 3, img, img, device=d) / (B * 3 * n)
    D0, O0 = torch.randn(B, 1, img, img, device=d) / (B * n), torch.randn(B, 1, img, img, device=d) / (B * n)
    lines = []

    def step(kind, S, hier):
        kw = dict(img_size=img, num_steps=S, hierarchical_sample=hier, nerf_noise=0., **G_KW)

        def run():
            for p in params:
                p.grad = None
            if kind == "a":
                imgs, _ = G(zs, **kw)
                imgs.backward(G0)
            else:
                r = G.render(zs, **kw)
                loss = (r.imgs * G0).sum()
                if kind == "c":
                    loss = loss + (r.depth * D0).sum() + (r.opacity * O0).sum()
                loss.backward()
        return run

    names = {"a": "a forward() + image loss", "b": "b render()  + image loss", "c": "c render()  + image, depth, opacity"}
    for S, hier in ((24, False), (12, True)):
        legs = [(names[k], step(k, S, hier)) for k in a.legs]
        times = _timed(legs, a.repeats)
        lines.append(f"G forward + backward, r{img}, S = {S}{' + ' + str(S) + ' hierarchical' if hier else ' flat'}, batch {B}, eager launches, "
                     f"{a.repeats} timed repeats per leg after 2 warm-up rounds, legs alternated")
        med = {}
        for k, ts in times.items():
            med[k], lo, hi = _median(ts)
            lines.append(f"  {k:<38} {med[k]:8.3f} ms (min {lo:.3f}, max {hi:.3f}, spread {hi - lo:.3f})")
        if a.legs == "abc":
            ma, mb, mc = (med[names[k]] for k in "abc")
            lines.append(f"  b - a = {mb - ma:+.3f} ms ({(mb / ma - 1) * 100:+.2f} %); the geometric losses add c - b = {mc - mb:+.3f} ms "
                         f"({(mc / mb - 1) * 100:+.2f} %)")

    if a.legs == "abc":
        # the compositing backward alone, flat shape: R = B * n rays of S = 24 samples
        lib = _lib.load()
        R, S = B * n, 24
        feat, sig = torch.randn(R, S, 32, device=d), torch.randn(R, S, device=d)
        z = torch.linspace(0.88, 1.12, S, device=d).expand(R, S).contiguous()
        dfea, dd, do = torch.randn(R, 32, device=d), torch.randn(R, device=d), torch.randn(R, device=d)
        dfeat, dsig = torch.empty_like(feat), torch.empty_like(sig)
        p_, st = ops._p, ops._stream
        head = (p_(feat), p_(sig), p_(z), None, None, None, None, 0.0, None, p_(dfea), p_(dfeat), p_(dsig), None, None, R, S, 0, 0, None)
        legs = [("cips_composite_bwd", lambda: _lib.check(lib.cips_composite_bwd(*head, st()), "bwd")),
                ("cips_composite_bwd_geo, both NULL", lambda: _lib.check(lib.cips_composite_bwd_geo(*head, None, None, st()), "geo0")),
                ("cips_composite_bwd_geo, ddepth + dopacity", lambda: _lib.check(lib.cips_composite_bwd_geo(*head, p_(dd), p_(do), st()), "geo"))]
        times = _timed(legs, a.repeats)
        moved = R * S * (2 * 128 + 2 * 4 + 4) + R * 128
        lines.append(f"compositing backward alone, R = {R} rays, S = {S}, relu, {moved / 1e6:.0f} MB moved, {a.repeats} timed repeats, alternated")
        for k, ts in times.items():
            m, lo, hi = _median(ts)
            lines.append(f"  {k:<42} {m:7.3f} ms (min {lo:.3f}, max {hi:.3f}, spread {hi - lo:.3f})  {moved / (m * 1e-3) / 1e12:.2f} TB/s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
