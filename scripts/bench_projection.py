"""Image projection (cips3d_amd/projection.py) measured on one GPU; the table goes to stdout and is appended to --out.

  1. steps per second of project() at the reference Projector's options (64 x 64, 24 samples per ray, flat sampling, mean styles
     of 10 000 latents) for batch 1, 8 and 32: wall clock around project(steps=N) ending in a device synchronise, for two step
     counts; the difference of the two over the difference of the counts is the time of a step without the set-up
  2. the pyramid loss kernel against the same loss composed from ATen operations (avg_pool2d, elementwise, reductions; autograd
     backward), forward + backward, device events, legs alternated
  3. the loss ratio reached after --fit-steps steps on a self-generated target, with one level and with upper pyramid levels
  4. the yaw fit_camera recovers from a 0.15 rad offset

  --profile N: run N steps at --batch only (the run to put under a kernel trace: scripts/prof_cmd.sh projection python
  scripts/bench_projection.py --profile 50 --batch 8); its per-kernel table gives the share of every kernel of a step.

Initialiser weights (bench.G_CFG under seed 0): there is no trained checkpoint in this repository, so parts 3 and 4 describe the
loop's behaviour on an untrained generator, whose images depend only weakly on styles and camera."""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from bench import G_CFG
from cips3d_amd import ops
from cips3d_amd.generator import GeneratorNerfINR
from cips3d_amd.projection import project

CAM = dict(fov=12, ray_start=0.88, ray_end=1.12, num_steps=24)


def _stat(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def aten_loss(pred, target, weight, level_weights, kind, eps):
    """ops.pyramid_loss as tensor operations (tests/fit_loss_oracle.py in the inputs' dtype)"""
    d = pred - target
    w = weight
    loss = 0
    for l, lam in enumerate(level_weights):
        if l:
            d = F.avg_pool2d(d, 2)
            w = F.avg_pool2d(w, 2) if w is not None else None
        r = d * d if kind == "mse" else torch.sqrt(d * d + eps * eps) - eps
        if w is not None:
            r = r * w
        loss = loss + lam * r.sum(dim=(1, 2, 3)) / (d.shape[1] * d.shape[2] * d.shape[3])
    return loss


def _target(G, b, img, dev, seed, yaw=math.pi / 2):
    g = torch.Generator().manual_seed(seed)
    zs = {"z_nerf": torch.randn(b, 256, generator=g).to(dev), "z_inr": torch.randn(b, 512, generator=g).to(dev)}
    with torch.no_grad():
        return G(zs, img_size=img, h_stddev=0., v_stddev=0., hierarchical_sample=False, psi=0.7, sample_dist="gaussian",
                 h_mean=yaw, **CAM)[0].clone()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", type=int, default=64)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--steps", type=int, nargs=2, default=[20, 60], help="the two step counts of part 1")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fit-steps", type=int, default=200)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=dev).to(dev)
    G.device = dev
    img = a.img
    if a.profile:
        target = _target(G, a.batch, img, dev, 1)
        project(G, target, steps=3, seed=1, **CAM)                       # code objects, library heuristics
        torch.cuda.synchronize()
        project(G, target, steps=a.profile, seed=1, **CAM)
        torch.cuda.synchronize()
        return
    lines = [f"project() at {img} x {img}, 24 samples per ray, flat sampling, init_samples 10000, noise 0.03, level_weights (1,), mse; "
             f"eager launches, wall clock to a device synchronise, {a.repeats} repeats per step count, counts alternated"]
    n0, n1 = a.steps
    for b in a.batches:
        target = _target(G, b, img, dev, 1)
        project(G, target, steps=3, seed=1, **CAM)
        torch.cuda.synchronize()
        ts = {n0: [], n1: []}
        for _ in range(a.repeats):
            for n in (n0, n1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                project(G, target, steps=n, seed=1, **CAM)
                torch.cuda.synchronize()
                ts[n].append(time.perf_counter() - t0)
        (m0, lo0, hi0), (m1, lo1, hi1) = _stat(ts[n0]), _stat(ts[n1])
        per = (m1 - m0) / (n1 - n0)
        lines.append(f"  batch {b:2d}: {n0} steps {m0 * 1e3:8.1f} ms (min {lo0 * 1e3:.1f}, max {hi0 * 1e3:.1f}), {n1} steps {m1 * 1e3:8.1f} ms "
                     f"(min {lo1 * 1e3:.1f}, max {hi1 * 1e3:.1f}) -> {per * 1e3:7.3f} ms per step, {1 / per:7.1f} steps/s, "
                     f"{b / per:8.1f} image-steps/s; set-up {(m0 - n0 * per) * 1e3:.1f} ms")

    lines.append("pyramid loss, forward + backward of sum(loss): the HIP kernels against the same loss from ATen operations, charbonnier, "
                 "weighted; device events, 20 timed repeats after 3 warm-up rounds, legs alternated")
    lam = (1.0, 0.5, 0.25, 0.125, 0.0625, 0.03, 0.015)
    for (b, c, h, w, L) in ((32, 3, 64, 64, 5), (4, 3, 256, 256, 7)):
        pred = (torch.rand(b, c, h, w, device=dev) * 2 - 1).requires_grad_(True)
        target, weight = torch.rand(b, c, h, w, device=dev) * 2 - 1, torch.rand(b, 1, h, w, device=dev)

        def leg(fn):
            def run():
                pred.grad = None
                fn(pred, target, weight, lam[:L], "charbonnier", 1e-3).sum().backward()
            return run
        legs = [("ops.pyramid_loss", leg(ops.pyramid_loss)), ("ATen composition", leg(aten_loss))]
        times = {k: [] for k, _ in legs}
        for rep in range(23):
            for k, fn in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    times[k].append(e0.elapsed_time(e1))
        g_own = leg(ops.pyramid_loss)() or pred.grad.clone()
        g_aten = leg(aten_loss)() or pred.grad.clone()
        err = float((g_own - g_aten).abs().max() / g_aten.abs().max())
        lines.append(f"  ({b}, {c}, {h}, {w}) L = {L}: gradients agree to max_rel {err:.1e}")
        for k, t in times.items():
            m, lo, hi = _stat(t)
            lines.append(f"    {k:<18} {m * 1e3:8.1f} us (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")

    b = 8
    target = _target(G, b, img, dev, 2)
    lines.append(f"fit to a self-generated target (psi 0.7 styles, batch {b}), {a.fit_steps} steps, lr 1e-2, noise 0.03: pixel MSE of the last "
                 f"render over the pixel MSE of the first, per image min / median / max")
    for name, lw in (("level_weights (1,)", (1.,)), ("level_weights (1, 1, 1, 1)", (1., 1., 1., 1.))):
        res = project(G, target, steps=a.fit_steps, level_weights=lw, seed=3, **CAM)
        first = project(G, target, steps=1, level_weights=(1.,), seed=3, **CAM).losses[0]
        last = ((res.imgs - target) ** 2).mean(dim=(1, 2, 3))
        ratio = (last / first).cpu()
        own = (res.losses[-5:].mean(0) / res.losses[0]).cpu()
        lines.append(f"  {name:<28} MSE ratio {float(ratio.min()):.3f} / {float(ratio.median()):.3f} / {float(ratio.max()):.3f}; its own loss, "
                     f"mean of the last five over the first: {float(own.min()):.3f} / {float(own.median()):.3f} / {float(own.max()):.3f}")

    # camera: the target is the render of the mean styles the loop starts from, at yaw pi / 2; the loop starts 0.15 rad off
    torch.manual_seed(4)
    with torch.no_grad():
        avg = G.generate_avg_frequencies(num_samples=10000, device=dev)
        styles = {n: avg[n].expand(2, -1).contiguous() for n in G.style_names}
        torch.manual_seed(5)
        target = G.forward_styles(styles, img_size=img, h_stddev=0., v_stddev=0., hierarchical_sample=False, sample_dist="gaussian",
                                  **CAM)[0].clone()
    res = project(G, target, steps=a.fit_steps, fit_styles=False, fit_camera=True, camera_lr=1e-2, noise=0., h_mean=math.pi / 2 + 0.15,
                  seed=4, **CAM)
    off = (res.h_mean - math.pi / 2).flatten().tolist()
    lines.append(f"fit_camera alone from yaw pi/2 + 0.150, target at pi/2, {a.fit_steps} steps, camera_lr 1e-2: remaining yaw offset "
                 f"{', '.join(f'{v:+.4f}' for v in off)} rad; pitch offset {', '.join(f'{v:+.4f}' for v in (res.v_mean - math.pi / 2).flatten().tolist())} rad; "
                 f"loss {', '.join(f'{v:.3e}' for v in res.losses[0].tolist())} -> {', '.join(f'{v:.3e}' for v in res.losses[-1].tolist())}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
