#!/usr/bin/env python
"""One generator forward + backward step of generator_v1.GeneratorNerfINR against generator.GeneratorNerfINR at the C2 geometry
of bench.py (r64, S=24 flat, batch 32, fresh latents, hipGraph replay), timed with bench.py's pattern: warm-up steps, a fence,
then the wall clock of --steps steps between fences, plus per-step event times.  The two generators run one after the other in
one process, v0 first.  Prints one JSON line.  A single measurement, not a benchmark of record.

v1 joins the INR mapping side stream before the ray march (its colour FiLM reads nerf_rgb_mapping's output), where v0 joins
right before the INR head ("generator_v1"); this shows what that costs at the headline geometry.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import G_CFG, G_KW           # noqa: E402


def rate(G, dev, b, img, S, hier, steps, warmup, graph):
    """-> (ms per step over the timed window, median per-step event time in ms, launch mode)"""
    torch.manual_seed(1234)
    G0 = torch.randn(b, 3, img, img, device=dev) / (b * 3 * img * img)
    params = list(G.parameters())

    def fwd_bwd():
        zs = G.get_zs(b)
        for p in params:
            p.grad = None
        imgs, _ = G(zs, img_size=img, num_steps=S, hierarchical_sample=hier, nerf_noise=0., return_aux_img=False,
                    grad_points=None, forward_points=None, **G_KW)
        imgs.backward(G0)

    step = fwd_bwd
    if graph:
        from cips3d_amd.graph import capture
        step = capture(fwd_bwd, warmup=2).replay
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    evs = []
    t0 = time.perf_counter()
    for _ in range(steps):
        e = torch.cuda.Event(enable_timing=True); e.record(); evs.append(e)
        step()
    e = torch.cuda.Event(enable_timing=True); e.record(); evs.append(e)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ts = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1))
    return dt / steps * 1e3, ts[len(ts) // 2], "hipGraph replay" if graph else "eager"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--img-size", type=int, default=64)
    ap.add_argument("--num-steps", type=int, default=24)
    ap.add_argument("--hier", action="store_true")
    ap.add_argument("--no-graph", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_v1_step.py needs a ROCm GPU")
    dev = torch.device("cuda", 0)
    from cips3d_amd import generator, generator_v1
    out = dict(metric="generator fwd+bwd step, ms", batch=a.batch, img_size=a.img_size, num_steps=a.num_steps, hier=a.hier,
               steps=a.steps, warmup=a.warmup, note="single measurement; v0, then v1, in one process")
    for name, cls in (("v0", generator.GeneratorNerfINR), ("v1", generator_v1.GeneratorNerfINR)):
        torch.manual_seed(1234)
        G = cls(**G_CFG, device=dev).to(dev)
        G.device = dev
        ms, med, launch = rate(G, dev, a.batch, a.img_size, a.num_steps, a.hier, a.steps, a.warmup, not a.no_graph)
        out[name] = dict(ms_per_step=round(ms, 3), median_step_ms=round(med, 3), launch=launch)
        del G
        torch.cuda.empty_cache()
    out["v1_minus_v0_ms"] = round(out["v1"]["ms_per_step"] - out["v0"]["ms_per_step"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
