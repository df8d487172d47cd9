"""The headline G step (bench.py's C2 geometry: r64, 24 SIREN evaluations per ray, batch 32, G forward + backward, captured with
cips3d_amd.graph.capture) in the head's two split-plane modes, INR_MODE "bf16x3" (3 passes, default) and "bf16" (single pass),
inside ONE process: one captured graph per mode, the modes alternated --rounds times, --warmup untimed and --steps timed replays
per visit, device-event times.  Also the in-situ microseconds of the head's NT and K-major GEMM launches per mode (an event pair
around every launch of `reps` eager steps, as bench.py --full's roofline leg does).  Prints one JSON line.

    python scripts/bench_inr_modes.py [--rounds 3] [--steps 50] [--warmup 10]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

MODES = ("bf16x3", "bf16")


def in_situ(fwd_bwd, n, reps=3):
    """-> {launch family: (launches per step, mean microseconds)} of the head's 512-wide GEMMs in `reps` eager steps"""
    from cips3d_amd import ops
    rec = []
    real = {k: getattr(ops, k) for k in ("gemm_x3", "gemm_x3_torgb", "gemm_x3_km", "gemm_x3_km_grouped")}

    inside = [False]       # a wrapped call is running: what it launches itself (the grouped entry's one-by-one fallback) belongs to its pair

    def wrap(name, family, is_head):
        def f(*a, **kw):
            if inside[0] or not is_head(a):
                return real[name](*a, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            inside[0] = True
            try:
                e0.record()
                real[name](*a, **kw)
                e1.record()
            finally:
                inside[0] = False
            rec.append((family, e0, e1))
        return f

    nt = lambda a: tuple(a[2:5]) == (n, 512, 512)                      # (A, B, M, N, K, ...)
    ops.gemm_x3, ops.gemm_x3_torgb = wrap("gemm_x3", "nt", nt), wrap("gemm_x3_torgb", "nt", nt)
    ops.gemm_x3_km = wrap("gemm_x3_km", "km", lambda a: tuple(a[2:4]) == (512, 512))
    ops.gemm_x3_km_grouped = wrap("gemm_x3_km_grouped", "km_grouped", lambda a: tuple(a[1:3]) == (512, 512))   # (problems, M, N, K, ...)
    try:
        fwd_bwd(); torch.cuda.synchronize(); rec.clear()
        for _ in range(reps):
            fwd_bwd()
        torch.cuda.synchronize()
    finally:
        for k, v in real.items():
            setattr(ops, k, v)
    by = {}
    for family, e0, e1 in rec:
        by.setdefault(family, []).append(e0.elapsed_time(e1) * 1e3)
    return {k: {"launches_per_step": len(v) // reps, "launch_us": round(sum(v) / len(v), 1),
                "ms_per_step": round(sum(v) / reps * 1e-3, 3)} for k, v in sorted(by.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--img-size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--num-steps", type=int, default=24)
    a = ap.parse_args()
    import bench
    from cips3d_amd import ops
    from cips3d_amd.generator import GeneratorNerfINR
    from cips3d_amd.graph import capture
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    G = GeneratorNerfINR(**bench.G_CFG, device=dev).to(dev)
    G.device = dev
    b, img, S = a.batch, a.img_size, a.num_steps
    G0 = torch.randn(b, 3, img, img, device=dev) / (b * 3 * img * img)
    params = list(G.parameters())

    def fwd_bwd():
        zs = G.get_zs(b)
        for p in params:
            p.grad = None
        imgs, _ = G(zs, img_size=img, num_steps=S, hierarchical_sample=False, nerf_noise=0., return_aux_img=False,
                    grad_points=None, forward_points=None, **bench.G_KW)
        imgs.backward(G0)

    keep = ops.INR_MODE
    graphs, situ = {}, {}
    try:
        for mode in MODES:                       # the mode is read when the head runs: each graph keeps the one it was captured in
            ops.INR_MODE = mode
            situ[mode] = in_situ(fwd_bwd, img * img)
            graphs[mode] = capture(fwd_bwd, warmup=2, params=params)
    finally:
        ops.INR_MODE = keep
    visits = {m: [] for m in MODES}
    for _ in range(a.rounds):
        for mode in MODES:
            g = graphs[mode]
            for _ in range(a.warmup):
                g()
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
            for i in range(a.steps):
                evs[i].record()
                g()
            evs[-1].record()
            torch.cuda.synchronize()
            ts = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(a.steps))
            visits[mode].append({"mean_ms": round(evs[0].elapsed_time(evs[-1]) / a.steps, 4), "median_ms": round(ts[len(ts) // 2], 4)})
    out = {"workload": f"r{img}, {S} SIREN evals/ray, batch {b}, G fwd+bwd, hipGraph replay", "rounds": a.rounds, "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(dev)}
    for mode in MODES:
        ms = sum(v["mean_ms"] for v in visits[mode]) / len(visits[mode])
        out[mode] = {"ms_per_step": round(ms, 4), "img_per_s": round(b / ms * 1e3, 1), "visits": visits[mode], "head_gemms_in_situ": situ[mode]}
    out["speedup_step"] = round(out["bf16x3"]["ms_per_step"] / out["bf16"]["ms_per_step"], 4)
    for fam in situ["bf16"]:
        if fam in situ["bf16x3"]:
            out[f"speedup_{fam}"] = round(situ["bf16x3"][fam]["launch_us"] / situ["bf16"][fam]["launch_us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
