"""The D step of scripts/probe/d_step_only.py (forward on the real batch, R1 through the double-backward graph, forward on the
fake batch, backward; auxiliary discriminator, no optimizer) in the discriminator's two split-plane modes, CONV_MODE "bf16x3"
(3 passes, default) and "bf16" (single pass where discriminator._single_pass allows), inside ONE process: the modes alternated
--rounds times, --warmup untimed and --steps timed eager steps per visit, device-event times.  Two geometries: C2 (64 x 64,
batch 32) and 256 x 256 with batch 4 + 4 and DiffAugment.  Per mode also the in-situ microseconds of the three implicit-GEMM
convolution families (an event pair around every call of `reps` steps: forward / stride-1 data gradient, parity data gradient,
weight gradient incl. its finish pass), how many of those calls ran single-pass, and the in-situ time of the operators that
write split planes of activations and gradients (split_planes_nhwc, lrelu_bwd_bias_nhwc: their lo halves are what "bf16" mode
still writes and no longer reads; the batched weight prep is not in that figure).  And how far the mode moves the step's results: logits,
R1 input gradient and parameter gradients of one step on the same inputs and draws, "bf16" against "bf16x3".
Writes one JSON line to profiles/d_bf16_mode_bench.json and prints it.

    python scripts/bench_d_modes.py [--rounds 3] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

MODES = ("bf16x3", "bf16")
CONV_FAMILIES = {"conv2d_x3": "fwd_dgrad_s1", "conv2d_x3_dgrad_s2": "dgrad_parity", "conv2d_x3_wgrad": "wgrad"}
PLANE_WRITERS = ("split_planes_nhwc", "lrelu_bwd_bias_nhwc")


def in_situ(step, reps=2):
    """-> {family: launches per step, single-pass launches per step, ms per step} over `reps` eager steps"""
    from cips3d_amd import ops
    rec = []
    names = list(CONV_FAMILIES) + list(PLANE_WRITERS)
    real = {n: getattr(ops, n) for n in names}

    def wrap(name, family):
        def f(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = real[name](*a, **kw)
            e1.record()
            rec.append((family, bool(kw.get("single")), e0, e1))
            return out
        return f

    for n in names:
        setattr(ops, n, wrap(n, CONV_FAMILIES.get(n, "plane_writers")))
    try:
        step(); torch.cuda.synchronize(); rec.clear()
        for _ in range(reps):
            step()
        torch.cuda.synchronize()
    finally:
        for n, v in real.items():
            setattr(ops, n, v)
    by = {}
    for family, single, e0, e1 in rec:
        ent = by.setdefault(family, [0, 0, 0.0])
        ent[0] += 1; ent[1] += single; ent[2] += e0.elapsed_time(e1)
    return {k: {"calls_per_step": v[0] // reps, "single_pass_calls_per_step": v[1] // reps, "ms_per_step": round(v[2] / reps, 3)}
            for k, v in sorted(by.items())}


def geometry(name, img, b, diffaug, a, dev):
    from cips3d_amd import discriminator as dm
    torch.manual_seed(0)
    D = dm.Discriminator_MultiScale_Aux(diffaug=diffaug, max_size=1024, channel_multiplier=2, first_downsample=False, stddev_group=0).to(dev)
    real = torch.rand(b, 3, img, img, device=dev) * 2 - 1
    gen = torch.rand(2 * b, 3, img, img, device=dev) * 2 - 1
    params = list(D.parameters())
    last = {}

    def d_step():
        real2 = torch.cat([real, real]).requires_grad_(True)
        r_preds, _, _ = D(real2, alpha=1.0, use_aux_disc=True)
        grad_real, = torch.autograd.grad(outputs=r_preds.sum(), inputs=real2, create_graph=True)
        pen = 0.5 * 10.0 * grad_real.flatten(1).square().sum(1, keepdim=True)
        g_preds, _, _ = D(gen, alpha=1.0, use_aux_disc=True)
        loss = (F.softplus(g_preds) + F.softplus(-r_preds) + pen).mean()
        for p in params:
            p.grad = None
        loss.backward()
        last["out"], last["gr"] = r_preds.detach(), grad_real.detach()

    keep = dm.CONV_MODE
    situ, results, visits = {}, {}, {m: [] for m in MODES}
    try:
        for mode in MODES:                               # the mode is read per call
            dm.CONV_MODE = mode
            d_step(); torch.cuda.synchronize()
            situ[mode] = in_situ(d_step)
            torch.manual_seed(7)                         # DiffAugment's draws: the same in both modes
            d_step(); torch.cuda.synchronize()
            results[mode] = (last["out"].double(), last["gr"].double(), [None if p.grad is None else p.grad.double().clone() for p in params])
        for _ in range(a.rounds):
            for mode in MODES:
                dm.CONV_MODE = mode
                for _ in range(a.warmup):
                    d_step()
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
                for i in range(a.steps):
                    evs[i].record()
                    d_step()
                evs[-1].record()
                torch.cuda.synchronize()
                ts = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(a.steps))
                visits[mode].append({"mean_ms": round(evs[0].elapsed_time(evs[-1]) / a.steps, 4), "median_ms": round(ts[len(ts) // 2], 4)})
    finally:
        dm.CONV_MODE = keep
    rel = lambda x, y: float((x - y).norm() / y.norm().clamp_min(1e-300))
    (o3, g3, p3), (o1, g1, p1) = results["bf16x3"], results["bf16"]
    perr = [rel(x, y) for x, y in zip(p1, p3) if y is not None and float(y.abs().max()) > 0]
    out = {"workload": f"{name}: {img} x {img}, batch {b} real (x2: R1) + {2 * b} fake, aux discriminator" + (", DiffAugment" if diffaug else ""),
           "movement_bf16_vs_bf16x3": {"logits_rel_l2": rel(o1, o3), "logits_max_abs": float((o1 - o3).abs().max()),
                                       "r1_input_gradient_rel_l2": rel(g1, g3), "parameter_gradient_rel_l2_median": statistics.median(perr),
                                       "parameter_gradient_rel_l2_max": max(perr)}}
    for mode in MODES:
        ms = sum(v["mean_ms"] for v in visits[mode]) / len(visits[mode])
        out[mode] = {"ms_per_step": round(ms, 4), "visits": visits[mode], "in_situ": situ[mode]}
    out["speedup_step"] = round(out["bf16x3"]["ms_per_step"] / out["bf16"]["ms_per_step"], 4)
    for fam in CONV_FAMILIES.values():
        if fam in situ["bf16"] and fam in situ["bf16x3"] and situ["bf16"][fam]["ms_per_step"] > 0:
            out[f"speedup_{fam}"] = round(situ["bf16x3"][fam]["ms_per_step"] / situ["bf16"][fam]["ms_per_step"], 3)
    pw = situ["bf16"].get("plane_writers")
    if pw:
        out["plane_writers_share_of_bf16_step"] = round(pw["ms_per_step"] / out["bf16"]["ms_per_step"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "d_bf16_mode_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"rounds": a.rounds, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
           "c2": geometry("C2", 64, 32, False, a, dev), "r256": geometry("r256", 256, 4, True, a, dev)}
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
