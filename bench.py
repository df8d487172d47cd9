#!/usr/bin/env python
"""bench.py — BASELINE.json metric: rendered images / second, generator forward + backward,
FFHQ geometry, synthetic latents, on N MI355X (one process per GPU, RCCL gradient all-reduce).

Workload at N=1 (config.workload): BASELINE configs[1] = C2 of SURVEY.md §8:
  img_size 64, 24 SIREN evaluations per ray, per-GPU batch 32, fp32.
  Default E=24 as S=24 / hierarchical off (SURVEY §8 "primary"); --hier gives S=12 + 12 resampled.
One step = G(zs, ...) forward on fresh latents + imgs.backward(G0) populating every generator
parameter gradient the reference populates (+ gradient all-reduce when N > 1).
Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times --steps steps and prints the headline; --full adds the
secondary legs (exact-fp32 timings, full GAN step, other geometries, roofline / power, cpu_baseline).
--dump-outputs DIR writes what the last timed step computed (images, parameter gradients) as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
G_KW = dict(fov=12, ray_start=0.88, ray_end=1.12, h_stddev=0.3, v_stddev=0.155, psi=1., sample_dist="gaussian")
G_CFG = dict(
    z_dim=256,
    nerf_cfg=dict(in_dim=3, hidden_dim=128, hidden_layers=2, rgb_dim=32, style_dim=128),
    mapping_nerf_cfg=dict(z_dim=256, hidden_dim=128, base_layers=4, head_layers=0),
    inr_cfg=dict(input_dim=32, style_dim=512, hidden_dim=512, pre_rgb_dim=3),
    mapping_inr_cfg=dict(z_dim=512, hidden_dim=512, base_layers=8, head_layers=0, add_norm=True, norm_out=True),
)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--img-size", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32, help="per-GPU batch")
    ap.add_argument("--num-steps", type=int, default=None, help="coarse samples per ray")
    ap.add_argument("--hier", action="store_true", help="hierarchical sampling (S coarse + S fine)")
    ap.add_argument("--freeze", action="store_true", help="GeneratorNerfINR_freeze_NeRF (the r256 stages: gradients for the INR head only)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the secondary legs (exact-fp32 timings, full GAN step, other geometries, "
                         "roofline / power, cpu_baseline); the --no-* options below trim them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (imgs, every parameter gradient) as DIR/<name>.npy, float32")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-exact", action="store_true", help="skip the extra exact-fp32-MFMA timing")
    ap.add_argument("--no-full-step", action="store_true",
                    help="skip the secondary measurement: one full GAN step (D step with R1 + G step + fused clip/Adam/EMA)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the short extra timings of BASELINE's other geometries (C4 at 256x256, C3's per-GPU share, C2 eager)")
    ap.add_argument("--inr-mode", default=None, choices=["bf16x3", "f32"])
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying the captured hipGraph of the step")
    ap.add_argument("--rccl", action="store_true",
                    help="N = 1: bring up a one-rank RCCL process group anyway and run the gradient exchange through it every step "
                         "(communicator init with device_id, thread-local graph capture beside the watchdog, presence exchange and "
                         "bucket all-reduce on RCCL's streams) — what a one-GPU box can execute of the N > 1 path; implied when "
                         "torchrun launched a single rank")
    ap.add_argument("--overlap-reduce", action="store_true",
                    help="N > 1: issue each gradient bucket's all-reduce from autograd hooks while backward is still running "
                         "(implies --no-graph; validated over gloo only: not the default)")
    return ap.parse_args()


BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA (the 5 PF headline includes 2:1 sparsity)


def _time_launches(fn, reps=60, warm=60):
    """average launch duration (s) with HIP events on the launch stream (torch's current stream); the warm-up is longer than the
    ~50 launches the clock controller takes to settle on a looped matrix-bound kernel (profiles/r5_power_envelope.txt)"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


HBM_PEAK_TBS = 8.0               # MI355X_MICROARCH.md: HBM3E


def gemm_roofline(dev, b, n, mode):
    """Dominant kernel FAMILY of the step (~45 % of GPU time): the 512x512 modulated-FC layer GEMMs of the CIPS head,
    every epilogue flavour the step launches, each timed live with events on the launch stream; `frac` is the
    launch-count-weighted family value (sum of algorithmic flops / sum of time / peak), the per-flavour rows are under
    `flavours`.  bf16x3 mode: every fp32 product is 3 bf16 MFMA passes, so the roof for ALGORITHMIC (fp32-equivalent)
    flops is the dense bf16 MFMA peak / 3.  f32 mode: gemm_f32_kernel on fp32 MFMA (forward form only)."""
    from cips3d_amd import ops
    x = torch.randn(b, n, 512, device=dev)
    w = torch.randn(b, 512, 512, device=dev) * 0.04
    flops = 2.0 * b * n * 512 * 512
    act_b = b * n * 512 * 4          # bytes of one (b, n, 512) fp32-equivalent tensor (two bf16 planes)
    w_b = b * 512 * 512 * 4
    if mode != "bf16x3":
        out = torch.empty(b, n, 512, device=dev)
        t = _time_launches(lambda: ops.bmm_nn(x, w, out=out, act=1))
        ach = flops / t / 1e12
        return {"bound": "mfma", "kernel": "gemm_f32_kernel<false,false> (modfc 512x512 fwd, act=lrelu)",
                "achieved": round(ach, 2), "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(ach / F32_MFMA_PEAK_TFLOPS, 4), "traffic": None, "launch_us": round(t * 1e6, 1),
                "flops_per_launch": flops, "hbm_frac": round((2 * act_b + w_b) / t / 1e12 / HBM_PEAK_TBS, 4)}
    peak = BF16_MFMA_PEAK_TFLOPS / 3.0
    xP, _ = ops.split_planes(x, want_t=False)
    wP, _ = ops.split_planes(w, want_t=False)
    oP = ops.Planes.empty(b, n, 512, device=dev)
    bits = torch.empty(b, n, 64, device=dev, dtype=torch.uint8)
    gate = (torch.rand(b, n, 64, device=dev) * 256).to(torch.uint8)
    rg = torch.randn(b * n, 3, device=dev)
    rw = torch.randn(3, 512, device=dev)
    G = lambda **kw: ops.gemm_x3(xP, wP, n, 512, 512, 512, 512, b, n * 512, 512 * 512, P=oP, **kw)
    # (name, launches per G fwd+bwd step at 9 blocks, callable, algorithmic HBM bytes per launch)
    nbits = b * n * 64
    part = torch.empty(4, b * n, 4, device=dev)          # ToRGB partials of the fused forward flavours (N / 128 blocks)
    flav = [
        ("fwd: lrelu, gate bits out, planes out  <ADD0,MASK0,RES0>", 11, lambda: G(act=1, mask_out=bits, gate_bits=2),
         2 * act_b + w_b + nbits),
        ("fwd + ToRGB partials  <0,0,0,RGBF>", 1, lambda: G(act=1, mask_out=bits, gate_bits=2, torgb=(rw, part)),
         2 * act_b + w_b + nbits + part.numel() * 4),
        ("fwd + residual planes + ToRGB partials  <0,0,1,RGBF>", 5,
         lambda: G(act=1, res=xP, mask_out=bits, gate_bits=2, torgb=(rw, part)), 3 * act_b + w_b + nbits + part.numel() * 4),
        ("dX: gate bits in, planes out  <0,1,0>", 12, lambda: G(mask=gate, gate_bits=1), 2 * act_b + w_b + nbits),
        ("dX + skip addend (previous layer's gated planes, un-gated on the fly) + ToRGB term + gate  <1,1,0,ADDP>", 5,
         lambda: G(addp=(xP, gate), rgb_g=rg, rgb_w=rw, mask=gate, gate_bits=1), 3 * act_b + w_b + 2 * nbits),
    ]
    rows, tot_t, tot_f = [], 0.0, 0.0
    for name, count, fn, bytes_ in flav:
        t = _time_launches(fn)
        rows.append({"flavour": name, "launches_per_step": count, "launch_us": round(t * 1e6, 1),
                     "achieved": round(flops / t / 1e12, 2), "frac": round(flops / t / 1e12 / peak, 4),
                     "algorithmic_bytes": bytes_, "hbm_frac": round(bytes_ / t / 1e12 / HBM_PEAK_TBS, 4)})
        tot_t += count * t
        tot_f += count * flops
    ach = tot_f / tot_t / 1e12
    r = {"bound": "mfma", "kernel": "gemm_bf16x3_v3_kernel family (modfc 512x512 layer GEMMs of the CIPS head, 256x256 tiles): "
                                    "launch-count-weighted over the five epilogue flavours of the step",
         "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
         "traffic": None, "launch_us": round(tot_t / sum(f[1] for f in flav) * 1e6, 1), "flops_per_launch": flops,
         "hbm_frac": round(sum(f[1] * f[3] for f in flav) / tot_t / 1e12 / HBM_PEAK_TBS, 4),
         "flavours": rows,
         "note": "algorithmic fp32-equivalent flops; raw bf16 MFMA rate = 3x achieved vs 2500 dense peak; hbm_frac = "
                 "algorithmic bytes / time / 8 TB/s"}
    # HBM bytes per launch of the forward flavour from the PMC counters, collected in their own rocprofv3 --pmc passes
    # (scripts/pmc_roofline.sh -> profiles/r2_roofline_pmc.json, r1 as fallback); null if absent
    for f in ("r6_roofline_pmc.json", "r5_roofline_pmc.json", "r4_roofline_pmc.json", "r3_roofline_pmc.json", "r2_roofline_pmc.json", "r1_roofline_pmc.json"):
        try:
            pm = json.load(open(os.path.join(ROOT, "profiles", f)))
            if b == 32 and n == 4096:
                r["traffic"] = pm["hbm_bytes"]
                r["traffic_algorithmic_bytes"] = pm["algorithmic_bytes"]
                r["traffic_kernel"] = pm["kernel"]
                r["traffic_source"] = (f"profiles/{f}: rocprofv3 --kernel-trace --pmc passes of scripts/pmc_roofline.sh on the same kernel and "
                                       "shape (counters cannot be collected inside this run); a tracked record, not a measurement of this run")
                break
        except Exception:
            pass
    return r


def head_gemm_in_situ(fwd_bwd, b, n, reps=3):
    """The same kernel family timed IN SITU: `reps` eager steps of the benchmarked workload with a HIP event pair around every
    512x512 modulated-FC GEMM launch of the head (events on the launch stream; the stream is in order, so the pair brackets
    exactly that kernel — between the large GEMMs of the head the host runs ahead and no launch gap falls inside a pair).
    -> per-flavour launch counts and mean durations as the step actually runs them (isolated launches on resident operands
    run 5-15 % faster than the same kernel behind its predecessor's 268 MB store burst: VERDICT r4 weak-2)."""
    from cips3d_amd import ops
    rec = []
    real_x3, real_torgb = ops.gemm_x3, ops.gemm_x3_torgb

    def flavour(kw, torgb):
        if kw.get("addp") is not None or kw.get("add") is not None:
            return "dX + skip addend + gate"
        if kw.get("mask") is not None:
            return "dX: gate bits in"
        if kw.get("res") is not None:
            return "fwd + residual" + (" + ToRGB partials" if torgb else "")
        return "fwd" + (" + ToRGB partials" if torgb else "")

    def timed_call(real, name, args, kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        real(*args, **kw)
        e1.record()
        rec.append((name, e0, e1))

    def x3(A, Bm, M, N, K, *rest, **kw):
        if (M, N, K) == (n, 512, 512):
            return timed_call(real_x3, flavour(kw, False), (A, Bm, M, N, K) + rest, kw)
        return real_x3(A, Bm, M, N, K, *rest, **kw)

    def x3_torgb(A, Bm, M, N, K, *rest, **kw):
        if (M, N, K) == (n, 512, 512):
            return timed_call(real_torgb, flavour(kw, True), (A, Bm, M, N, K) + rest, kw)
        return real_torgb(A, Bm, M, N, K, *rest, **kw)

    ops.gemm_x3, ops.gemm_x3_torgb = x3, x3_torgb
    try:
        fwd_bwd(); torch.cuda.synchronize(); rec.clear()
        for _ in range(reps):
            fwd_bwd()
        torch.cuda.synchronize()
    finally:
        ops.gemm_x3, ops.gemm_x3_torgb = real_x3, real_torgb
    flops = 2.0 * b * n * 512 * 512
    by = {}
    for name, e0, e1 in rec:
        by.setdefault(name, []).append(e0.elapsed_time(e1) * 1e-3)
    peak = BF16_MFMA_PEAK_TFLOPS / 3.0
    rows, tot_t, tot_n = [], 0.0, 0
    for name, ts in sorted(by.items()):
        t = sum(ts) / len(ts)
        rows.append({"flavour": name, "launches_per_step": len(ts) // reps, "launch_us": round(t * 1e6, 1),
                     "frac": round(flops / t / 1e12 / peak, 4)})
        tot_t += sum(ts); tot_n += len(ts)
    if not tot_n:
        return None
    ach = tot_n * flops / tot_t / 1e12
    return {"achieved": round(ach, 2), "frac": round(ach / peak, 4), "launch_us": round(tot_t / tot_n * 1e6, 1),
            "launches_per_step": tot_n // reps, "family_ms_per_step": round(tot_t / reps * 1e3, 3), "flavours": rows,
            "how": f"{reps} eager steps of the benchmarked workload, a HIP event pair around every head GEMM launch (ToRGB finish "
                   "launch of the fused flavours included in its pair)"}


def power_sample(run_step, seconds=1.5):
    """Socket power and shader clock while the benchmarked step replays (AFTER the timed region: a separate loop of `seconds`,
    sampled by a thread through rocm-smi).  -> dict or None when rocm-smi is not there.  Evidence, in the run's own line, for what
    profiles/r5_power_envelope.txt measured with a dedicated probe: the step runs against the board's power limit."""
    import re, shutil, subprocess, threading
    smi = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if not os.path.exists(smi):
        return None

    def one():
        try:
            out = subprocess.run([smi, "--showpower", "--showclocks", "--json"], capture_output=True, text=True, timeout=5).stdout
            c = next(iter(json.loads(out[out.index("{"):]).values()))
            pw = [float(v) for k, v in c.items() if "ower" in k and "(W)" in k]
            sc = [int(re.sub(r"[^0-9]", "", v)) for k, v in c.items() if k.lower().startswith("sclk clock speed")]
            return (pw[0] if pw else None), (sc[0] if sc else None)
        except Exception:                           # noqa: BLE001
            return None, None

    try:
        cap = subprocess.run([smi, "--showmaxpower", "--json"], capture_output=True, text=True, timeout=5).stdout
        capw = [float(v) for v in next(iter(json.loads(cap[cap.index("{"):]).values())).values()]
    except Exception:                               # noqa: BLE001
        capw = []
    samples, stop = [], threading.Event()
    th = threading.Thread(target=lambda: [samples.append(one()) for _ in iter(stop.is_set, True)])
    th.start()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
            run_step()
        torch.cuda.synchronize()
        n += 10
    dt = time.perf_counter() - t0
    stop.set(); th.join()
    pw = [p for p, _ in samples if p is not None]
    sc = [c for _, c in samples if c is not None]
    if not pw and not sc:
        return None
    return {"board_power_limit_w": capw[0] if capw else None, "socket_power_w": [min(pw), max(pw)] if pw else None,
            "sclk_mhz": [min(sc), max(sc)] if sc else None, "samples": len(samples), "steps": n,
            "ms_per_step_while_sampling": round(dt / n * 1e3, 3),
            "how": "rocm-smi --showpower --showclocks sampled by a thread during a separate replay loop after the timed region"}


def cpu_baseline(img_size, S, hier):
    """Oracle (CPU restatement of the reference path, kind 'port': /root/reference does not exist on the GPU box) on
    this host's cores, bounded sample per SURVEY.md §8d: b=4 images at the bench geometry (b=32 needs ~20 GB of
    autograd state on the CPU), 1 warm-up + 3 timed fwd+bwd, median, reported per image."""
    from oracle import cips3d_oracle as orc
    from cips3d_amd.generator import GeneratorNerfINR
    torch.manual_seed(1234)
    G = GeneratorNerfINR(**G_CFG, device="cpu")
    sd = dict(G.named_parameters())
    b, n = (4 if img_size <= 64 else 1), img_size * img_size
    E = 2 * S if hier else S
    g = torch.Generator().manual_seed(1)

    def one():
        zs = {"z_nerf": torch.randn(b, 256, generator=g), "z_inr": torch.randn(b, 512, generator=g)}
        rand = dict(jitter=torch.rand(b, n, S, 1, generator=g), theta=torch.randn(b, 1, generator=g),
                    phi=torch.randn(b, 1, generator=g), noise_c=torch.randn(b, n, S, 1, generator=g),
                    u=torch.rand(b * n, S, generator=g), noise_f=torch.randn(b, n, E, 1, generator=g))
        G.zero_grad()
        t0 = time.time()
        out = orc.generator_forward(sd, zs, rand, img_size, 12, 0.88, 1.12, S, 0.3, 0.155, hier)
        out["imgs"].backward(torch.ones_like(out["imgs"]) / out["imgs"].numel())
        return time.time() - t0
    # thread count: ATen's CPU kernels at this size stop scaling long before 128 threads (8 threads of the build container
    # run this sample 4x faster than all 128 of the GPU box's cores, scripts/time_reference_cpu.py): one warm-up iteration at
    # each candidate, the faster setting is timed
    all_threads = torch.get_num_threads()
    cands = sorted({all_threads, min(all_threads, 32), min(all_threads, 16)}, reverse=True)
    best = None
    for t in cands:
        torch.set_num_threads(t)
        dt1 = one()
        if best is None or dt1 < best[1]:
            best = (t, dt1)
    torch.set_num_threads(best[0])
    reps = 3
    ts = sorted(one() for _ in range(reps))
    torch.set_num_threads(all_threads)
    dt = ts[len(ts) // 2]
    return {"value": round(b / dt, 4), "unit": "img/s", "cores": best[0], "kind": "port",
            "sample": f"oracle G fwd+bwd, {img_size}x{img_size}, E={E} evals/ray, b={b}, median of {reps} timed iters "
                      f"(min {b / ts[-1]:.3f}, max {b / ts[0]:.3f} img/s) at {best[0]} threads, the fastest of {cands} "
                      f"(one warm-up iteration each; the box has {os.cpu_count()} logical CPUs)"}


def full_gan_step(dev, b, img, S, steps=4, warmup=2, freeze=False, diffaug=False, aux=True, torch_optim=False):
    """Secondary measurement: one full GAN training step as exp/cips3d/scripts/train.py:334-491 drives
    it — D step (G under no_grad with the aux image, R1 double-backward on the reals, clip, Adam), G step through the
    frozen D (clip, Adam, EMA) — on synthetic "real" images, with the fused step tail (FusedClipAdamEMA).  S coarse
    samples + hierarchical resampling (the training configuration).  Returns ms per phase and images / s."""
    import copy
    import torch.nn.functional as F
    from cips3d_amd.generator import GeneratorNerfINR, GeneratorNerfINR_freeze_NeRF
    from cips3d_amd.discriminator import Discriminator_MultiScale_Aux
    from cips3d_amd.optim import FusedClipAdamEMA
    torch.manual_seed(1234)
    G = (GeneratorNerfINR_freeze_NeRF if freeze else GeneratorNerfINR)(**G_CFG, device=dev).to(dev); G.device = dev
    G_ema = copy.deepcopy(G)
    D = Discriminator_MultiScale_Aux(diffaug=diffaug, max_size=1024, channel_multiplier=2, first_downsample=False,
                                     stddev_group=0).to(dev)
    kw = dict(G_KW); kw.update(num_steps=S, hierarchical_sample=True)
    if torch_optim:
        oG = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.0, 0.999)); oD = torch.optim.Adam(D.parameters(), lr=2e-3, betas=(0.0, 0.999))
    else:
        oG = FusedClipAdamEMA(G.parameters(), lr=2e-4, betas=(0.0, 0.999), max_norm=10.0, ema_params=G_ema.parameters())
        oD = FusedClipAdamEMA(D.parameters(), lr=2e-3, betas=(0.0, 0.999), max_norm=10.0)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.manual_seed(1234 + torch.distributed.get_rank())     # per-rank reals, latents and cameras (train.py:221)
    real = torch.rand(b, 3, img, img, device=dev) * 2 - 1
    # N > 1 (scripts/bench_full_step.py --gpus N): the step exchanges BOTH gradient sets, like the reference's two DDP
    # wrappers (train.py:235-236) — D's after the D backward (~150 MB, three buckets), G's after the G backward (45 MB)
    # (a one-rank group — bench.py --rccl — runs the same exchanges: what a one-GPU box can execute of this path)
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    red_bytes = {"D": 0, "G": 0}
    if dist_on:
        from cips3d_amd.distributed import GradAllReducer
        one = torch.distributed.get_world_size() == 1
        red_D = GradAllReducer(list(D.parameters()), single_rank_exchange=one)
        red_G = GradAllReducer(list(G.parameters()), single_rank_exchange=one)

    def d_step():
        for p in G.parameters(): p.requires_grad_(False)
        for p in D.parameters(): p.requires_grad_(True)
        with torch.no_grad():
            gen, _ = G(G.get_zs(b), img_size=img, nerf_noise=0.5, return_aux_img=aux, forward_points=None, grad_points=None, **kw)
        real2 = (torch.cat([real, real]) if aux else real.clone()).requires_grad_(True)
        r_preds, _, _ = D(real2, alpha=1.0, use_aux_disc=aux)
        grad_real, = torch.autograd.grad(outputs=r_preds.sum(), inputs=real2, create_graph=True)       # d_reg_every: 1
        pen = 0.5 * 10.0 * grad_real.flatten(1).square().sum(1, keepdim=True)
        g_preds, _, _ = D(gen, alpha=1.0, use_aux_disc=aux)
        loss = (F.softplus(g_preds) + F.softplus(-r_preds) + pen).mean()
        for p in D.parameters(): p.grad = None
        loss.backward()
        if dist_on:
            red_bytes["D"] = red_D()
        if torch_optim:
            torch.nn.utils.clip_grad_norm_(D.parameters(), 10.0)
        oD.step()

    def g_step():
        for p in G.parameters(): p.requires_grad_(True)
        for p in D.parameters(): p.requires_grad_(False)
        imgs, _ = G(G.get_zs(b), img_size=img, nerf_noise=0.5, return_aux_img=aux, grad_points=None, forward_points=None, **kw)
        preds, _, _ = D(imgs, alpha=1.0, use_aux_disc=aux)
        loss = F.softplus(-preds).mean()
        for p in G.parameters(): p.grad = None
        loss.backward()
        if dist_on:
            red_bytes["G"] = red_G()
        if torch_optim:
            torch.nn.utils.clip_grad_norm_(G.parameters(), 10.0); oG.step()
            with torch.no_grad():
                for e, p in zip(G_ema.parameters(), G.parameters()): e.copy_(e * 0.999 + p * 0.001)
        else:
            oG.step()

    for _ in range(warmup):
        d_step(); g_step()
    torch.cuda.synchronize()
    tD = tG = 0.0
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for _ in range(steps):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record(); d_step(); e1.record(); g_step(); e2.record()
        torch.cuda.synchronize()
        tD += e0.elapsed_time(e1); tG += e1.elapsed_time(e2)
    extra = {}
    if dist_on:
        # the same initial weights and the same averaged gradients on every rank: the parameters must still be identical
        world = torch.distributed.get_world_size()
        sums = torch.stack([torch.stack([p.detach().double().sum() for p in net.parameters()]).sum() for net in (G, D, G_ema)])
        allsums = [torch.zeros_like(sums) for _ in range(world)]
        torch.distributed.all_gather(allsums, sums)
        extra = {"ranks": world, "allreduce_bytes_D": int(red_bytes["D"]), "allreduce_bytes_G": int(red_bytes["G"]),
                 "replicas_identical": bool(all(torch.equal(allsums[0], t) for t in allsums[1:]))}
        b = b * world
    return {**extra,
            "metric": "full GAN step (D step with R1 + G step + clip/Adam/EMA), synthetic reals, eager launches",
            "img_size": img, "batch": b, "num_steps": S, "hierarchical": True, "aux": aux, "freeze_nerf": freeze,
            "diffaug": diffaug, "optimizer": "torch" if torch_optim else "fused clip+Adam+EMA", "steps": steps,
            "ms_D_step": round(tD / steps, 2), "ms_G_step": round(tG / steps, 2), "ms_step": round((tD + tG) / steps, 2),
            "img_per_s": round(b * steps / ((tD + tG) * 1e-3), 1)}


def g_step_rate(dev, img, b, S, hier, freeze, steps, warmup, graph=True):
    """images / s of the G forward + backward at another geometry of BASELINE.json (same step definition as the headline:
    fresh latents, every gradient the reference populates for that generator class; hipGraph replay unless graph=False)."""
    from cips3d_amd.generator import GeneratorNerfINR, GeneratorNerfINR_freeze_NeRF
    torch.manual_seed(1234)
    G = (GeneratorNerfINR_freeze_NeRF if freeze else GeneratorNerfINR)(**G_CFG, device=dev).to(dev)
    G.device = dev
    G0 = torch.randn(b, 3, img, img, device=dev) / (b * 3 * img * img)
    params = list(G.parameters())

    def fwd_bwd():
        zs = G.get_zs(b)
        for p in params:
            p.grad = None
        imgs, _ = G(zs, img_size=img, num_steps=S, hierarchical_sample=hier, nerf_noise=0., return_aux_img=False,
                    grad_points=None, forward_points=None, **G_KW)
        imgs.backward(G0)

    g = None
    if graph:
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    fwd_bwd()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fwd_bwd()
        except Exception as e:                      # noqa: BLE001
            print(f"[bench] other-config capture failed ({type(e).__name__}: {e}); eager", file=sys.stderr)
            g = None
            torch.cuda.synchronize()
    run = g.replay if g is not None else fwd_bwd
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    E = 2 * S if hier else S
    return {"workload": f"r{img}, {E} SIREN evals/ray (num_steps {S}, hierarchical {hier}), batch {b}, G fwd+bwd"
                        + (", NeRF frozen" if freeze else ""),
            "value": round(b * steps / dt, 2), "unit": "img/s", "ms_per_step": round(dt / steps * 1e3, 3), "steps": steps,
            "warmup": warmup, "launch": "hipGraph replay" if g is not None else "eager"}


def other_configs(dev, mode):
    """BASELINE.json's other geometries in the driver-timed line (north_star: img/s "at 64^2 and 256^2"): short runs, N = 1,
    rank 0, default numeric mode.  Each entry is guarded: a failure is reported in place and never costs the headline."""
    legs = [("c2_eager", "C2 with eager launches (what exp/cips3d/scripts/train.py does)", dict(img=64, b=32, S=24, hier=False, freeze=False, steps=10, warmup=3, graph=False)),
            ("c2_hier", "C2 as S = 12 + 12 resampled (ffhq_exp.yaml:169-189)", dict(img=64, b=32, S=12, hier=True, freeze=False, steps=10, warmup=3)),
            ("c3_r128_share", "C3's per-GPU share: r128, batch 64 / 8 GPUs (ffhq_exp.yaml:190-199)", dict(img=128, b=8, S=12, hier=True, freeze=False, steps=10, warmup=3)),
            ("c4_r256", "C4's G step: r256, E = 48, batch 4 per GPU, NeRF frozen (ffhq_exp.yaml:192-210)", dict(img=256, b=4, S=24, hier=True, freeze=True, steps=10, warmup=3)),
            ("c4_r256_full_backward", "r256, E = 48, batch 4, gradients for the NeRF as well", dict(img=256, b=4, S=24, hier=True, freeze=False, steps=6, warmup=2))]
    out = {}
    for key, what, kw in legs:
        try:
            r = g_step_rate(dev, **kw)
            r["what"] = what
            out[key] = r
        except Exception as e:                      # noqa: BLE001
            out[key] = {"what": what, "error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()
    return out


DUMP_CAP_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """name -> tensor: each written as out_dir/<name>.npy in float32.  Over DUMP_CAP_BYTES in all, every array of more than
    64 Ki elements is replaced by the same fixed fraction of its flattened elements (sorted indices drawn with seed 0, so two
    runs of the same configuration sample the same positions); smaller arrays are always written whole."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    big = [k for k, x in host.items() if x.size > 65536]
    total = sum(x.nbytes for x in host.values())
    keep = 1.0
    if total > DUMP_CAP_BYTES:
        small = total - sum(host[k].nbytes for k in big)
        keep = (DUMP_CAP_BYTES - small) / (total - small)
    for k, x in host.items():
        if keep < 1.0 and k in big:
            idx = np.random.RandomState(0).choice(x.size, max(1, int(x.size * keep)), replace=False)
            x = x.reshape(-1)[np.sort(idx)]
        np.save(os.path.join(out_dir, k + ".npy"), np.ascontiguousarray(x, dtype=np.float32))


def _free_port():
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def spawn_ranks(a):
    """`python bench.py --gpus N` without a launcher: re-exec under torch.distributed.run, one rank per GPU over RCCL
    (the form the driver's contract names); rank 0 of the child job prints the JSON line."""
    import subprocess
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL between processes needs it on this driver
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(a)
    rank = int(os.environ.get("RANK", 0))
    local = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a ROCm GPU (no CPU fallback for the product path)")
    # CIPS_BENCH_BACKEND=gloo: functional check of the N > 1 path on a box with fewer GPUs than ranks (ranks share
    # devices, the all-reduce goes through the host); never a measurement
    backend = os.environ.get("CIPS_BENCH_BACKEND", "nccl")
    local = local % torch.cuda.device_count() if backend != "nccl" else local
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if backend == "nccl" and torch.cuda.device_count() < world:
        raise SystemExit(f"bench.py: --gpus {world} needs {world} GPUs on this node, found {torch.cuda.device_count()} "
                         "(CIPS_BENCH_BACKEND=gloo runs a functional check with ranks sharing devices)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # a process group exists for N > 1, and for N = 1 when asked for (--rccl, or torchrun started the single rank)
    pg = world > 1 or a.rccl or ("WORLD_SIZE" in os.environ and "MASTER_ADDR" in os.environ)
    if pg:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")     # --rccl without a launcher
        if "MASTER_PORT" not in os.environ:
            os.environ["MASTER_PORT"] = str(_free_port())
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    from cips3d_amd.generator import GeneratorNerfINR, GeneratorNerfINR_freeze_NeRF
    from cips3d_amd.distributed import GradAllReducer
    from cips3d_amd import ops
    if a.inr_mode:
        ops.INR_MODE = a.inr_mode
    mode = ops.INR_MODE

    S = a.num_steps if a.num_steps is not None else (12 if a.hier else 24)
    torch.manual_seed(1234)                       # identical initial weights on every rank
    G = (GeneratorNerfINR_freeze_NeRF if a.freeze else GeneratorNerfINR)(**G_CFG, device=dev).to(dev)
    G.device = dev
    torch.manual_seed(1234 + rank)                # per-rank latents / cameras (train.py:221)
    b, img = a.batch, a.img_size
    G0 = torch.randn(b, 3, img, img, device=dev) / (b * 3 * img * img)
    params = list(G.parameters())
    overlap = bool(a.overlap_reduce and pg)
    if overlap:
        a.no_graph = True                      # hooks run in eager autograd only
    reduce_grads = GradAllReducer(params, bucket_mb=8.0 if overlap else 64.0, overlap=overlap, single_rank_exchange=pg and world == 1)
    # the images of the latest step, for --dump-outputs: an eager call keeps its own; in graph mode only the captured call's
    # (the graph's static output, rewritten by every replay) — nothing kept from a warm-up call is released inside the capture
    last = {}
    keep_eager = [True]

    def fwd_bwd():
        zs = G.get_zs(b)
        for p in params:
            p.grad = None
        imgs, _ = G(zs, img_size=img, num_steps=S, hierarchical_sample=a.hier, nerf_noise=0.,
                    return_aux_img=False, grad_points=None, forward_points=None, **G_KW)
        imgs.backward(G0)
        if keep_eager[0] or torch.cuda.is_current_stream_capturing():
            last["imgs"] = imgs

    graph = None
    if not a.no_graph:
        # ~570 kernel launches per step: capture latents (graph-safe Philox RNG: fresh draws per replay) + forward +
        # backward once, replay per step; the gradient all-reduce stays outside the graph.  Eager on any capture error.
        keep_eager[0] = False
        try:
            # the product's capture helper (cips3d_amd/graph.py): two eager warm-up calls on a side stream, then the capture;
            # with a process group up, RCCL's watchdog thread may touch the HIP runtime while this thread captures, so only
            # this thread's calls belong to the capture (thread_local)
            from cips3d_amd.graph import capture
            graph = capture(fwd_bwd, warmup=2, thread_local=pg)
        except Exception as e:                      # noqa: BLE001
            print(f"[bench] hipGraph capture failed ({type(e).__name__}: {e}); running eagerly", file=sys.stderr)
            graph = None
            torch.cuda.synchronize()
        keep_eager[0] = True
    use_graph = [graph is not None]

    ar_events, ar_bytes = [], [0]

    def step():
        if use_graph[0]:
            graph.replay()
        else:
            fwd_bwd()
        if pg:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ar_bytes[0] = reduce_grads() or ar_bytes[0]
            e1.record()
            ar_events.append((e0, e1))

    def fence():
        torch.cuda.synchronize()
        if pg:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    per_step = {}

    def timed(nsteps, nwarm, record=False):
        """wall clock of exactly nsteps steps between fences (the contract's number); with `record`, an event is
        recorded before every step and after the last, which costs nothing and gives the per-step distribution"""
        for _ in range(nwarm):
            step()
        fence()
        evs = []
        t0 = time.perf_counter()
        for _ in range(nsteps):
            if record:
                e = torch.cuda.Event(enable_timing=True); e.record(); evs.append(e)
            step()
        if record:
            e = torch.cuda.Event(enable_timing=True); e.record(); evs.append(e)
        fence()
        dt = time.perf_counter() - t0
        if record and len(evs) > 1:
            ts = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(len(evs) - 1))
            per_step.update(median=ts[len(ts) // 2], min=ts[0], max=ts[-1])
        if pg:
            t = torch.tensor([dt], device=dev)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            dt = float(t.item())
        return dt

    dt = timed(a.steps, a.warmup, record=True)
    ms = dt / a.steps * 1e3
    value = world * b * a.steps / dt
    if a.dump_outputs and rank == 0:
        # before any secondary leg runs the generator again: the images and the (all-reduced) gradients of the last timed step
        outs = {"imgs": last["imgs"]}
        outs.update({"grad." + k: p.grad for k, p in G.named_parameters() if p.grad is not None})
        dump_outputs(a.dump_outputs, outs)
    exact = None
    f32_all = None
    if a.full and mode == "bf16x3" and not a.no_exact:
        # two extra legs, timed like the headline (same launch mode, step count and warm-up):
        #  * f32_mfma_head_and_siren_forward: head GEMMs (forward and backward) and the SIREN forward on exact fp32 MFMA
        #    (v_mfma_f32_32x32x2_f32); the SIREN backward stays the fused split-bf16 kernel — the key says so;
        #  * f32_all (round 6): additionally the SIREN backward as an fp32 data pass with fp32-staged activations and fp32-MFMA
        #    weight-gradient GEMMs (CIPS_SIREN_BWD=staged_f32): no split operand anywhere in the step.
        fwd_was, bwd_was = ops.SIREN_FWD_MODE, ops.SIREN_BWD_MODE
        was, g_was = use_graph[0], graph

        def leg(siren_bwd):
            nonlocal graph
            ops.INR_MODE = "f32"
            ops.SIREN_FWD_MODE = "f32"
            ops.SIREN_BWD_MODE = siren_bwd
            g32 = None
            if was:
                try:
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        fwd_bwd()
                    torch.cuda.current_stream().wait_stream(side)
                    torch.cuda.synchronize()
                    g32 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g32, capture_error_mode="thread_local" if pg else "global"):
                        fwd_bwd()
                except Exception as e:                  # noqa: BLE001
                    print(f"[bench] hipGraph capture of the fp32 leg ({siren_bwd}) failed ({type(e).__name__}: {e}); eager", file=sys.stderr)
                    g32 = None
                    torch.cuda.synchronize()
            graph = g32
            use_graph[0] = g32 is not None
            try:
                dte = timed(a.steps, a.warmup)
                launch32 = "hipGraph replay" if use_graph[0] else "eager"
            finally:
                graph = g_was
                use_graph[0] = was
                ops.INR_MODE = mode
                ops.SIREN_FWD_MODE, ops.SIREN_BWD_MODE = fwd_was, bwd_was
            return {"value": round(world * b * a.steps / dte, 2), "ms_per_step": round(dte / a.steps * 1e3, 3), "steps": a.steps,
                    "warmup": a.warmup, "launch": launch32}

        exact = leg("x3")
        exact.update({"fp32_mfma": ["INR head GEMMs, forward and backward (gemm_f32_kernel)", "SIREN forward (siren.hip)"],
                      "split_bf16": ["SIREN backward (siren_bwd_x4_kernel, the fused form)"],
                      "note": "CIPS_INR_MODE=f32 CIPS_SIREN_FWD=f32"})
        try:
            f32_all = leg("staged_f32")
            f32_all.update({"fp32_mfma": ["INR head GEMMs, forward and backward", "SIREN forward", "SIREN backward: fp32 data pass "
                                          "(siren_bwd_kernel, activations staged as fp32) + weight-gradient GEMMs on gemm_f32_kernel (k-major A)"],
                            "split_operand": [], "note": "CIPS_INR_MODE=f32 CIPS_SIREN_FWD=f32 CIPS_SIREN_BWD=staged_f32; rays, SIREN and "
                            "composite as separate launches (the fused march exists in the split-operand form only)"})
        except Exception as e:                          # noqa: BLE001 — an extra leg must never cost the headline line
            f32_all = {"error": f"{type(e).__name__}: {e}"}
    E = 2 * S if a.hier else S
    line = {
        "metric": "rendered imgs/sec (G fwd+bwd)", "value": round(value, 2), "unit": "img/s", "n_gpus": world,
        "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 3),
        "ms_per_step_median": round(per_step.get("median", ms), 3), "ms_per_step_min": round(per_step.get("min", ms), 3),
        "ms_per_step_max": round(per_step.get("max", ms), 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if mode == "f32" else ("f32 (dense layers as 3-pass split-operand MFMA with fp32 accumulate: SIREN forward on fp16 hi/lo planes, "
                                               "~2e-7 rel., sigma in the fp32 class; INR head and all backward GEMMs on bf16 hi/lo planes, ~5e-6 rel. per "
                                               "layer; everything else fp32)"),
        "data": "synthetic",
        "config": {"workload": f"FFHQ r{img}, {E} SIREN evals/ray (num_steps {S}, hierarchical {a.hier}), "
                               f"batch {b}/GPU, G fwd+bwd, all 9 CIPS blocks" + (", NeRF frozen" if a.freeze else ""),
                   "global_batch": world * b, "parallelism": f"dp{world}", "rccl_ranks": (world if backend == "nccl" else 0) if pg else 0,
                   "inr_gemm_mode": mode,
                   "launch": "hipGraph replay" if use_graph[0] else "eager",
                   "grad_reduce": ("bucketed all-reduce issued from autograd hooks during backward" if overlap else
                                   "flat-bucket all-reduce after backward") if pg else "none"},
        **({"backend_note": f"{backend} functional check, not a measurement"} if backend != "nccl" and world > 1 else {}),
    }
    if exact:
        line["f32_mfma_head_and_siren_forward"] = exact
    if f32_all:
        line["f32_all"] = f32_all
    if pg and ar_events:
        # gradient exchange as the stream sees it (events around the all-reduce of every timed step; with the overlapped
        # form this is what is left exposed after the backward): median ms, bytes per rank, ring bus bandwidth
        tail = ar_events[-a.steps:]
        ts = sorted(e0.elapsed_time(e1) for e0, e1 in tail)
        med = ts[len(ts) // 2]
        line["allreduce"] = {"ms_median": round(med, 4), "ms_min": round(ts[0], 4), "ms_max": round(ts[-1], 4),
                             "bytes_per_rank": int(ar_bytes[0]),
                             "bus_GBps": round(ar_bytes[0] * 2 * (world - 1) / world / (med * 1e-3) / 1e9, 2) if (med > 0 and world > 1) else None,
                             # both terms from this rank's own stream events (median all-reduce / median step)
                             "step_ms_median_events": round(per_step.get("median", ms), 4),
                             "frac_of_step": round(med / max(per_step.get("median", ms), 1e-9), 4)}
    if a.full and rank == 0 and world == 1 and not a.no_full_step:
        try:
            line["full_step"] = full_gan_step(dev, b, img, 12, steps=4, warmup=2)
        except Exception as e:                      # noqa: BLE001 — the secondary number must never cost the headline line
            line["full_step"] = {"error": f"{type(e).__name__}: {e}"}
    if a.full and rank == 0 and world == 1 and not a.no_other_configs and mode == "bf16x3":
        line["other_configs"] = other_configs(dev, mode)
    if rank == 0:
        if a.full and not a.no_roofline:
            r = gemm_roofline(dev, b, img * img, mode)
            if mode == "bf16x3" and world == 1:
                try:
                    ins = head_gemm_in_situ(fwd_bwd, b, img * img)
                except Exception as e:                      # noqa: BLE001
                    ins = {"error": f"{type(e).__name__}: {e}"}
                if ins and "frac" in ins:
                    # the line's achieved / frac / launch_us are the IN-SITU family values; the isolated-launch microbenchmark
                    # (what rounds 2-4 quoted) stays beside them
                    r["isolated"] = {k: r[k] for k in ("achieved", "frac", "launch_us", "hbm_frac")}
                    r["isolated"]["flavours"] = r.pop("flavours")
                    r["achieved"], r["frac"], r["launch_us"] = ins["achieved"], ins["frac"], ins["launch_us"]
                    r["hbm_frac"] = None
                    r["measured"] = "in situ: " + ins["how"]
                r["in_situ"] = ins
            try:
                # the shader clock the family runs at INSIDE the step (per-dispatch counters: profiles/r6_step_clock.txt) and the
                # family priced against the roof at that clock; a tracked record, `frac` stays priced against the nominal peak
                sc = json.load(open(os.path.join(ROOT, "profiles", "r6_step_clock.json")))
                if mode == "bf16x3" and isinstance(r.get("achieved"), (int, float)):
                    r["sclk_ghz_in_step"] = sc["head_gemm_family_sclk_ghz"]
                    r["frac_at_step_clock"] = round(r["achieved"] / (r["peak"] * sc["head_gemm_family_sclk_ghz"] / sc["nominal_sclk_ghz"]), 4)
                    r["step_clock_source"] = sc["source"]
            except Exception:                       # noqa: BLE001
                pass
            try:
                # what the board's 1400 W limit leaves of the nominal (2.4 GHz) roof on real operands: a tracked record of the
                # power probe, not a measurement of this run — `frac` above stays priced against the nominal peak
                pw = json.load(open(os.path.join(ROOT, "profiles", "r5_power_envelope.json")))
                if mode == "bf16x3" and isinstance(r.get("achieved"), (int, float)):
                    r["power_limited"] = {"board_power_limit_w": pw["board_power_limit_w"],
                                          "sustained_tflops": pw["sustained_x3_tflops"],
                                          "frac_of_sustained": round(r["achieved"] / pw["sustained_x3_tflops"], 4),
                                          "source": pw["source"],
                                          "note": "every matrix-bound launch on real operands pins the socket at its power limit and the "
                                                  "shader clock drops to 1.75-1.9 GHz; the same kernels hold 2.4 GHz on zero operands "
                                                  "(K-major schedule 0.84 of the nominal roof)"}
            except Exception:                       # noqa: BLE001
                pass
            line["roofline"] = r
        if a.full and world == 1 and not a.no_roofline:
            try:
                line["power"] = power_sample(step)
            except Exception as e:                      # noqa: BLE001
                line["power"] = {"error": f"{type(e).__name__}: {e}"}
        if a.full and world == 1 and not a.no_cpu_baseline:
            line["cpu_baseline"] = cpu_baseline(img, S, a.hier)
            try:
                # the UNMODIFIED reference's CPU path: it exists only in the build container (/root/reference does not travel),
                # so its timing is a tracked record written there by scripts/time_reference_cpu.py — never measured here
                line["cpu_baseline"]["reference"] = json.load(open(os.path.join(ROOT, "profiles", "reference_cpu.json")))
            except Exception:                       # noqa: BLE001
                pass
        print(json.dumps(line), flush=True)
    if pg:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
