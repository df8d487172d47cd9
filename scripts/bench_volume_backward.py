"""Baked-volume backward microbench: what the gradient of a view with respect to the nodes costs (cips_volume_render_bwd), next
to the forward of the same view, for both shapes of its atomic adds.  Device-event timings over windows of at least --window-ms
of calls, legs alternated inside every repeat of one process (scripts/bench_volume.py's scheme):

  per N (default 128), img x img, S samples per ray, 1 camera and a turntable of 8 over the one volume (Bv = 1), relu, skip on
  (f) ops.render_volume               the forward launch alone
  (q) cips_volume_render_bwd, quads   memset of dpacked + the kernel; the four lanes of a quad exchange their values so that every
                                      atomic instruction covers whole 16-byte nodes (flags bit 3 clear: what autograd runs)
  (l) cips_volume_render_bwd, lanes   the same with every lane adding its own four dwords per corner (flags bit 3 set)
  (a) forward + backward by autograd  ops.render_volume on a leaf and torch.autograd.grad: (f) + (q) + the allocations of the
                                      outputs, dpacked and the scratch records
  (s) evaluation.fit_volume           per step, 8 views: occupancy refresh, forward, pyramid loss, backward, fused Adam

The upstream gradients are seeded randn on all three outputs.  Atomic bytes: every live sample adds 8 nodes x 16 B; the live
samples are counted from the kernel's own records (x > 0 and fp32(T) > 0 under relu without last_back, which is the live rule
there), and bytes / time is set against the chip-wide rate of float atomic adds (1.3 TB/s: the figure this project budgets
atomics by).  The kernel also marches the ray forward once and writes and re-reads 16 B per sample, so bytes / time is a lower
bound of the rate the adds themselves run at.
Then, not timed: the kernel's error and its bar on every case of tests/volume_grad_oracle.py, and how far fit_volume lowers the
loss on the synthetic two-blob volume and on this generator.  Real initialiser weights (bench.G_CFG under seed 0), a seeded
latent.  The table goes to stdout and to --out."""
import argparse
import ctypes as C
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch

from bench import G_CFG
from bench_volume import FOV, L, PITCH, T0, T1, YAW, row, timed
from cips3d_amd import _lib, evaluation, ops
from cips3d_amd.generator import GeneratorNerfINR, _zc
from cips3d_amd.ops import _p, _stream

ATOMIC_RATE = 1.3e12          # bytes of float atomic adds per second, chip-wide


def backward_call(vol, cams, img, zg, ups, per_lane):
    """-> (fn, dpacked, scratch): one call of the entry point on preallocated buffers"""
    lib = _lib.load()
    d = vol.rgbs.device
    b, S = cams.shape[0], zg.shape[0]
    Bv, nx, ny, nz = vol.rgbs.shape[:4]
    xg, yg, _ = ops.pixel_grids(img, img, 2, 0., 1., d)
    lo, hi = (C.c_float * 3)(*vol.lo), (C.c_float * 3)(*vol.hi)
    dpacked = torch.empty_like(vol.rgbs)
    scratch = torch.empty(lib.cips_volume_render_bwd_scratch(b, img, img, S) // 4, device=d)
    flags = 4 | (8 if per_lane else 0)
    zc = _zc(FOV)

    def fn():
        _lib.check(lib.cips_volume_render_bwd(_p(vol.rgbs), _p(vol.occupancy), lo, hi, _p(xg), _p(yg), _p(zg), _p(cams), zc, 0, flags,
                                              _p(ups[0]), _p(ups[1]), _p(ups[2]), _p(dpacked), _p(scratch), b, Bv, nx, ny, nz, img,
                                              img, S, _stream()), "cips_volume_render_bwd")
    return fn, dpacked, scratch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=100., help="least device time of one timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("at least 5 timed repeats per leg")
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=d).to(d)
    G.device = d
    g = torch.Generator().manual_seed(1)
    zs = {"z_nerf": torch.randn(1, 256, generator=g).to(d), "z_inr": torch.randn(1, 512, generator=g).to(d)}
    img, S = a.img, a.steps
    n = img * img
    zc = _zc(FOV)
    zg = ops.pixel_grids(img, img, S, T0, T1, d)[2]
    views = {1: evaluation.orbit_cameras([YAW], [PITCH], device=d),
             8: evaluation.orbit_cameras([YAW + 0.1 * i for i in range(8)], [PITCH] * 8, device=d)}
    head = f"leg  {'what':<52} ms(median)    ms(min)    ms(max)"
    lines = [f"baked-volume backward: cube {L}, fov {FOV}, rays {T0}..{T1}, view {img} x {img}, S = {S} ({n * S} samples per view), relu, "
             f"skip on; {a.repeats} timed windows per leg of at least {a.window_ms:.0f} ms each (as many calls as fill it), after a "
             "warm-up, legs alternated", "MEASURED on the device this ran on; every figure below is a measurement unless it says otherwise",
             head]
    med = lambda ts: ts[len(ts) // 2]
    for N in a.resolutions:
        with torch.no_grad():
            vol = G.bake(zs, resolution=N, cube_length=L)
        for b, cams in views.items():
            gen = torch.Generator().manual_seed(5)
            ups = [torch.randn(b, c, img, img, generator=gen).to(d) for c in (3, 1, 1)]
            quad, dq, scratch = backward_call(vol, cams, img, zg, ups, False)
            lane, dl, _ = backward_call(vol, cams, img, zg, ups, True)
            fwd = lambda: ops.render_volume(vol.rgbs, vol.occupancy, vol.lo, vol.hi, cams, zc, img, img, zg=zg)
            leaf = vol.rgbs.clone().requires_grad_(True)

            def auto():
                out = ops.render_volume(leaf, vol.occupancy, vol.lo, vol.hi, cams, zc, img, img, zg=zg)
                torch.autograd.grad(out, leaf, ups)
            quad(); lane()
            torch.cuda.synchronize()
            rec = scratch.view(S, -1, 4)
            live = int(((rec[..., 3] > 0) & (rec[..., 1] > 0)).sum())
            diff = float((dq - dl).abs().max() / dq.abs().max())
            same_nodes = bool(torch.equal(dq != 0, dl != 0))
            touched = int((dq != 0).any(-1).sum())
            t, _ = timed([("f", fwd), ("q", quad), ("l", lane), ("a", auto)], a.repeats, a.window_ms)
            nbytes = live * 8 * 16
            what = f"N = {N}, {b} view{'s' if b > 1 else ''}"
            lines.append(row("f", f"render_volume forward, {what}", t["f"], f"{b * n * S / (med(t['f']) * 1e-3) / 1e9:.1f} Gsample/s"))
            for k, name in (("q", "quads (16-B segments)"), ("l", "lanes (dwords)")):
                rate = nbytes / (med(t[k]) * 1e-3)
                lines.append(row(k, f"backward, {name}, {what}", t[k],
                                 f"(.) / (f) = {med(t[k]) / med(t['f']):.2f}; {rate / 1e9:.0f} GB/s of atomic bytes = "
                                 f"{100 * rate / ATOMIC_RATE:.1f} % of the chip-wide rate"))
            lines.append(row("a", f"forward + backward by autograd, {what}", t["a"], f"(a) - (f) - (q) = {med(t['a']) - med(t['f']) - med(t['q']):.4f} ms"))
            lines.append(f"     {what}: {live} live samples of {b * n * S} ({100 * live / (b * n * S):.2f} %) add {nbytes / 1e6:.1f} MB into {touched} of "
                         f"{N ** 3} nodes ({live * 8 / max(touched, 1):.0f} adds per touched node and channel on average); scratch records "
                         f"{scratch.numel() * 4 / 1e6:.0f} MB; (l) / (q) = {med(t['l']) / med(t['q']):.2f}; the two shapes differ by "
                         f"{diff:.1e} of the largest gradient and touch {'the same' if same_nodes else 'DIFFERENT'} nodes")
            del quad, lane, dq, dl, scratch, rec, leaf
        with torch.no_grad():
            targets = ops.render_volume(vol.rgbs, vol.occupancy, vol.lo, vol.hi, views[8], zc, img, img, zg=zg)[0] * 0.5
        fit = lambda: evaluation.fit_volume(vol, targets, views[8], FOV, T0, T1, S, steps=10, lr=0.01)
        t, _ = timed([("s", fit)], 5, a.window_ms)
        lines.append(row("s", f"fit_volume, per step, N = {N}, 8 views", [v / 10 for v in t["s"]], "10 steps per call, set-up included"))
        del vol, targets

    # the yardstick's cases
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import volume_grad_oracle as go
    lines.append("against the fp64 yardstick (tests/volume_grad_oracle.py): max|g - g64| / max|g64| per channel group, its bar (8 x the fp32 "
                 "reference rule's own, floor 16 * 2^-24), and their ratio")
    worst = 0.
    for name in go.all_cases():
        ref = go.reference(name)
        case = ref.case
        packed, occ = ops.bake_volume(case.sigma.to(d), case.rgb.to(d))
        leaf = packed.clone().requires_grad_(True)
        out = ops.render_volume(leaf, occ, case.lo, case.hi, case.cam2world.to(d), case.zc, case.H, case.W, zg=case.zg.to(d),
                                clamp_mode=case.clamp_mode, last_back=case.last_back, white_back=case.white_back,
                                skip=case.clamp_mode == 'relu')
        gk, = torch.autograd.grad(out, leaf, [u.to(d) for u in ref.ups])
        m = go.measure(gk, ref.g64)
        worst = max(worst, m[0] / ref.bar[0], m[1] / ref.bar[1])
        lines.append(f"     {name:<34} sigma {m[0]:.3e} / {ref.bar[0]:.3e} = {m[0] / ref.bar[0]:.3f}   colour {m[1]:.3e} / {ref.bar[1]:.3e} = "
                     f"{m[1] / ref.bar[1]:.3f}")
    lines.append(f"     largest ratio {worst:.3f}")

    # fitting: how far the loss falls (tests/test_gpu_volume_grad.py asserts only that it falls)
    case = go.blob_case(False)
    packed, occ = ops.bake_volume(case.sigma[:1].to(d), case.rgb[:1].to(d))
    truth = SimpleNamespace(rgbs=packed, occupancy=occ, lo=case.lo, hi=case.hi, resolution=None)
    cams = evaluation.orbit_cameras([0.8, 1.5, 2.2, 2.9], [1.2, 1.6, 1.9, 1.4], device=d)
    targets = evaluation.render_volume(truth, cams, 16, 16, 0.8, 1.2, 12).imgs
    start = packed.clone()
    start[..., :3] = 0
    fit = evaluation.fit_volume(SimpleNamespace(**{**vars(truth), "rgbs": start}), targets, cams, 16, 0.8, 1.2, 12, steps=30, lr=0.05)
    lines.append("fit_volume, two-blob volume with its colours zeroed, 4 views of 16 x 16, S = 12, 30 steps, lr 0.05: loss last / first per "
                 "image  " + "  ".join(f"{float(v):.4f}" for v in (fit.losses[-1] / fit.losses[0]).cpu()))
    with torch.no_grad():
        vol = G.bake(zs, resolution=64, cube_length=L)
        yaws = [YAW - 0.3, YAW, YAW + 0.3]
        targets = torch.cat(evaluation.render_views(G, G.styles(zs), yaws, [PITCH] * 3, img_size=64, num_steps=24), 0).contiguous()
    fit = evaluation.fit_volume(vol, targets, evaluation.orbit_cameras(yaws, [PITCH] * 3, device=d), FOV, T0, T1, 24, steps=100, lr=0.02)
    lines.append("fit_volume, this generator baked at N = 64 ('aux' colours) fitted to forward_styles' pictures, 3 views of 64 x 64, "
                 "S = 24, 100 steps, lr 0.02: loss last / first per image  "
                 + "  ".join(f"{float(v):.4f}" for v in (fit.losses[-1] / fit.losses[0]).cpu())
                 + "  (first: " + "  ".join(f"{float(v):.3e}" for v in fit.losses[0].cpu()) + ")")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
