"""Baked-volume camera-gradient microbench: what the gradient of a view with respect to cam2world costs
(cips_volume_render_bwd_cam), next to the forward and to the node backward of the same view.  Device-event timings over windows
of at least --window-ms of calls, legs alternated inside every repeat of one process (scripts/bench_volume.py's scheme):

  per N (default 128 and 256), img x img, S samples per ray, 1 camera and a turntable of 8 over the one volume (Bv = 1), relu,
  skip on
  (f) ops.render_volume                the forward launch alone
  (n) cips_volume_render_bwd           the node backward: memset of dpacked + the kernel (quads: what autograd runs)
  (c) cips_volume_render_bwd_cam       the camera backward: the kernel + the finish launch, no memset, no atomics
  (b) (n) then (c)                     what autograd launches when both the nodes and the cameras ask
  (s) evaluation.fit_cameras           per step, 8 views: cameras from the angles, forward, pyramid loss, backward, fused Adam

The upstream gradients are seeded randn on all three outputs.  The live samples are counted from the kernel's own records
(x > 0 and fp32(T) > 0 under relu without last_back, which is the live rule there): only they gather their eight corners again.
Then, not timed: the kernel's error and its bar on every case of tests/volume_cam_grad_oracle.py, and where fit_cameras ends on
the two-blob volume.  Real initialiser weights (bench.G_CFG under seed 0), a seeded latent.  The table goes to stdout and to
--out."""
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
from bench_volume_backward import backward_call
from cips3d_amd import _lib, evaluation, ops
from cips3d_amd.generator import GeneratorNerfINR, _zc
from cips3d_amd.ops import _p, _stream


def camera_call(vol, cams, H, W, zg, ups, zc, clamp=0, flags=4):
    """-> (fn, dcam, scratch): one call of the entry point on preallocated buffers"""
    lib = _lib.load()
    d = vol.rgbs.device
    b, S = cams.shape[0], zg.shape[0]
    Bv, nx, ny, nz = vol.rgbs.shape[:4]
    xg, yg, _ = ops.pixel_grids(W, H, 2, 0., 1., d)
    lo, hi = (C.c_float * 3)(*vol.lo), (C.c_float * 3)(*vol.hi)
    dcam = torch.empty(b, 4, 4, device=d)
    scratch = torch.empty(lib.cips_volume_render_bwd_cam_scratch(b, H, W, S) // 4, device=d)

    def fn():
        _lib.check(lib.cips_volume_render_bwd_cam(_p(vol.rgbs), _p(vol.occupancy), lo, hi, _p(xg), _p(yg), _p(zg), _p(cams), zc, clamp,
                                                  flags, _p(ups[0]), _p(ups[1]), _p(ups[2]), _p(dcam), _p(scratch), b, Bv, nx, ny,
                                                  nz, H, W, S, _stream()), "cips_volume_render_bwd_cam")
    return fn, dcam, scratch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
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
    yaws8 = [YAW + 0.1 * i for i in range(8)]
    views = {1: evaluation.orbit_cameras([YAW], [PITCH], device=d), 8: evaluation.orbit_cameras(yaws8, [PITCH] * 8, device=d)}
    head = f"leg  {'what':<52} ms(median)    ms(min)    ms(max)"
    lines = [f"baked-volume camera gradient: cube {L}, fov {FOV}, rays {T0}..{T1}, view {img} x {img}, S = {S} ({n * S} samples per view), "
             f"relu, skip on; {a.repeats} timed windows per leg of at least {a.window_ms:.0f} ms each (as many calls as fill it), after a "
             "warm-up, legs alternated; the spread is the min and max column",
             "MEASURED on the device this ran on; every figure below is a measurement unless it says otherwise",
             "the slope of the interpolant is formed by gathering the eight corners again in the reverse pass, live samples only (the "
             "16-byte record is the node backward's); storing two 3-vectors per sample in the forward march was not built", head]
    med = lambda ts: ts[len(ts) // 2]
    for N in a.resolutions:
        with torch.no_grad():
            vol = G.bake(zs, resolution=N, cube_length=L)
        for b, cams in views.items():
            gen = torch.Generator().manual_seed(5)
            ups = [torch.randn(b, c, img, img, generator=gen).to(d) for c in (3, 1, 1)]
            node, dq, _ = backward_call(vol, cams, img, zg, ups, False)
            cam, dc, scratch = camera_call(vol, cams, img, img, zg, ups, zc)
            fwd = lambda: ops.render_volume(vol.rgbs, vol.occupancy, vol.lo, vol.hi, cams, zc, img, img, zg=zg)

            def both():
                node(); cam()
            cam()
            torch.cuda.synchronize()
            first = dc.clone()
            rec = scratch[:_lib.load().cips_volume_render_bwd_scratch(b, img, img, S) // 4].view(S, -1, 4)     # the partials follow
            live = int(((rec[..., 3] > 0) & (rec[..., 1] > 0)).sum())
            t, _ = timed([("f", fwd), ("n", node), ("c", cam), ("b", both)], a.repeats, a.window_ms)
            same = bool(torch.equal(first, dc))
            what = f"N = {N}, {b} view{'s' if b > 1 else ''}"
            lines.append(row("f", f"render_volume forward, {what}", t["f"], f"{b * n * S / (med(t['f']) * 1e-3) / 1e9:.1f} Gsample/s"))
            lines.append(row("n", f"node backward, {what}", t["n"], f"(n) / (f) = {med(t['n']) / med(t['f']):.2f}"))
            lines.append(row("c", f"camera backward, {what}", t["c"],
                             f"(c) / (f) = {med(t['c']) / med(t['f']):.2f}; (c) / (n) = {med(t['c']) / med(t['n']):.2f}"))
            lines.append(row("b", f"both backwards, {what}", t["b"], f"(b) - (n) - (c) = {med(t['b']) - med(t['n']) - med(t['c']):.4f} ms"))
            lines.append(f"     {what}: {live} live samples of {b * n * S} ({100 * live / (b * n * S):.2f} %) gather their corners again; scratch "
                         f"{scratch.numel() * 4 / 1e6:.0f} MB; max|dcam| {float(dc.abs().max()):.3e}; every timed call gave "
                         f"{'the same bits as the first' if same else 'DIFFERENT bits'}")
            del node, cam, dq, dc, scratch, rec
        with torch.no_grad():
            targets = ops.render_volume(vol.rgbs, vol.occupancy, vol.lo, vol.hi, views[8], zc, img, img, zg=zg)[0]
        fit = lambda: evaluation.fit_cameras(vol, targets, FOV, T0, T1, S, yaws=[y + 0.02 for y in yaws8], pitches=[PITCH + 0.02] * 8,
                                             steps=10, lr=0.002)
        t, _ = timed([("s", fit)], 5, a.window_ms)
        lines.append(row("s", f"fit_cameras, per step, N = {N}, 8 views", [v / 10 for v in t["s"]], "10 steps per call, set-up included"))
        del vol, targets

    # the yardstick's cases
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import volume_cam_grad_oracle as co
    import volume_grad_oracle as go
    lines.append("against the fp64 yardstick (tests/volume_cam_grad_oracle.py): per camera max|g - g64| / max|g64| over the 3 x 4 block, its bar "
                 "(8 x the fp32 reference rule's own, floor 16 * 2^-24), and their ratio")
    worst = 0.
    for name in co.all_cases():
        ref = co.reference(name)
        case = ref.case
        packed, occ = ops.bake_volume(case.sigma.to(d), case.rgb.to(d))
        vol = SimpleNamespace(rgbs=packed, occupancy=occ, lo=case.lo, hi=case.hi)
        relu = case.clamp_mode == 'relu'
        flags = (1 if case.last_back else 0) | (2 if case.white_back else 0) | (4 if relu else 0)
        fn, dc, _ = camera_call(vol, case.cam2world.to(d), case.H, case.W, case.zg.to(d), [u.to(d) for u in ref.ups], case.zc,
                                0 if relu else 1, flags)
        fn()
        m = co.measure(dc, ref.g64)
        worst = max([worst] + [x / y for x, y in zip(m, ref.bar)])
        lines.append(f"     {name:<36} " + "   ".join(f"{x:.3e} / {y:.3e} = {x / y:.3f}" for x, y in zip(m, ref.bar)))
    lines.append(f"     largest ratio {worst:.3f}")

    # fitting: where the angles end (tests/test_gpu_volume_cam_grad.py asserts only that loss and errors fall)
    case = go.blob_case(False)
    packed, occ = ops.bake_volume(case.sigma.to(d), case.rgb.to(d))
    vol = SimpleNamespace(rgbs=packed, occupancy=occ, lo=case.lo, hi=case.hi, resolution=None)
    ty, tp = [0.8, 2.2], [1.2, 1.9]
    targets = evaluation.render_volume(vol, evaluation.orbit_cameras(ty, tp, device=d), 16, 16, 0.8, 1.2, 12).imgs
    fit = evaluation.fit_cameras(vol, targets, 16, 0.8, 1.2, 12, yaws=[y - 0.1 for y in ty], pitches=[p + 0.1 for p in tp], steps=30, lr=0.01)
    lines.append("fit_cameras, the two-blob volumes, 2 views of 16 x 16, S = 12, start 0.1 rad off (yaw - 0.1, pitch + 0.1), 30 steps, lr 0.01: "
                 "loss first -> last per view  " + "  ".join(f"{float(x):.3e} -> {float(y):.3e}" for x, y in zip(fit.losses[0].cpu(), fit.losses[-1].cpu()))
                 + ";  |yaw error|  " + "  ".join(f"{abs(float(x) - y):.4f}" for x, y in zip(fit.yaws.cpu(), ty))
                 + ";  |pitch error|  " + "  ".join(f"{abs(float(x) - y):.4f}" for x, y in zip(fit.pitches.cpu(), tp)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
