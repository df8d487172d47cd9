"""Point / camera gradient microbench, one process, device-event timings, legs alternated inside every repeat:

  1. cips_siren_bwd_points_x3 at B x P points (default 32 x 98 304: the headline step's samples), next to cips_siren_fwd_x3 and
     cips_siren_sigma_grad_x3 at the same shape
  2. cips_rays_bwd_cam at the same shape (r64, S = 24), against the bytes it has to read
  3. the G forward + backward of the headline geometry (r64, S = 24, flat, eager launches) through forward_camera_pos_and_lookup,
     with and without camera_pos / camera_lookup requiring grad

Real initialiser weights (bench.G_CFG under seed 0), random styles and upstream gradients.  The table goes to stdout and is
appended to --out (the file's other sections — the compiler's resource table, the two bench.py lines — are written by hand)."""
import argparse
import ctypes as C
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench import G_CFG, G_KW
from cips3d_amd import _lib, ops
from cips3d_amd.generator import GeneratorNerfINR

MAC = {"fwd": 128 * 3 + 128 * 128 + 128 + 64 * 128 + 32 * 64,            # 27 136
       "sigma_grad": 128 * 3 + 128 * 128 + 128 + 128 * 128 + 128 * 3,    # 33 664
       "bwd_points": 128 * 3 + 128 * 128 + 64 * 128 + 32 * 64 + 64 * 128 + 128 + 128 * 128 + 128 * 3}     # 52 096
BYTES = {"fwd": 12 + 132, "sigma_grad": 12 + 16, "bwd_points": 12 + 132 + 12, "rays_bwd_cam": 12 + 4}    # HBM bytes per point


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
    ap.add_argument("--steps", type=int, default=24, help="samples per ray")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("at least 5 timed repeats per leg")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    d = torch.device("cuda:0")
    lib = _lib.load()
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=d).to(d)
    G.device = d
    B, img, S = a.batch, a.img, a.steps
    n = img * img
    P = n * S
    st = ops._stream
    with torch.no_grad():
        style = {k: torch.randn(B, 128, device=d) for k in G.siren.style_dim_dict}
        t = ops._siren_prep(G.siren._siren_args(style))
    sw = ops._siren_struct(t)
    xg, yg, zg = ops.pixel_grids(img, img, S, 0.88, 1.12, d)
    zc = -1.0 / math.tan((2 * math.pi * 12 / 360) / 2)
    c2w = torch.eye(4, device=d).repeat(B, 1, 1)
    c2w[:, 2, 3] = 1.0
    jit = torch.rand(B, n, S, device=d)
    pts = ops.rays_fwd(xg, yg, zg, zc, c2w, jit, B, img, img, S)[0].view(B, P, 3)
    dfeat, dsig = torch.randn(B, P, 32, device=d), torch.randn(B, P, device=d)
    feat, sig, grad, dpts = (torch.empty(B, P, 32, device=d), torch.empty(B, P, device=d), torch.empty(B, P, 3, device=d),
                             torch.empty(B, P, 3, device=d))
    dcam = torch.empty(B, 4, 4, device=d)
    rp = ops._ray_params(xg, yg, zg, zc, c2w, jit, img, img, S)
    p_ = ops._p
    legs = [("fwd", lambda: _lib.check(lib.cips_siren_fwd_x3(C.byref(sw), p_(pts), p_(feat), p_(sig), B, P, st()), "fwd")),
            ("sigma_grad", lambda: _lib.check(lib.cips_siren_sigma_grad_x3(C.byref(sw), p_(pts), p_(sig), p_(grad), B, P, st()), "sg")),
            ("bwd_points", lambda: _lib.check(lib.cips_siren_bwd_points_x3(C.byref(sw), p_(pts), p_(dfeat), p_(dsig), p_(dpts), B, P,
                                                                           st()), "bp")),
            ("rays_bwd_cam", lambda: _lib.check(lib.cips_rays_bwd_cam(C.byref(rp), p_(dpts), p_(dcam), B, st()), "cam"))]
    times = _timed(legs, a.repeats)
    lines = [f"kernels at B = {B}, P = {P} (r{img}, S = {S}), trig_mode {ops.TRIG_MODE}, {a.repeats} timed repeats per leg after 2 warm-up "
             f"rounds, legs alternated",
             "leg            ms(median)  ms(min)  ms(max)  Gpoint/s  MAC/point  TMAC/s  HBM_B/point  TB/s"]
    for k, _ in legs:
        med, lo, hi = _median(times[k])
        rate = B * P / (med * 1e-3)
        mac = MAC.get(k, 0)
        lines.append(f"{k:<14} {med:10.3f}  {lo:7.3f}  {hi:7.3f}  {rate / 1e9:8.3f}  {mac:9d}  {rate * mac / 1e12:6.2f}  {BYTES[k]:11d}  "
                     f"{rate * BYTES[k] / 1e12:.3f}")
    med = {k: _median(times[k])[0] for k, _ in legs}
    lines.append(f"bwd_points / fwd = {med['bwd_points'] / med['fwd']:.2f}, bwd_points / sigma_grad = {med['bwd_points'] / med['sigma_grad']:.2f} "
                 f"(MAC ratios {MAC['bwd_points'] / MAC['fwd']:.2f}, {MAC['bwd_points'] / MAC['sigma_grad']:.2f}); rays_bwd_cam reads "
                 f"{B * P * BYTES['rays_bwd_cam'] / 1e6:.1f} MB with one workgroup per image ({B} workgroups)")

    # 3. the G step with and without the camera gradient (eager launches on both legs)
    G0 = torch.randn(B, 3, img, img, device=d) / (B * 3 * img * img)
    zs = G.get_zs(B)
    pos = torch.nn.functional.normalize(torch.randn(B, 3, device=d) * 0.2 + torch.tensor([0., 0., 1.], device=d), dim=-1)
    params = list(G.parameters())

    def step(cam_grad):
        def run():
            for p in params:
                p.grad = None
            c, l = pos.clone().requires_grad_(cam_grad), (-pos).clone().requires_grad_(cam_grad)
            imgs, _ = G.forward_camera_pos_and_lookup(zs, img_size=img, num_steps=S, hierarchical_sample=False, camera_pos=c,
                                                      camera_lookup=l, h_mean=math.pi / 2, v_mean=math.pi / 2, nerf_noise=0.,
                                                      **G_KW)
            imgs.backward(G0)
            assert (c.grad is not None) == cam_grad
        return run
    times = _timed([("G step", step(False)), ("G step + camera grad", step(True))], a.repeats)
    lines.append(f"G forward + backward, r{img}, S = {S}, batch {B}, explicit camera, eager launches, {a.repeats} timed repeats, alternated")
    for k, ts in times.items():
        m, lo, hi = _median(ts)
        lines.append(f"{k:<22} {m:8.3f} ms (min {lo:.3f}, max {hi:.3f})")
    m0, m1 = _median(times["G step"])[0], _median(times["G step + camera grad"])[0]
    lines.append(f"the camera gradient adds {m1 - m0:.3f} ms ({(m1 / m0 - 1) * 100:.1f} %) to the step")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
