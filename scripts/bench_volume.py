"""Baked-volume microbench: what a volume costs to build (GeneratorNerfINR.bake: color_grid(return_sigma=True) + ops.bake_volume)
and what a view of it costs (evaluation.render_volume's kernel), next to GeneratorNerfINR.render of the same camera and sample
count.  Device-event timings over windows of at least --window-ms of calls, legs alternated inside every repeat of one process:

  bake, N = 128 and 256, one image
  (g) color_grid(return_sigma=True)   the network on N^3 points: the part of bake that is not new
  (p) ops.bake_volume                 pack (16 B in, 16 B out per node) + brick maxima (4 B in per node, re-read at brick faces)
  view, img x img, S samples per ray, one camera (three-quarter), per N
  (s) ops.render_volume skip=True     one 4-byte occupancy read per inside sample, eight 16-byte gathers where occ > 0
  (n) ops.render_volume skip=False    eight 16-byte gathers per inside sample
  (t) / (u) a turntable of 8 cameras over the one volume in one call, skip=True / skip=False, per view: a single 256^2 view is
      65 536 rays — one wave per SIMD of the chip — and its call is bound by the launch and the host, not by the kernel
  (r) GeneratorNerfINR.render         same camera, same S, no hierarchical sampling: the NeRF path and the INR head per frame

Not timed, for the record: the share of samples the skip does not fetch (on these synthetic weights); how far the baked image is
from compositing the network's own density and 'aux' colour at the very same sample points (zeroed outside the box, as the
baked volume is) at N = 64, 128, 256 — the discretisation error of the lattice, a measurement, not an assertion; and the largest
error over the fp64 yardstick's bar on the cases of tests/test_gpu_volume.py.
Real initialiser weights (bench.G_CFG under seed 0), a seeded latent.  The table goes to stdout and to --out."""
import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bench import G_CFG
from cips3d_amd import evaluation, ops
from cips3d_amd.generator import GeneratorNerfINR, _zc

FOV, T0, T1, L = 12, 0.88, 1.12, 0.3
YAW, PITCH = 1.2, 1.45


def timed(legs, repeats, window_ms):
    """Two warm-up rounds of every leg, then the timed ones, alternated.  Every timed window holds as many calls as fill
    window_ms, sized per leg from a 10-call probe after its warm-up: a window of one sub-millisecond call measures the clock."""
    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls
    inner = {}
    for k, fn in legs:
        window(fn, 2)
        inner[k] = max(1, int(math.ceil(window_ms / max(window(fn, 10), 1e-4))))
    times = {k: [] for k, _ in legs}
    for rep in range(repeats):
        for k, fn in legs:
            times[k].append(window(fn, inner[k]))
    return {k: sorted(v) for k, v in times.items()}, inner


def row(k, what, ts, extra=""):
    return f"({k})  {what:<52} {ts[len(ts) // 2]:10.4f}  {ts[0]:9.4f}  {ts[-1]:9.4f}  {extra}"


def sample_points(cam, img, S, d):
    """the sample points of the view as cips_rays_fwd materialises them -> (1, n*S, 3), and zg"""
    xg, yg, zg = ops.pixel_grids(img, img, S, T0, T1, d)
    pts = ops.rays_fwd(xg, yg, zg, _zc(FOV), cam, None, 1, img, img, S)[0]
    return pts.reshape(1, img * img * S, 3).contiguous(), zg


def inside_and_brick(pts, vol):
    n = torch.tensor(vol.rgbs.shape[1:4], device=pts.device)
    lo, hi = (torch.tensor(v, device=pts.device) for v in (vol.lo, vol.hi))
    u = (pts[0] - lo) * ((n - 1).float() / (hi - lo))
    inside = ((u >= 0) & (u <= (n - 1).float())).all(-1)
    cell = torch.minimum(u.clamp_min(0).long(), (n - 2).expand_as(u))
    brick = cell >> 3
    occ = vol.occupancy[0][brick[:, 0].clamp_max(vol.occupancy.shape[1] - 1), brick[:, 1].clamp_max(vol.occupancy.shape[2] - 1),
                           brick[:, 2].clamp_max(vol.occupancy.shape[3] - 1)]
    return inside, occ


def composite(sigma, rgb, zg):
    """oracle/cips3d_oracle.py::integrate in fp64, relu, no noise, no back: sigma (n,S), rgb (n,S,3) -> rgb, depth, opacity"""
    sigma, rgb, z = sigma.double(), rgb.double(), zg.double()
    delta = torch.cat([z[1:] - z[:-1], torch.full((1,), 1e10, dtype=torch.float64, device=z.device)])
    alpha = 1 - torch.exp(-delta * torch.relu(sigma))
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1 - alpha + 1e-10], 1), 1)[:, :-1]
    w = alpha * T
    return (w.unsqueeze(-1) * rgb).sum(1), (w * z).sum(1), w.sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--img", type=int, default=256)
    ap.add_argument("--steps", type=int, default=48)
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
    cam = evaluation.orbit_cameras([YAW], [PITCH], device=d)
    cams8 = evaluation.orbit_cameras([YAW + 0.1 * i for i in range(8)], [PITCH] * 8, device=d)
    zc = _zc(FOV)
    head = f"leg  {'what':<52} ms(median)    ms(min)    ms(max)"
    lines = [f"baked volumes: cube {L}, fov {FOV}, rays {T0}..{T1}, view {img} x {img}, S = {S} ({n * S} samples per view); "
             f"{a.repeats} timed windows per leg of at least {a.window_ms:.0f} ms each (as many calls as fill it), after a warm-up, legs alternated",
             "MEASURED on the device this ran on; every figure below is a measurement unless it says otherwise", head]
    volumes = {}
    with torch.no_grad():
        for N in (128, 256):
            rgb, sigma = G.color_grid(zs, resolution=N, cube_length=L, return_sigma=True)
            t = timed([("g", lambda: G.color_grid(zs, resolution=N, cube_length=L, return_sigma=True)),
                       ("p", lambda: ops.bake_volume(sigma, rgb))], a.repeats, a.window_ms)[0]
            nodes = N ** 3
            lines.append(row("g", f"color_grid(return_sigma=True), N = {N}", t["g"]))
            lines.append(row("p", f"ops.bake_volume, N = {N}", t["p"],
                             f"{36 * nodes / (t['p'][len(t['p']) // 2] * 1e-3) / 1e9:.0f} GB/s of the 36 B per node it must move"))
            del rgb, sigma
            volumes[N] = G.bake(zs, resolution=N, cube_length=L)
        volumes[64] = G.bake(zs, resolution=64, cube_length=L)

        ref = G.render(zs, img, FOV, T0, T1, S, 0., 0., False, h_mean=YAW, v_mean=PITCH, sample_dist='gaussian')
        lines.append(f"     the camera is render()'s own cam2world for yaw {YAW}, pitch {PITCH}; orbit_cameras of the same angles differs "
                     f"from it by at most {float((ref.cam2world - cam).abs().max()):.1e}")
        cam = ref.cam2world.contiguous()
        pts, zg = sample_points(cam, img, S, d)
        for N in (128, 256):
            vol = volumes[N]
            rv = lambda cams, skip: ops.render_volume(vol.rgbs, vol.occupancy, vol.lo, vol.hi, cams, zc, img, img, zg=zg, skip=skip)
            on, off = rv(cam, True), rv(cam, False)
            same = all(torch.equal(x, y) for x, y in zip(on, off))
            legs = [("s", lambda: rv(cam, True)), ("n", lambda: rv(cam, False)), ("t", lambda: rv(cams8, True)),
                    ("u", lambda: rv(cams8, False))]
            if N == 128:
                legs.append(("r", lambda: G.render(zs, img, FOV, T0, T1, S, 0., 0., False, h_mean=YAW, v_mean=PITCH,
                                                   sample_dist='gaussian')))
            t, inner = timed(legs, a.repeats, a.window_ms)
            inside, occ = inside_and_brick(pts, vol)
            n_in = int(inside.sum())
            skipped = int((inside & (occ <= 0)).sum())
            med = lambda k: t[k][len(t[k]) // 2]
            fetched = n_in - skipped
            lines.append(row("s", f"render_volume skip=True, N = {N}", t["s"],
                             f"{n * S / (med('s') * 1e-3) / 1e9:.2f} Gsample/s; {128 * fetched / (med('s') * 1e-3) / 1e9:.0f} GB/s of 128-B gathers, cache hits included"))
            lines.append(row("n", f"render_volume skip=False, N = {N}", t["n"],
                             f"{n * S / (med('n') * 1e-3) / 1e9:.2f} Gsample/s; {128 * n_in / (med('n') * 1e-3) / 1e9:.0f} GB/s of 128-B gathers, cache hits included"))
            lines.append(row("t", f"8 views in one call, skip=True, per view, N = {N}", [v / 8 for v in t["t"]],
                             f"{n * S / (med('t') / 8 * 1e-3) / 1e9:.1f} Gsample/s"))
            lines.append(row("u", f"8 views in one call, skip=False, per view, N = {N}", [v / 8 for v in t["u"]],
                             f"{n * S / (med('u') / 8 * 1e-3) / 1e9:.1f} Gsample/s; (u) / (t) = {med('u') / med('t'):.2f}"))
            if "r" in t:
                lines.append(row("r", "GeneratorNerfINR.render, same camera and S", t["r"],
                                 f"(r) / (s) = {med('r') / med('s'):.1f}"))
            lines.append(f"     N = {N}: {100 * n_in / (n * S):.1f} % of the samples lie inside the box; the skip leaves out {skipped} of them "
                         f"({100 * skipped / max(n_in, 1):.1f} % of the inside samples, {100 * float((vol.occupancy <= 0).float().mean()):.1f} % "
                         f"of the bricks have occ <= 0); skip on / off give {'equal' if same else 'DIFFERENT'} bits; "
                         f"(n) - (s) = {med('n') - med('s'):.4f} ms, min-max spread of (s) {t['s'][-1] - t['s'][0]:.4f} ms")

        # discretisation: the network at the same sample points, zeroed outside the box, composited in fp64
        lines.append("discretisation error of the lattice (baked view against the network composited at the same sample points, relu, "
                     "no back; max / mean |difference| over the pixels; the last delta is 1e10, so a pixel whose last sample has a sigma "
                     "of another sign on the lattice than in the network differs by its whole remaining transmittance: that is the max):")
        style = G._nerf_styles(G._density_styles(zs['z_nerf'], 1.0))
        sig_net = G.siren.density(pts, style)
        rgb_net = G.point_colors(zs, pts)
        for N in (64, 128, 256):
            vol = volumes[N]
            inside, _ = inside_and_brick(pts, vol)
            want = composite(torch.where(inside, sig_net[0], torch.zeros_like(sig_net[0])).view(n, S),
                             (rgb_net[0] * inside.unsqueeze(-1)).view(n, S, 3), zg)
            got = ops.render_volume(vol.rgbs, vol.occupancy, vol.lo, vol.hi, cam, zc, img, img, zg=zg)
            dr = (got[0][0].permute(1, 2, 0).reshape(n, 3).double() - want[0]).abs()
            dd = (got[1].reshape(n).double() - want[1]).abs()
            do = (got[2].reshape(n).double() - want[2]).abs()
            lines.append(f"     N = {N:<4} rgb {float(dr.max()):.3e} / {float(dr.mean()):.3e}   depth {float(dd.max()):.3e} / {float(dd.mean()):.3e}   "
                         f"opacity {float(do.max()):.3e} / {float(do.mean()):.3e}   (opacity of the network's view: mean {float(want[2].mean()):.3f})")
        del pts, sig_net, rgb_net

    # the yardstick's cases: largest error over the bar per output
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import volume_oracle as vo
    worst = dict(rgb=0., depth=0., opacity=0.)
    for name, case in vo.cases().items():
        packed, occ = ops.bake_volume(case.sigma.to(d), case.rgb.to(d))
        out = ops.render_volume(packed, occ, case.lo, case.hi, case.cam2world.to(d), case.zc, case.H, case.W, zg=case.zg.to(d),
                                clamp_mode=case.clamp_mode, last_back=case.last_back, white_back=case.white_back,
                                skip=case.clamp_mode == 'relu')
        q = vo.compare(vo.reference(name), *out)
        for k in worst:
            worst[k] = max(worst[k], getattr(q, k))
    lines.append(f"against the fp64 yardstick (tests/volume_oracle.py, {len(vo.cases())} cases): largest |err| / bar  rgb {worst['rgb']:.4f}  "
                 f"depth {worst['depth']:.4f}  opacity {worst['opacity']:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
