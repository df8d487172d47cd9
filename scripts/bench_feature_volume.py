"""Feature-volume microbench: what a view of a baked FEATURE volume costs (ops.render_feature_volume's kernel and the head pass
evaluation.render_feature_volume adds), next to the rgb renderer on the volume of the same sigma and to
GeneratorNerfINR.forward_styles of the same image size and sample count, the path it replaces.  Device-event timings over
windows of at least --window-ms of calls, legs alternated inside every repeat of one process (scripts/bench_volume.py's scheme).

  per N (64, 128), image size (64, 256), views per call (1, 8), S (24, 48):
  (f) ops.render_feature_volume skip=True   sigma gathers where the brick is occupied, 8 x 8 16-byte feature gathers where w != 0
  (v) ops.render_volume skip=True           the rgb volume of the same sigma: eight 16-byte gathers per fetched sample
  per image size, views and S (the lattice does not enter):
  (h) the head pass alone                   G._head + G._images on the composited features
  (w) GeneratorNerfINR.forward_styles       same styles, image size and S, no hierarchical sampling, no noise
  per N: (b) GeneratorNerfINR.bake_features

Next to (f): the share of the samples whose features were fetched (w != 0, counted in torch from sigma at the kernel's own
sample points), and the time over the kernel's byte-count bar — fetched samples x 8 x 128 B plus S x 8 x 4 B per ray, over the
gather rate the MI355X microarchitecture notes give for a uniformly gathered table of that size (8.6 TB/s for 38 MB, the
34.6 MB volume of N = 64; 7.4 TB/s for 151 MB and beyond, used for the 277 MB volume of N = 128, which no longer fits the 256 MiB
last-level cache).  The bar counts every gathered byte as fetched from that level: neighbouring rays share cells, so a kernel can
beat it.  Not timed: the convergence of the baked image towards forward()'s as N grows, and the largest error over the fp64
yardstick's bar on the cases of tests/test_gpu_feature_volume.py.
Real initialiser weights (bench.G_CFG under seed 0), a seeded latent.  The table goes to stdout and to --out."""
import argparse
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import torch

from bench import G_CFG
from bench_volume import timed, row
from cips3d_amd import evaluation, ops
from cips3d_amd.generator import GeneratorNerfINR, _zc

FOV, T0, T1, L = 12, 0.88, 1.12, 0.3
YAW, PITCH = 1.2, 1.45
GATHER_TBS = {64: 8.6, 128: 7.4}


def fetched_share(vol, cams, img, S, d):
    """the share of all samples with w != 0 (relu, no back), from torch on the kernel's own sample points: the trilinear sigma
    by grid_sample would round differently, so sigma is interpolated by the kernel's nested lerps"""
    xg, yg, zg = ops.pixel_grids(img, img, S, T0, T1, d)
    b = cams.shape[0]
    pts = ops.rays_fwd(xg, yg, zg, _zc(FOV), cams, None, b, img, img, S)[0].reshape(b, -1, 3)
    n = torch.tensor(vol.sigma.shape[1:4], device=d)
    lo, hi = (torch.tensor(v, device=d) for v in (vol.lo, vol.hi))
    u = (pts - lo) * ((n - 1).float() / (hi - lo))
    inside = ((u >= 0) & (u <= (n - 1).float())).all(-1)
    cell = torch.minimum(u.clamp_min(0).long(), (n - 2).expand_as(u))
    t = u - cell.float()
    sig = vol.sigma[0]
    i, j, k = cell.unbind(-1)
    lerp = lambda p, q, w: p + w * (q - p)
    c = [[lerp(sig[i + di, j + dj, k], sig[i + di, j + dj, k + 1], t[..., 2]) for dj in (0, 1)] for di in (0, 1)]
    x = lerp(lerp(c[0][0], c[0][1], t[..., 1]), lerp(c[1][0], c[1][1], t[..., 1]), t[..., 0])
    x = torch.where(inside, x, torch.zeros_like(x)).view(b, img * img, S)
    delta = torch.cat([zg[1:] - zg[:-1], torch.full((1,), 1e10, device=d)])
    alpha = 1 - torch.exp(-delta * torch.relu(x))
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), (1 - alpha + 1e-10).double()], -1), -1)[..., :-1].float()
    return float(((alpha * T) != 0).float().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=40., help="least device time of one timed window")
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128])
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
    zc = _zc(FOV)
    med = lambda ts: ts[len(ts) // 2]
    head = f"leg  {'what':<52} ms(median)    ms(min)    ms(max)"
    lines = [f"baked feature volumes: cube {L}, fov {FOV}, rays {T0}..{T1}; {a.repeats} timed windows per leg of at least "
             f"{a.window_ms:.0f} ms each (as many calls as fill it), after a warm-up, legs alternated",
             "MEASURED on the device this ran on; every figure below is a measurement unless it says otherwise", head]
    cams = {1: evaluation.orbit_cameras([YAW], [PITCH], device=d),
            8: evaluation.orbit_cameras([YAW + 0.1 * i for i in range(8)], [PITCH] * 8, device=d)}
    shapes = [(img, views, S) for img in (64, 256) for views in (1, 8) for S in (24, 48)]
    with torch.no_grad():
        vols = {}
        for N in a.sizes:
            vols[N] = G.bake_features(zs, resolution=N, cube_length=L)
            t = timed([("b", lambda: G.bake_features(zs, resolution=N, cube_length=L))], a.repeats, a.window_ms)[0]
            lines.append(row("b", f"bake_features, N = {N} ({132 * N ** 3 / 1e6:.1f} MB)", t["b"]))
        styles = vols[a.sizes[0]].styles
        for img, views, S in shapes:
            what = f"{img}^2 x {views} view{'s' if views > 1 else ''}, S = {S}"
            cam = cams[views]
            zg = ops.pixel_grids(img, img, S, T0, T1, d)[2]
            rays = img * img * views
            legs, packed = [], {}
            for N in a.sizes:
                vol = vols[N]
                packed[N] = ops.bake_volume(vol.sigma, torch.zeros(1, N, N, N, 3, device=d))
                legs.append((f"f{N}", lambda vol=vol: ops.render_feature_volume(vol.sigma, vol.features, vol.occupancy, vol.lo, vol.hi,
                                                                              cam, zc, img, img, zg=zg)))
                legs.append((f"v{N}", lambda vol=vol, p=packed[N]: ops.render_volume(p[0], p[1], vol.lo, vol.hi, cam, zc, img, img,
                                                                                   zg=zg)))
            vol = vols[a.sizes[0]]
            fea = ops.render_feature_volume(vol.sigma, vol.features, vol.occupancy, vol.lo, vol.hi, cam, zc, img, img, zg=zg)[0]
            st = {k: v.expand(views, -1).contiguous() for k, v in styles.items()}
            flag = SimpleNamespace(return_aux_img=False)
            legs.append(("h", lambda: G._images(*G._head(flag, fea, st, False), views, img)[0].contiguous()))
            legs.append(("w", lambda: G.forward_styles(st, img, FOV, T0, T1, S, 0., 0., False, h_mean=YAW, v_mean=PITCH,
                                                       sample_dist='gaussian', nerf_noise=0.)))
            t = timed(legs, a.repeats, a.window_ms)[0]
            for N in a.sizes:
                share = fetched_share(vols[N], cam, img, S, d)
                bar_ms = (share * rays * S * 8 * 128 + rays * S * 8 * 4) / (GATHER_TBS.get(N, 7.4) * 1e12) * 1e3
                lines.append(row("f", f"render_feature_volume, N = {N}, {what}", t[f"f{N}"],
                                 f"features fetched for {100 * share:.1f} % of the samples; byte-count bar {bar_ms:.4f} ms at "
                                 f"{GATHER_TBS.get(N, 7.4)} TB/s: time / bar = {med(t[f'f{N}']) / bar_ms:.2f}"))
                lines.append(row("v", f"render_volume (rgb, same sigma), N = {N}, {what}", t[f"v{N}"],
                                 f"(f) / (v) = {med(t[f'f{N}']) / med(t[f'v{N}']):.2f}"))
            lines.append(row("h", f"the head pass alone, {what}", t["h"]))
            n0 = a.sizes[0]
            lines.append(row("w", f"forward_styles, {what}", t["w"],
                             f"(w) / ((f) + (h)) at N = {n0}: {med(t['w']) / (med(t[f'f{n0}']) + med(t['h'])):.1f}"))
            del fea, packed

        # convergence towards the network: forward()'s picture without noise, jitter or resampling, box holding every sample
        img, S, Lc = 64, 24, 0.5
        net = G.render_styles(styles, img, FOV, T0, T1, S, 0., 0., False, h_mean=YAW, v_mean=PITCH, sample_dist='gaussian',
                              nerf_noise=0., last_back=True, rand_override={"jitter": torch.full((1, img * img, S, 1), 0.5, device=d)})
        lines.append(f"convergence (mean |baked image - forward()'s image|, {img}^2, S = {S}, last_back, cube {Lc} holding every sample, "
                     "jitter zeroed):")
        prev = None
        for N in (24, 48, 96):
            vol = G.bake_features(zs, resolution=N, cube_length=Lc)
            out = evaluation.render_feature_volume(G, vol, net.cam2world, FOV, img, T0, T1, S, last_back=True)
            e = float((out.imgs - net.imgs).abs().mean())
            lines.append(f"     N = {N:<3} image {e:.3e}" + (f"   (previous / this = {prev / e:.2f})" if prev else ""))
            prev = e

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import feature_volume_oracle as fo
    worst = dict(fea=0., depth=0., opacity=0.)
    for name, case in fo.cases().items():
        sigma = case.sigma.to(d)
        planes, occ = ops.bake_feature_volume(sigma, case.feat.to(d))
        out = ops.render_feature_volume(sigma, planes, occ, case.lo, case.hi, case.cam2world.to(d), case.zc, case.H, case.W,
                                        zg=case.zg.to(d), clamp_mode=case.clamp_mode, last_back=case.last_back,
                                        white_back=case.white_back, skip=case.clamp_mode == 'relu')
        q = fo.compare(fo.reference(name), *out)
        for k in worst:
            worst[k] = max(worst[k], getattr(q, k))
    lines.append(f"against the fp64 yardstick (tests/feature_volume_oracle.py, {len(fo.cases())} cases): largest |err| / bar  "
                 f"fea {worst['fea']:.4f}  depth {worst['depth']:.4f}  opacity {worst['opacity']:.4f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
