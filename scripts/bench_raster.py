"""Mesh-rasterisation microbench: one N = 256 GeneratorNerfINR.extract_mesh of a random generator (auxiliary colours) seen from
B cameras at S x S pixels, device-event timings, legs alternated inside every repeat of one process:

  (raster)   ops.rasterize            scratch and output allocation, the memset of the keys, the vertex, face, large-triangle and
                                      resolve kernels
  (render)   evaluation.render_mesh   (raster) and three interpolations (points, normals, colours) with their torch glue
  (surface)  G.surface                the ray cast of the same level set at the same image size, B images, 24 steps, refine 8,
                                      normals included: what a view costs without a mesh
  (extract)  G.extract_mesh           the extraction itself (sigma lattice, marching tetrahedra, normals, colours), once per shape

and, for the workgroup path, two synthetic legs at 1024^2: 64 full-frame triangles stacked in depth, listed back to front and
front to back (--layers 0 leaves them out, as the traced runs do).  Processed in sequence the first order would issue 64 atomics
per pixel and the second one; the layers of one launch run side by side, so the legs measure the path's fragment rate, not the
rate of the 64-bit atomicMin.

The split of (raster) into its launches comes from a run of its own under the kernel tracer:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_raster.py --sizes 1024 --cameras 1 --layers 0
  python scripts/bench_raster.py --kernel-stats DIR --label "S=1024 B=1" --out profiles/raster.txt      (appends)

Bytes are algorithmic (what a launch has to move once: V vertices, T triangles, P = B S^2 pixels, h the hit pixels): memset 8 P;
vertex B (12 V + 16 V); face B (12 T + 48 T) + 16 h (one key read and one atomic per winning fragment at least); resolve
P (8 + 21) + 60 h; interpolation of C channels P (16 + 4 C) + h (12 + 12 C).  No time is a pass / fail bar: the file records
the numbers."""
import argparse
import csv
import glob
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.3e12


def merge_kernel_stats(directory, label, out):
    """append the rasteriser's rows of a rocprofv3 --kernel-trace --stats run to `out`"""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    lines = [f"kernel times of a traced run ({label}; rocprofv3 --kernel-trace --stats, a run of its own):",
             "  kernel                      calls   avg_us    min_us    max_us"]
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            if "raster_" in name or "siren_surface" in name or "fillBuffer" in name:
                short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0][:26]
                lo, hi = (f"{float(row[k]) / 1e3:8.1f}" if row.get(k) else "     n/a" for k in ("MinNs", "MaxNs"))
                lines.append(f"  {short:<26} {int(row['Calls']):6d} {float(row['AverageNs']) / 1e3:8.1f}  {lo}  {hi}")
    text = "\n".join(lines)
    print(text)
    with open(out, "a") as fh:
        fh.write(text + "\n")


def timed(legs, repeats):
    import torch
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
    return {k: sorted(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--cameras", default="1,8")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-stats", default=None, metavar="DIR", help="append the kernel rows of a traced run to --out and exit")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.kernel_stats:
        return merge_kernel_stats(a.kernel_stats, a.label, a.out)
    if a.repeats < 7:
        raise SystemExit("at least 7 timed repeats per leg")
    import torch

    from bench import G_CFG
    from cips3d_amd import evaluation, ops
    from cips3d_amd.generator import GeneratorNerfINR, _zc
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=d).to(d)
    G.device = d
    G.eval()
    FOV, KW = 12, dict(fov=12, ray_start=0.88, ray_end=1.12, num_steps=24, h_stddev=0., v_stddev=0., sample_dist='gaussian')
    zs = G.get_zs(1)
    level = float(G.density_grid(zs, resolution=64).median())
    extract = lambda: G.extract_mesh(zs, level, resolution=a.n, colors='aux')
    mesh = extract()[0]
    V, T = mesh.vertices.shape[0], mesh.faces.shape[0]
    lines = [f"mesh rasterisation: one extract_mesh at N={a.n} of a random generator at its median density (V={V} T={T}), "
             f"{a.repeats} timed repeats per leg after 2 warm-up rounds, legs alternated; device events around whole calls",
             f"rates against {HBM / 1e12:.1f} TB/s (achievable HBM)",
             "S     B   leg       ms(median)  ms(min)  ms(max)   note"]
    ts = timed([("extract", extract)], a.repeats)["extract"]
    t_extract = ts[len(ts) // 2]
    lines.append(f"-     1   extract  {t_extract:10.3f}  {ts[0]:7.3f}  {ts[-1]:7.3f}   G.extract_mesh(colors='aux'), once per shape")
    for S in (int(v) for v in a.sizes.split(",")):
        for B in (int(v) for v in a.cameras.split(",")):
            cams = evaluation.orbit_cameras([math.pi / 2 + 0.5 * (i - (B - 1) / 2) / max(B - 1, 1) for i in range(B)], device=d)
            w2c = evaluation.world2cam(cams)
            zsB = {k: v.expand(B, -1).contiguous() for k, v in zs.items()}
            legs = [("raster", lambda: ops.rasterize(mesh.vertices, mesh.faces, w2c, _zc(FOV), S, S)),
                    ("render", lambda: evaluation.render_mesh(mesh, cams, FOV, S)),
                    ("surface", lambda: G.surface(zsB, level, img_size=S, **KW))]
            times = timed(legs, a.repeats)
            out = evaluation.render_mesh(mesh, cams, FOV, S)
            # the agreement line: rays that start outside the lattice's cube (half diagonal 0.26), at the timed leg's spacing
            sf = G.surface(zsB, level, img_size=S, h_mean=math.pi / 2, **dict(KW, ray_start=0.7, ray_end=1.3, num_steps=61))
            front = evaluation.render_mesh(mesh, sf.cam2world, FOV, S, far=1.3)
            h, P = int(out.mask.sum()), B * S * S
            both = (sf.mask == 1) & (front.mask == 1)
            agree = float(((sf.mask != 0) == (front.mask == 1)).float().mean())
            cell = 0.3 / (a.n - 1)
            med_dd = float(((sf.depth - front.depth)[both].abs() / cell).median()) if both.any() else float('nan')
            # ... and where the ray cast's crossing lies inside the lattice's cube: the untrained field has density outside it too
            inside = (sf.mask == 1) & (sf.points.abs().amax(1, keepdim=True) <= 0.15)
            in_hit = float((front.mask == 1)[inside].float().mean()) if inside.any() else float('nan')
            in_dd = ((sf.depth - front.depth)[inside & both].abs() / cell)
            in_med, in_p90 = (float(in_dd.median()), float(in_dd.float().quantile(0.9)) if in_dd.numel() < 2 ** 24 else float('nan')) \
                if in_dd.numel() else (float('nan'), float('nan'))
            nb = {"memset": 8 * P, "vertex": B * 28 * V, "face": B * 60 * T + 16 * h, "resolve": 29 * P + 60 * h,
                  "interp C=3": 28 * P + 48 * h}
            med = {k: v[len(v) // 2] for k, v in times.items()}
            for k, _ in legs:
                v = times[k]
                note = ""
                if k == "render":
                    gain = med["surface"] - med["render"]
                    note = (f"surface / render = {med['surface'] / med['render']:.1f}; extraction repaid after "
                            f"{t_extract / gain * B:.1f} views" if gain > 0 else "surface is cheaper: never repaid")
                if k == "raster":
                    note = f"{h} of {P} pixels hit ({h / P:.3f})"
                lines.append(f"{S:<5} {B:<3} {k:<8} {med[k]:10.3f}  {v[0]:7.3f}  {v[-1]:7.3f}   {note}".rstrip())
            for k, n in nb.items():
                lines.append(f"{S:<5} {B:<3} kernel:{k:<11} algorithmic MB {n / 1e6:8.1f} = {n / HBM * 1e6:7.1f} us at the HBM rate")
            lines.append(f"{S:<5} {B:<3} render_mesh against G.surface, frontal camera: masks agree on {100 * agree:.2f} % of the pixels, median "
                         f"|depth difference| {med_dd:.3f} lattice cells over {int(both.sum())} pixels; of the {int(inside.sum())} pixels whose "
                         f"crossing lies inside the lattice's cube the mesh is hit at {100 * in_hit:.2f} %, median |depth difference| "
                         f"{in_med:.3f} cells (90th percentile {in_p90:.3f})")
            del out, sf, front
            torch.cuda.empty_cache()
    if a.layers > 0:
        lines += layer_legs(a, d, FOV)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


def layer_legs(a, d, FOV):
    """the workgroup path and the early-out: stacked full-frame triangles, listed back to front and front to back"""
    import torch

    from cips3d_amd import evaluation, ops
    from cips3d_amd.generator import _zc
    lines = []
    S, Lr = 1024, a.layers
    zdepth = torch.linspace(-0.1, 0.1, Lr, device=d)                                   # world z: the camera sits at z = +1
    tri = torch.tensor([[-3.0, -2.5, 0.], [3.2, -2.4, 0.], [0.1, 4.0, 0.]], device=d)
    verts = (tri.view(1, 3, 3) + torch.stack([torch.zeros_like(zdepth)] * 2 + [zdepth], -1).view(Lr, 1, 3)).reshape(-1, 3).contiguous()
    faces_b2f = torch.arange(3 * Lr, dtype=torch.int32, device=d).view(Lr, 3)          # layer 0 is the farthest
    faces_f2b = faces_b2f.flip(0).contiguous()
    w2c = evaluation.world2cam(evaluation.orbit_cameras([math.pi / 2], device=d))
    legs = [("b2f", lambda: ops.rasterize(verts, faces_b2f, w2c, _zc(FOV), S, S)),
            ("f2b", lambda: ops.rasterize(verts, faces_f2b, w2c, _zc(FOV), S, S))]
    times = timed(legs, a.repeats)
    r1, r2 = ops.rasterize(verts, faces_b2f, w2c, _zc(FOV), S, S), ops.rasterize(verts, faces_f2b, w2c, _zc(FOV), S, S)
    assert bool((r1[3] == 1).all()) and torch.equal(r1[2], r2[2]) and bool((r1[0] == Lr - 1).all()) and bool((r2[0] == 0).all())
    med = {k: v[len(v) // 2] for k, v in times.items()}
    frags = Lr * S * S
    for k, v in times.items():
        lines.append(f"{S:<5} 1   {k:<8} {med[k]:10.3f}  {v[0]:7.3f}  {v[-1]:7.3f}   {Lr} full-frame triangles, {frags} fragments")
    lines.append(f"workgroup path: b2f {frags / med['b2f'] / 1e6:.1f} G fragments/s, f2b {frags / med['f2b'] / 1e6:.1f} (whole calls).  The layers of "
                 f"one launch run side by side, so the list order decides little about which fragments find a nearer key already there: "
                 f"this does not isolate the rate of the 64-bit atomicMin (between {S * S} and {frags} were issued)")
    return lines


if __name__ == "__main__":
    main()
