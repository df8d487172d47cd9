"""Mesh-extraction microbench: ops.mesh_from_volume's launches on an N^3 density volume (GeneratorNerfINR.extract_mesh's path),
device-event timings, legs alternated inside every repeat of one process:

  (count)  cips_mesh_count           the count kernel and the scan of its per-workgroup totals (two launches)
  (emit)   cips_mesh_emit            the vertex kernel and the face kernel (two launches) into preallocated outputs
  (e2e)    ops.mesh_from_volume      scratch and output allocation, count, the host read of the totals, emit
  (sigma)  cips_siren_sigma_x3_grid  the sigma lattice kernel that made the volume: the cost extraction is added to

on two volumes: an analytic sphere (0.1 - |x| on the lattice, level 0) and the seeded generator's own volume at its median sigma.
The split of (count) and (emit) into their kernels comes from a run of its own under the kernel tracer:

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_mesh.py --batches 1 --volumes sphere --repeats 7
  python scripts/bench_mesh.py --kernel-stats DIR --label "B=1 sphere" --out profiles/mesh_extraction.txt      (appends)

Bytes are algorithmic (what each launch has to move once, P points, V vertices, T triangles, W workgroups per image):
count 4 P + 8 W, scan 16 W, vertices 4 P + 5 P + 12 V, faces 4 P + 5 P + 12 T; the rate is set against the 6.3 TB/s a streaming
kernel reaches from HBM (a 64 MB volume also fits the 256 MB Infinity Cache, so a leg may read faster than that).
No time is a pass / fail bar: the file records the numbers."""
import argparse
import csv
import ctypes as C
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 6.3e12
RUN = 1024            # lattice points per workgroup (csrc/mesh.hip MESH_RUN)


def leg_bytes(P, V, T, B):
    W = -(-P // RUN)
    return {"count": B * (4 * P + 8 * W) + 16 * B * W, "emit": B * 18 * P + 12 * (V + T),
            "kernel:count": B * (4 * P + 8 * W), "kernel:scan": 16 * B * W, "kernel:verts": B * 9 * P + 12 * V,
            "kernel:faces": B * 9 * P + 12 * T}


def merge_kernel_stats(directory, label, out):
    """append the mesh kernels' rows of a rocprofv3 --kernel-trace --stats run to `out`"""
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    lines = [f"kernel times of a traced run ({label}; rocprofv3 --kernel-trace --stats, a run of its own):",
             "  kernel                      calls   avg_us    min_us    max_us"]
    for f in files:
        for row in csv.DictReader(open(f)):
            name = row.get("Name", "")
            if "mesh_" in name or "siren_sigma_x3_kernel" in name:
                short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0][:26]
                lo, hi = (f"{float(row[k]) / 1e3:8.1f}" if row.get(k) else "     n/a" for k in ("MinNs", "MaxNs"))
                lines.append(f"  {short:<26} {int(row['Calls']):6d} {float(row['AverageNs']) / 1e3:8.1f}  {lo}  {hi}")
    text = "\n".join(lines)
    print(text)
    with open(out, "a") as fh:
        fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--volumes", default="sphere,generator")
    ap.add_argument("--repeats", type=int, default=7)
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
    from cips3d_amd import _lib, ops
    from cips3d_amd._lib import GridParams
    from cips3d_amd.evaluation import density_lattice
    from cips3d_amd.generator import GeneratorNerfINR
    d = torch.device("cuda:0")
    lib = _lib.load()
    torch.manual_seed(0)
    G = GeneratorNerfINR(**G_CFG, device=d).to(d)
    G.device = d
    N = a.n
    P = N ** 3
    gx, gy, gz = (g.to(d) for g in density_lattice(N, 0.3, (0., 0., 0.)))
    gp = GridParams(ops._p(gx), ops._p(gy), ops._p(gz), N, N, N)
    st = ops._stream
    lines = [f"mesh extraction on a density lattice N={N} ({P} points per image), {a.repeats} timed repeats per leg after 2 warm-up "
             f"rounds, legs alternated; device events", f"rates against {HBM / 1e12:.1f} TB/s (achievable HBM)",
             "volume     B   leg      ms(median)  ms(min)  ms(max)   MB(algorithmic)  TB/s   of_HBM"]
    for B in (int(v) for v in a.batches.split(",")):
        zs = G.get_zs(B)
        with torch.no_grad():
            styles = G._nerf_styles(G._density_styles(zs['z_nerf'], 1.0))
            t = ops._siren_prep(G.siren._siren_args(G.siren._sigma_args(styles)))
        sw = ops._siren_struct(t)
        gen_vol = torch.empty(B, N, N, N, device=d)

        def leg_sigma():
            _lib.check(lib.cips_siren_sigma_x3_grid(C.byref(sw), C.byref(gp), ops._p(gen_vol), B, st()), "sigma_x3_grid")

        leg_sigma()
        for kind in a.volumes.split(","):
            if kind == "sphere":
                r = (gx.view(N, 1, 1) ** 2 + gy.view(1, N, 1) ** 2 + gz.view(1, 1, N) ** 2).sqrt()
                vol, level = (0.1 - r).expand(B, N, N, N).contiguous(), 0.0
            else:
                vol, level = gen_vol.clone(), float(gen_vol.median())
            meshes = ops.mesh_from_volume(vol, gx, gy, gz, level)
            V, T = sum(m[0].shape[0] for m in meshes), sum(m[1].shape[0] for m in meshes)
            nbytes = lib.cips_mesh_scratch_bytes(C.byref(gp), B)
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=d)
            totals = torch.empty(B, 2, dtype=torch.int64, device=d)
            verts = torch.empty(V, 3, device=d)
            faces = torch.empty(T, 3, dtype=torch.int32, device=d)

            def leg_count():
                _lib.check(lib.cips_mesh_count(C.byref(gp), ops._p(vol), level, B, ops._p(scratch), nbytes, ops._p(totals), st()), "mesh_count")

            def leg_emit():
                _lib.check(lib.cips_mesh_emit(C.byref(gp), ops._p(vol), level, B, ops._p(scratch), nbytes, ops._p(totals), ops._p(verts),
                                              ops._p(faces), st()), "mesh_emit")

            def leg_e2e():
                ops.mesh_from_volume(vol, gx, gy, gz, level)

            legs = [("count", leg_count), ("emit", leg_emit), ("e2e", leg_e2e), ("sigma", leg_sigma)]
            times = {k: [] for k, _ in legs}
            for rep in range(a.repeats + 2):
                for k, fn in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if rep >= 2:
                        times[k].append(e0.elapsed_time(e1))
            # the timed outputs are the mesh the end-to-end call returns
            assert torch.equal(torch.cat([m[0] for m in meshes]).view(torch.int32), verts.view(torch.int32))
            assert torch.equal(torch.cat([m[1] for m in meshes]), faces)
            nb = leg_bytes(P, V, T, B)
            nb["e2e"] = nb["count"] + nb["emit"]
            lines.append(f"{kind:<10} {B:<3} V={V} T={T} ({V / B / P:.4f} vertices and {T / B / P:.4f} triangles per lattice point)")
            for k, _ in legs:
                ts = sorted(times[k])
                med = ts[len(ts) // 2]
                rate = f"{nb[k] / 1e6:15.1f}  {nb[k] / (med * 1e-3) / 1e12:5.2f}  {nb[k] / (med * 1e-3) / HBM:6.2f}" if k in nb else ""
                lines.append(f"{kind:<10} {B:<3} {k:<8} {med:10.3f}  {ts[0]:7.3f}  {ts[-1]:7.3f}  {rate}".rstrip())
            for k in ("kernel:count", "kernel:scan", "kernel:verts", "kernel:faces"):
                lines.append(f"{kind:<10} {B:<3} {k:<13} algorithmic MB {nb[k] / 1e6:.1f} = {nb[k] / HBM * 1e6:.1f} us at the HBM rate")
            del vol, scratch, verts, faces, meshes
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
