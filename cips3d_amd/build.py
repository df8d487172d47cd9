"""Build libcips3d_hip.so (gfx950) in-tree with hipcc.  `python -m cips3d_amd.build`.

hipcc cross-compiles without a GPU.  The shared object is git-ignored but travels to the GPU
box with the gpurun snapshot."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "lib", "libcips3d_hip.so")
SOURCES = ["gemm_f32.hip", "gemm_bf16x3.hip", "gemm_bf16x3_wide.hip", "gemm_bf16x3_v3.hip", "gemm_bf16x3_km_wide.hip", "siren.hip", "siren_bwd_x3.hip", "siren_fwd_x3.hip", "siren_bwd_points_x3.hip", "siren_surface_x3.hip", "siren_color_x3.hip", "mesh.hip", "render.hip", "modfc.hip", "disc_ops.hip", "optim.hip", "fit_loss.hip", "reproject.hip", "raster.hip", "volume.hip", "small_ops.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "-Wno-unused-result"]
# per-source extras.  siren_bwd_x3.hip: the m-major layers of siren_bwd_x4_kernel unroll 32 items x (3 MFMAs + 3 epilogue slots);
# before unrolling every slot call carries all of its six variants, which puts the loop over clang's 16 384-instruction limit for
# `#pragma unroll` — it then stays a loop, the accumulator / activation arrays are indexed dynamically and live in scratch
# (1 728 bytes per lane, measured).  The limit is raised for this file only (the other sources' code generation is unchanged).
EXTRA_FLAGS = {"siren_bwd_x3.hip": ["-mllvm", "-pragma-unroll-threshold=1000000"]}
HIPCC_EXTRA = []      # scripts/probe/build_tuning.sh appends the probe-build define here; the product build passes nothing
LIBDIR = "lib"        # ... and points this at "lib_tuning": a probe build never overwrites the product's objects or library


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    out = os.path.join(HERE, LIBDIR, "libcips3d_hip.so")
    os.makedirs(os.path.join(HERE, LIBDIR), exist_ok=True)
    objdir = os.path.join(HERE, LIBDIR, "obj")
    os.makedirs(objdir, exist_ok=True)
    # objects of sources that are no longer listed (removed experiments) are deleted, not left beside the product
    keep = {src.replace(".hip", ".o") for src in SOURCES}
    for f in os.listdir(objdir):
        if f.endswith(".o") and f not in keep:
            os.remove(os.path.join(objdir, f))
    # every header and textually included fragment: a change to any of them rebuilds all sources
    headers = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".inc")))
    headers.append(os.path.join(HERE, "..", "include", "cips3d_hip.h"))
    objs = []
    procs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + headers):
            cmd = [HIPCC] + FLAGS + HIPCC_EXTRA + EXTRA_FLAGS.get(src, []) + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    if force or procs or _stale(out, objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(OUT)
