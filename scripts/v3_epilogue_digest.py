"""SHA-1 of everything the epilogue of gemm_bf16x3_v3_kernel writes — planes (hi, lo), gate bit plane, ToRGB partials and
finished ToRGB sums — for the five flavours of the training step (bench.py's gemm_roofline) at the shapes of
tests/test_gpu_gemm_v3_epilogue.py (N = 512; K = 512 and 64; B x M = 2 x 512 and 8 x 4608) and at the C2 shape, from fixed
seeds.  Two builds of the library that print the same lines compute the same bits:
    python scripts/v3_epilogue_digest.py [path/to/libcips3d_hip.so]"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cips3d_amd import _lib
if len(sys.argv) > 1:
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
from cips3d_amd import ops
d = torch.device("cuda:0")
ops.X3_KERNEL = 2          # the 256x256-tile kernels at every shape (the small ones would go to the 256x128 kernel)
N = 512


def sha(*ts):
    h = hashlib.sha1()
    for t in ts:
        h.update(t.cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()[:16]


for B, M, K in ((2, 512, 512), (2, 512, 64), (8, 4608, 512), (8, 4608, 64), (32, 4096, 512)):
    g = torch.Generator(device=d).manual_seed(B * 1000003 + M * 101 + K)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    xP, _ = ops.split_planes(rn(B, M, K), want_t=False); wP, _ = ops.split_planes(rn(B, N, K) * 0.04, want_t=False)
    rP, _ = ops.split_planes(rn(B, M, N), want_t=False)
    gate = (torch.rand(B, M, N // 8, device=d, generator=g) * 256).to(torch.uint8)
    pgate = (torch.rand(B, M, N // 8, device=d, generator=g) * 256).to(torch.uint8)
    rg, rw, T, tau = rn(B * M, 3), rn(3, N), rn(3, N), rn(3)
    sh = (xP, wP, M, N, K, K, K, B, M * K, N * K)
    for name in ("fwd", "fwd+torgb", "fwd+res+torgb", "dx", "dx+addp+rgb"):
        P = ops.Planes.empty(B, M, N, device=d); P.hi.zero_(); P.lo.zero_()
        mo = torch.zeros(B, M, N // 8, device=d, dtype=torch.uint8)
        part = torch.zeros(N // 128, B * M, 4, device=d); rgb = torch.zeros(B * M, 3, device=d)
        if name == "fwd":
            ops.gemm_x3(*sh, P=P, act=1, mask_out=mo, gate_bits=2)
        elif name.startswith("fwd"):
            res = rP if "res" in name else None
            ops.gemm_x3(*sh, P=P, act=1, res=res, mask_out=mo, gate_bits=2, torgb=(T, part))
            P2 = ops.Planes.empty(B, M, N, device=d)
            ops.gemm_x3_torgb(*sh, P2, T, tau, rgb, False, act=1, res=res, mask_out=torch.zeros_like(mo), gate_bits=2)
        elif name == "dx":
            ops.gemm_x3(*sh, P=P, mask=gate, gate_bits=1)
        else:
            ops.gemm_x3(*sh, P=P, addp=(rP, pgate), rgb_g=rg, rgb_w=rw, mask=gate, gate_bits=1)
        torch.cuda.synchronize()
        print(f"{B:2d} x {M:4d} x {N} x {K:3d}  {name:14s} planes {sha(P.hi, P.lo)}  gate bits {sha(mo)}  "
              f"torgb partials {sha(part)}  torgb sums {sha(rgb)}", flush=True)
