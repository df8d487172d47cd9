"""View reprojection (ops.reproject: csrc/reproject.hip) against its composition from ATen operations, forward + backward,
on one GPU; the table goes to stdout and is appended to --out (profiles/reproject.txt).

Shapes (32, 3, 64, 64), the projection loop's batch, and (4, 3, 256, 256); depths around 1, a 0.3 rad baseline between two
cameras on the unit sphere, fov 12, occlusion test on.  Both legs compute out, the mask, d src and d tgt_depth of sum(out * g).
The ATen leg is what one would write without the kernel: fp32 elementwise operations for the geometry, F.grid_sample
(bilinear, align_corners=True) for the two samples, torch.where for the mask, autograd for the backward.  Its frame test has no
1/256 px slack and its borders are grid_sample's, so the two legs' outputs are compared on the pixels whose masks agree.

Timing: device events around --inner consecutive forward + backward calls (one event pair per call would time the enqueue of a
few tens of microseconds of work), --repeats such windows per leg after 3 warm-up windows, the legs alternated."""
import argparse
import math
import os
import socket
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from cips3d_amd import ops
from cips3d_amd.evaluation import relative_pose
from cips3d_amd.generator import _zc, camera_origin_from_angles, create_cam2world_matrix


def _stat(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def aten_reproject(src, tgt_depth, pose, zc, src_depth, occ_tol):
    B, C, Hs, Ws = src.shape
    Ht, Wt = tgt_depth.shape[2:]
    dev = src.device
    x = torch.linspace(-1, 1, Wt, device=dev).view(1, 1, 1, Wt).expand(1, 1, Ht, Wt)
    y = torch.linspace(1, -1, Ht, device=dev).view(1, 1, Ht, 1).expand(1, 1, Ht, Wt)
    d = torch.cat([x, y, torch.full_like(x, zc)], 1)
    d = d / d.norm(dim=1, keepdim=True)
    q = d * tgt_depth
    qp = torch.einsum("bij,bjhw->bihw", pose[:, :, :3], q) + pose[:, :, 3].view(B, 3, 1, 1)
    xs, ys = qp[:, 0] * zc / qp[:, 2], qp[:, 1] * zc / qp[:, 2]
    grid = torch.stack([xs, -ys], -1)
    inside = (tgt_depth[:, 0] > 0) & (qp[:, 2] * zc > 0) & (xs.abs() <= 1) & (ys.abs() <= 1)
    out = F.grid_sample(src, grid, mode="bilinear", padding_mode="border", align_corners=True)
    ds = F.grid_sample(src_depth, grid.detach(), mode="bilinear", padding_mode="border", align_corners=True)
    visible = inside & (qp.detach().norm(dim=1) <= ds[:, 0] + occ_tol)
    mask = torch.where(inside, torch.where(visible, 1, 2), 0).to(torch.uint8).unsqueeze(1)
    return torch.where(visible.unsqueeze(1), out, torch.zeros_like(out)), mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    dev = torch.device("cuda:0")
    zc = _zc(12)
    props = torch.cuda.get_device_properties(0)
    lines = [f"ops.reproject against its ATen composition (grid_sample based), forward + backward of sum(out * g), occlusion test on; device "
             f"events around {a.inner} consecutive calls, {a.repeats} windows per leg after 3 warm-up windows, legs alternated; "
             f"{props.name} ({props.gcnArchName}, {props.multi_processor_count} CUs) on host "
             f"{socket.gethostname()}, torch {torch.__version__}"]
    for (b, c, h, w) in ((32, 3, 64, 64), (4, 3, 256, 256)):
        g = torch.Generator().manual_seed(b)
        theta = (math.pi / 2 + torch.tensor([[-0.15], [0.15]])).repeat_interleave(b, 0)
        origin, _ = camera_origin_from_angles(theta, torch.full_like(theta, math.pi / 2))
        cams = create_cam2world_matrix(-origin, origin).to(dev)
        pose = relative_pose(cams[:b], cams[b:])
        yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
        src = torch.sin(9 * xx + 4 * yy + torch.randn(b, c, 1, 1, generator=g)).to(dev).requires_grad_(True)
        depth = (1 + 0.05 * torch.sin(5 * xx - 3 * yy + torch.randn(b, 1, 1, 1, generator=g))).to(dev).requires_grad_(True)
        src_depth = (1 + 0.05 * torch.cos(4 * xx + 2 * yy + torch.randn(b, 1, 1, 1, generator=g))).to(dev)
        gout = torch.randn(b, c, h, w, generator=g).to(dev)

        def own(g=gout):
            src.grad = depth.grad = None
            out, mask = ops.reproject(src, depth, pose, zc, src_depth=src_depth, occ_tol=0.01)
            out.backward(g)
            return out, mask

        def aten(g=gout):
            src.grad = depth.grad = None
            out, mask = aten_reproject(src, depth, pose, zc, src_depth, 0.01)
            out.backward(g)
            return out, mask
        legs = [("ops.reproject", own), ("ATen composition", aten)]
        times = {k: [] for k, _ in legs}
        for rep in range(a.repeats + 3):
            for k, fn in legs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    times[k].append(e0.elapsed_time(e1) / a.inner)
        # the outputs of the two legs, compared with the upstream gradient zeroed on the pixels whose masks differ (such a pixel
        # adds its whole gradient to four source pixels in one leg and nothing in the other)
        with torch.no_grad():
            m1 = ops.reproject(src, depth, pose, zc, src_depth=src_depth, occ_tol=0.01)[1]
            m2 = aten_reproject(src, depth, pose, zc, src_depth, 0.01)[1]
        agree = (m1 == m2)
        o1, _ = own(gout * agree)
        gs1, gd1 = src.grad.clone(), depth.grad.clone()
        o2, _ = aten(gout * agree)
        gs2, gd2 = src.grad.clone(), depth.grad.clone()
        both = (m1 == 1) & agree
        differ = int((~agree).sum())
        e_out = float(((o1 - o2).abs() * both).max())
        e_gd = float(((gd1 - gd2).abs() * both).max() / gd2.abs().max())
        e_gs = float((gs1 - gs2).abs().max() / gs2.abs().max())
        lines.append(f"  ({b}, {c}, {h}, {w}): coverage {float((m1 == 1).float().mean()):.3f}; masks differ on {differ} of {m1.numel()} pixels "
                     f"(the ATen frame test has no slack and decides in fp32); on the others out differs by at most {e_out:.2e}, "
                     f"d tgt_depth by {e_gd:.2e} of its maximum, d src by {e_gs:.2e} of its maximum")
        for k, t in times.items():
            m, lo, hi = _stat(t)
            lines.append(f"    {k:<18} {m * 1e3:8.1f} us per forward + backward (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
