"""The fp64 yardstick of the view reprojection (csrc/reproject.hip, ops.reproject): the definition of include/cips3d_hip.h,
step by step, in fp64 torch on the fp32 inputs as given, with
  * the per-pixel decision margins (how far u and v are from the frame tests, ds + occ_tol - rho', how far u and v are from
    the nearest integer): a pixel inside a margin may be decided otherwise by a correct fp32 or fp64 implementation, and the
    GPU tests leave it out of their value comparisons;
  * the gradients, from fp64 autograd with the mask held fixed;
  * the quantities the tests' error bars are made of (the cell's largest neighbour difference, du/ddepth, the number and the
    absolute sum of the contributions to every source pixel).
tests/test_reproject_oracle_cpu.py holds this module to an analytic scene, to central differences and to the 2 % cap on the
share of pixels inside a margin for every input set the GPU tests use (`cases()`, built here so that both see the same)."""
import math
from types import SimpleNamespace

import torch

SLACK = 1.0 / 256.0
FRAME_MARGIN, OCC_MARGIN, INT_MARGIN = 1e-2, 2e-4, 1e-3
EPS32 = 2.0 ** -24


def zc_of(fov):
    """generator._zc in fp64, rounded to fp32 as the product hands it to the kernel"""
    return float(torch.tensor(-1.0 / math.tan(math.radians(fov) / 2), dtype=torch.float64).float())


def uv_bar(zc_src, Hs, Ws):
    """sixteen roundings on quantities of size max(1, |zc_src|) * max(Ws, Hs) / 2 px"""
    return 16 * EPS32 * max(1.0, abs(zc_src)) * max(Ws, Hs) / 2


def ray_dirs(H, W, zc):
    """the camera of csrc/raygen.h: (3, H, W) fp64 unit directions, pixel (row i, col j) at x = -1 + 2j/(W-1), y = 1 - 2i/(H-1)"""
    x = -1 + 2 * torch.arange(W, dtype=torch.float64) / (W - 1)
    y = 1 - 2 * torch.arange(H, dtype=torch.float64) / (H - 1)
    d = torch.stack([x.view(1, W).expand(H, W), y.view(H, 1).expand(H, W), torch.full((H, W), float(zc), dtype=torch.float64)])
    return d / d.norm(dim=0, keepdim=True)


def _gather(img, off):
    B, C = img.shape[:2]
    return img.flatten(2).gather(2, off.view(B, 1, -1).expand(B, C, -1)).view(B, C, *off.shape[1:])


def _corners(img, off, Ws):
    return _gather(img, off), _gather(img, off + 1), _gather(img, off + Ws), _gather(img, off + Ws + 1)


def _bilinear(c, fu, fv):
    s00, s01, s10, s11 = c
    return (s00 * (1 - fu) + s01 * fu) * (1 - fv) + (s10 * (1 - fu) + s11 * fu) * fv


def reproject64(src, tgt_depth, tgt2src, zc_tgt, zc_src=None, src_depth=None, occ_tol=None, dout=None):
    """-> SimpleNamespace of fp64 CPU tensors:
      out (B,C,Ht,Wt), mask (B,1,Ht,Wt) uint8, uv (B,2,Ht,Wt)                      the definition's outputs
      m_frame, m_occ, m_int (B,1,Ht,Wt)   the margins (inf where a test does not apply)
      near, near_grad (B,1,Ht,Wt) bool    inside a value margin / inside that or the integer margin
      lip (B,1,Ht,Wt)                     the largest difference of two neighbours in the sampled cell, over the channels
    and with dout (B,C,Ht,Wt):
      d_src (B,C,Hs,Ws), d_tgt_depth (B,1,Ht,Wt)      fp64 autograd of sum(out * dout) with the mask held fixed
      dudt, dvdt (B,1,Ht,Wt)                          du/ddepth, dv/ddepth (autograd), zero where mask != 1 or clamped
      dudt_abs, dvdt_abs (B,1,Ht,Wt)                  the same with the two terms of the numerator taken absolutely
      n (B,1,Hs,Ws), s_abs, s_dout (B,C,Hs,Ws)        per source pixel: contributions, sum |weight * dout|, sum |dout|"""
    zc_src = zc_tgt if zc_src is None else zc_src
    src64 = src.detach().cpu().double().requires_grad_(dout is not None)
    t_in = tgt_depth.detach().cpu().double()
    M = tgt2src.detach().cpu().double()
    B, C, Hs, Ws = src64.shape
    Ht, Wt = t_in.shape[2:]
    valid = torch.isfinite(t_in) & (t_in > 0)
    # an invalid depth is replaced before the arithmetic (its pixel is decided by `valid`): no NaN reaches autograd
    t = torch.where(valid, t_in, torch.ones_like(t_in)).requires_grad_(dout is not None)
    d = ray_dirs(Ht, Wt, zc_tgt)
    q = d.unsqueeze(0) * t                                                              # 1.
    qp = torch.einsum("bij,bjhw->bihw", M[:, :, :3], q) + M[:, :, 3].view(B, 3, 1, 1)    # 2.
    front = (qp[:, 2:3] * zc_src > 0).detach()
    qz = torch.where(front, qp[:, 2:3], torch.ones_like(qp[:, 2:3]))
    xs, ys = qp[:, 0:1] * zc_src / qz, qp[:, 1:2] * zc_src / qz                          # 3.
    u, v = (xs + 1) / 2 * (Ws - 1), (1 - ys) / 2 * (Hs - 1)                              # 4.
    ud, vd = u.detach(), v.detach()
    in_frame = valid & front & (ud >= -SLACK) & (ud <= Ws - 1 + SLACK) & (vd >= -SLACK) & (vd <= Hs - 1 + SLACK)   # 5.
    u = torch.where(in_frame, u, torch.zeros_like(u)).clamp(0, Ws - 1)
    v = torch.where(in_frame, v, torch.zeros_like(v)).clamp(0, Hs - 1)
    u0 = u.detach().floor().long().clamp(max=Ws - 2)                                     # 6.
    v0 = v.detach().floor().long().clamp(max=Hs - 2)
    off = (v0 * Ws + u0).view(B, Ht, Wt)
    fu, fv = u - u0, v - v0
    corners = _corners(src64, off, Ws)
    sample = _bilinear(corners, fu, fv)
    inf = torch.full_like(ud, float("inf"))
    m_occ = inf
    mask = in_frame.to(torch.uint8)
    if src_depth is not None:                                                            # 7.
        sd = src_depth.detach().cpu().double()
        ds = _bilinear(_corners(sd, off, Ws), fu.detach(), fv.detach())
        rho = qp.detach().norm(dim=1, keepdim=True)
        visible = rho <= ds + occ_tol
        mask = torch.where(in_frame, torch.where(visible, 1, 2), 0).to(torch.uint8)
        m_occ = torch.where(in_frame, (ds + occ_tol - rho).abs(), inf)
        m_occ = torch.where(torch.isnan(m_occ), inf, m_occ)                              # a NaN in ds decides firmly: occluded
    out = torch.where(mask == 1, sample, torch.zeros_like(sample))
    nan = torch.full_like(ud, float("nan"))
    uv = torch.cat([torch.where(mask != 0, u.detach(), nan), torch.where(mask != 0, v.detach(), nan)], 1)
    r = SimpleNamespace(out=out.detach(), mask=mask, uv=uv)
    could = valid & front                                    # the frame tests are reached
    m_frame = torch.minimum(torch.minimum((ud + SLACK).abs(), (ud - (Ws - 1 + SLACK)).abs()),
                            torch.minimum((vd + SLACK).abs(), (vd - (Hs - 1 + SLACK)).abs()))
    r.m_frame = torch.where(could, m_frame, inf)
    r.m_occ = m_occ
    uc, vc = u.detach(), v.detach()
    r.m_int = torch.where(mask == 1, torch.minimum((uc - uc.round()).abs(), (vc - vc.round()).abs()), inf)
    r.near = (r.m_frame < FRAME_MARGIN) | (r.m_occ < OCC_MARGIN)
    r.near_grad = r.near | (r.m_int < INT_MARGIN)
    s00, s01, s10, s11 = (c.detach() for c in corners)
    r.lip = torch.stack([(s01 - s00).abs(), (s11 - s10).abs(), (s10 - s00).abs(), (s11 - s01).abs()]).amax(0).amax(1, keepdim=True)
    if dout is None:
        return r
    g = dout.detach().cpu().double()
    r.d_src, r.d_tgt_depth = torch.autograd.grad((out * g).sum(), (src64, t), retain_graph=True)
    vis = (mask == 1)
    r.dudt, = torch.autograd.grad(torch.where(vis, u, torch.zeros_like(u)).sum(), t, retain_graph=True)
    r.dvdt, = torch.autograd.grad(torch.where(vis, v, torch.zeros_like(v)).sum(), t)
    # the two terms of (e_x q'_z - q'_x e_z), absolutely: what an fp32 evaluation of du/ddepth loses to their cancellation
    e = torch.einsum("bij,jhw->bihw", M[:, :, :3], d)
    qpd, qzd = qp.detach(), qz.detach()
    r.dudt_abs = (Ws - 1) / 2 * abs(zc_src) * ((e[:, 0:1] * qzd).abs() + (qpd[:, 0:1] * e[:, 2:3]).abs()) / qzd ** 2 * vis
    r.dvdt_abs = (Hs - 1) / 2 * abs(zc_src) * ((e[:, 1:2] * qzd).abs() + (qpd[:, 1:2] * e[:, 2:3]).abs()) / qzd ** 2 * vis
    fu, fv = fu.detach(), fv.detach()
    n = torch.zeros(B, 1, Hs * Ws, dtype=torch.float64)
    s_abs = torch.zeros(B, C, Hs * Ws, dtype=torch.float64)
    s_dout = torch.zeros(B, C, Hs * Ws, dtype=torch.float64)
    gv = (g * vis).flatten(2)
    for k, w in enumerate(((1 - fu) * (1 - fv), fu * (1 - fv), (1 - fu) * fv, fu * fv)):
        idx = (off + (0, 1, Ws, Ws + 1)[k]).view(B, 1, -1)
        n.scatter_add_(2, idx, vis.flatten(2).double())
        s_abs.scatter_add_(2, idx.expand(B, C, -1), (w.flatten(2) * gv).abs())
        s_dout.scatter_add_(2, idx.expand(B, C, -1), gv.abs())
    r.n, r.s_abs, r.s_dout = n.view(B, 1, Hs, Ws), s_abs.view(B, C, Hs, Ws), s_dout.view(B, C, Hs, Ws)
    return r


# ------------------------------------------------------------------------------------------
# an analytic scene: a textured plane z = -0.1, with or without a sphere of radius 0.1 about the origin, rendered in fp64
# ------------------------------------------------------------------------------------------
PLANE_Z, SPHERE_R = -0.1, 0.1


def texture(p):
    """a smooth function of the world point (..., 3) -> (..., 3) colours"""
    x, y, z = p.unbind(-1)
    return torch.stack([torch.sin(9 * x) * torch.cos(7 * y), torch.cos(5 * x + 3 * y) + 2 * z, torch.sin(4 * y - 6 * x + 11 * z)], -1)


def cameras(yaws, pitches=None):
    """cam2world (b,4,4) of cameras on the unit sphere looking at the origin, built with the generator's own helpers"""
    from cips3d_amd.generator import camera_origin_from_angles, create_cam2world_matrix
    theta = torch.tensor(yaws, dtype=torch.float32).view(-1, 1)
    phi = torch.full_like(theta, math.pi / 2) if pitches is None else torch.tensor(pitches, dtype=torch.float32).view(-1, 1)
    origin, _ = camera_origin_from_angles(theta, phi)
    return create_cam2world_matrix(-origin, origin)


def render_scene(cam2world, H, W, zc, sphere):
    """-> imgs (b,3,H,W), depth (b,1,H,W) fp32 (computed in fp64, rounded once), points (b,H,W,3) fp64: for every pixel the
    first hit of its ray with the sphere (if any) or the plane; depth is the distance along the normalised ray"""
    c = cam2world.double()
    R, o = c[:, :3, :3], c[:, :3, 3]
    d = torch.einsum("bij,jhw->bhwi", R, ray_dirs(H, W, zc))
    ob = o.view(-1, 1, 1, 3)
    t = (PLANE_Z - ob[..., 2]) / d[..., 2]
    if sphere:
        bq = (ob * d).sum(-1)
        disc = bq * bq - ((ob * ob).sum(-1) - SPHERE_R ** 2)
        ts = -bq - disc.clamp_min(0).sqrt()
        t = torch.where((disc > 0) & (ts > 0) & (ts < t), ts, t)
    p = ob + d * t.unsqueeze(-1)
    return texture(p).permute(0, 3, 1, 2).float().contiguous(), t.unsqueeze(1).float().contiguous(), p


def relative_pose64(tgt_c2w, src_c2w):
    """[R_s^T R_t | R_s^T (t_t - t_s)] in fp64 -> (b,3,4) fp32: evaluation.relative_pose's definition, written here on its own"""
    t, s = tgt_c2w.double(), src_c2w.double()
    RsT = s[:, :3, :3].transpose(1, 2)
    return torch.cat([RsT @ t[:, :3, :3], RsT @ (t[:, :3, 3:] - s[:, :3, 3:])], 2).float()


FOV = 12
_H = math.pi / 2
# (yaw A, yaw B, pitch A, pitch B): about yaw pi/2 +- 0.15.  Not the mirror pair at one pitch: two cameras that see the plane
# under the same angle map it at nearly the same scale, B's sampling positions then drift off A's pixel centres linearly from
# the image centre, and the bilinear error at 32 and 64 px is still in the regime where it falls like h (2.6x, measured), not h^2.
PAIRS = ((_H - 0.15, _H + 0.15, _H - 0.10, _H + 0.08), (_H + 0.15, _H - 0.15, _H + 0.12, _H - 0.07), (_H - 0.05, _H + 0.25, _H, _H))


def scene_pair(pair, size, sphere):
    """views A (target) and B (source) of the scene from the cameras of `pair` -> SimpleNamespace(a_img, a_depth, a_pts, b_img,
    b_depth, pose (1,3,4) fp32 A -> B, zc)"""
    zc = zc_of(FOV)
    cams = cameras(list(pair[:2]), list(pair[2:]))
    img, depth, pts = render_scene(cams, size, size, zc, sphere)
    return SimpleNamespace(a_img=img[:1], a_depth=depth[:1], a_pts=pts[:1], b_img=img[1:], b_depth=depth[1:],
                           pose=relative_pose64(cams[:1], cams[1:]), zc=zc, cams=cams)


# ------------------------------------------------------------------------------------------
# the input sets of tests/test_gpu_reproject.py
# ------------------------------------------------------------------------------------------
def _rigid(g, angle, shift):
    """a random rotation by `angle` rad about a random axis and a random translation of norm `shift` -> (3,4) fp32"""
    ax = torch.randn(3, generator=g, dtype=torch.float64)
    ax = ax / ax.norm()
    K = torch.tensor([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]], dtype=torch.float64)
    R = torch.eye(3, dtype=torch.float64) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K
    tr = torch.randn(3, 1, generator=g, dtype=torch.float64)
    return torch.cat([R, tr / tr.norm() * shift], 1).float()


def _smooth(g, B, C, H, W, lo=0.0, amp=1.0):
    """a smooth random image: a few random plane waves per channel"""
    y, x = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64), indexing="ij")
    k = torch.randn(B, C, 3, 3, generator=g, dtype=torch.float64) * 4
    img = sum(torch.sin(k[:, :, i, 0, None, None] * x + k[:, :, i, 1, None, None] * y + k[:, :, i, 2, None, None]) for i in range(3))
    return (lo + amp * img / 3).float()


def random_case(seed, B, C, Hs, Ws, Ht, Wt, with_depth, fov=FOV, angle=0.02, shift=0.02, bad_pixels=False, back=0.0):
    """a generic input set: smooth random images and depths around 1, a small random rigid motion per image; `back` moves the
    source camera that far backwards, which shrinks the target's frame inside the source's (a 2 x 2 image has all its pixels
    on the frame's corners: without it every one of them sits on a frame test)"""
    g = torch.Generator().manual_seed(seed)
    zc = zc_of(fov)
    c = SimpleNamespace(src=_smooth(g, B, C, Hs, Ws), tgt_depth=_smooth(g, B, 1, Ht, Wt, 1.0, 0.05),
                        pose=torch.stack([_rigid(g, angle, shift) for _ in range(B)]), zc_tgt=zc, zc_src=zc, src_depth=None, occ_tol=None)
    c.pose[:, 2, 3] -= back
    if with_depth:
        c.src_depth = _smooth(g, B, 1, Hs, Ws, 1.0 + back, 0.05)
        c.occ_tol = 0.01
    if bad_pixels:
        flat = c.tgt_depth.view(B, -1)
        flat[0, 1], flat[0, Wt + 1], flat[-1, 2], flat[-1, 3] = float("inf"), 0.0, float("nan"), -1.0
    return c


def scene_case(pair, size, sphere, with_depth=True):
    s = scene_pair(pair, size, sphere)
    return SimpleNamespace(src=s.b_img, tgt_depth=s.a_depth, pose=s.pose, zc_tgt=s.zc, zc_src=s.zc,
                           src_depth=s.b_depth if with_depth else None, occ_tol=2e-3 if with_depth else None)


def behind_case():
    """a wide target camera (fov 110, the source's is 60) and a source camera turned about a quarter turn about the y axis: in
    both images part of the target's frame lies behind the source camera, part in front of it outside its frame, part inside"""
    c = random_case(77, 2, 3, 16, 16, 16, 16, True, fov=60)
    c.zc_tgt = zc_of(110)
    for b, (ang, tr) in enumerate(((1.45, (0.8, 0.0, -0.6)), (1.7, (0.5, 0.0, -0.3)))):
        R = torch.tensor([[math.cos(ang), 0, math.sin(ang)], [0, 1, 0], [-math.sin(ang), 0, math.cos(ang)]])
        c.pose[b] = torch.cat([R, torch.tensor(tr).view(3, 1)], 1)
    return c


def cases():
    """name -> input set, every one the GPU tests run"""
    out = {
        "2x2_on_2x2": random_case(1, 1, 3, 2, 2, 2, 2, False, back=0.3),
        "2x2_on_2x2_depth": random_case(2, 1, 1, 2, 2, 2, 2, True, back=0.3),
        "5x7_on_6x9_c1": random_case(3, 2, 1, 6, 9, 5, 7, False, back=0.3),
        "5x7_on_6x9_c4_depth": random_case(4, 2, 4, 6, 9, 5, 7, True, bad_pixels=True, back=0.3),
        "16_c3": random_case(5, 2, 3, 16, 16, 16, 16, False, bad_pixels=True),
        "16_c4_depth": random_case(6, 2, 4, 16, 16, 16, 16, True),
        "64_c3_depth": random_case(7, 2, 3, 64, 64, 64, 64, True, bad_pixels=True),
        "64_c1": random_case(8, 2, 1, 64, 64, 64, 64, False),
        "behind": behind_case(),
    }
    for i, pair in enumerate(PAIRS):
        for size in (32, 64):
            out[f"plane_{i}_{size}"] = scene_case(pair, size, False, with_depth=(i != 0))
            out[f"sphere_{i}_{size}"] = scene_case(pair, size, True)
    return out


def dout_for(case, seed=0):
    """the upstream gradient the gradient tests use for an input set"""
    g = torch.Generator().manual_seed(1000 + seed)
    B, C = case.src.shape[:2]
    return torch.randn(B, C, *case.tgt_depth.shape[2:], generator=g)


def run(case, dout=None):
    return reproject64(case.src, case.tgt_depth, case.pose, case.zc_tgt, case.zc_src, case.src_depth, case.occ_tol, dout)
