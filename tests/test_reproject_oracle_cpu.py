"""CPU: the fp64 yardstick of the view reprojection (tests/reproject_oracle.py) held to three things that do not come from
the same pen: (a) an analytic scene rendered in fp64 from two cameras built with the generator's own camera helpers, (b) fp64
central differences, (c) the 2 % cap on the share of pixels inside a decision margin, for every input set the GPU tests use."""
import math

import pytest
import torch

import reproject_oracle as ro


@pytest.mark.parametrize("pair", range(len(ro.PAIRS)))
def test_plane_scene_warps_onto_itself_and_converges_at_second_order(pair):
    """warping view B into view A reproduces view A on the visible pixels, up to the bilinear interpolation of B: O(h^2), so
    the mean error falls by about 4x from 32^2 to 64^2 (3x to 5.5x is asked).  A flipped row order, a transposed matrix or a
    wrong sign leaves errors of the texture's own size (~0.5) and no convergence."""
    err = {}
    for size in (32, 64):
        s = ro.scene_pair(ro.PAIRS[pair], size, sphere=False)
        r = ro.reproject64(s.b_img, s.a_depth, s.pose, s.zc, s.zc, s.b_depth, 2e-3)
        vis = r.mask == 1
        assert not (r.mask == 2).any()                          # a plane hides nothing of itself
        assert 0.3 < vis.double().mean() < 1.0                  # the cameras are 0.3 rad apart: part of A is outside B
        e = ((r.out - s.a_img.double()).abs() * vis).sum() / (3 * vis.sum())
        err[size] = float(e)
        print(f"pair {pair} size {size}: coverage {float(vis.double().mean()):.3f} mean error {err[size]:.3e}")
        assert err[size] < 2e-2
        # the correspondence itself: uv is where B's camera sees A's world point
        cam_b = s.cams[1:].double()
        pb = torch.einsum("bji,bhwj->bhwi", cam_b[:, :3, :3], s.a_pts - cam_b[:, :3, 3].view(1, 1, 1, 3))
        u = (pb[..., 0] * s.zc / pb[..., 2] + 1) / 2 * (size - 1)
        v = (1 - pb[..., 1] * s.zc / pb[..., 2]) / 2 * (size - 1)
        # a_depth and the pose are fp32 roundings of the scene's fp64 values: 2^-24 * |zc| * size / 2 px each, a few of them
        tol = 8 * ro.EPS32 * abs(s.zc) * size / 2
        sel = vis[:, 0] & ~r.near[:, 0]
        assert (r.uv[:, 0][sel] - u[sel]).abs().max() < tol and (r.uv[:, 1][sel] - v[sel]).abs().max() < tol
    assert 3.0 < err[32] / err[64] < 5.5, err


@pytest.mark.parametrize("pair", range(len(ro.PAIRS)))
@pytest.mark.parametrize("size", [32, 64])
def test_sphere_hides_what_the_other_camera_cannot_see(pair, size):
    """with the sphere, the pixels of A whose world point B cannot see (B's ray to that point hits the sphere first) come out
    as mask == 2, the others that land in B's frame as 1; decided here by an exact ray-sphere test, away from the margins"""
    s = ro.scene_pair(ro.PAIRS[pair], size, sphere=True)
    r = ro.reproject64(s.b_img, s.a_depth, s.pose, s.zc, s.zc, s.b_depth, 2e-3)
    ob = s.cams[1, :3, 3].double()
    seg = s.a_pts[0] - ob                                        # B's camera -> A's world point
    L = seg.norm(dim=-1)
    dd = seg / L.unsqueeze(-1)
    bq = (ob * dd).sum(-1)
    disc = bq * bq - ((ob * ob).sum() - ro.SPHERE_R ** 2)
    t_hit = -bq - disc.clamp_min(0).sqrt()
    hidden = (disc > 0) & (t_hit > 0) & (t_hit < L - 1e-2)        # the sphere is met well before the point
    clear = (disc < 0) | (t_hit > L - 1e-4)                      # not met, or met at the point itself (it lies on the sphere)
    firm = (r.mask[0, 0] != 0) & ~r.near[0, 0]
    # at B's silhouette of the sphere the bilinear sample of B's depth mixes sphere and plane: those pixels are decided by the
    # interpolated depth, not by the exact test; they are the ones whose cell of B's depth spans the two surfaces
    u0, v0 = r.uv[0, 0].nan_to_num().floor().long().clamp(max=size - 2), r.uv[0, 1].nan_to_num().floor().long().clamp(max=size - 2)
    bd = s.b_depth[0, 0].double()
    cell = torch.stack([bd[v0, u0], bd[v0, u0 + 1], bd[v0 + 1, u0], bd[v0 + 1, u0 + 1]])
    flat = (cell.amax(0) - cell.amin(0)) < 5e-3
    assert (hidden & firm).sum() > 0.01 * size * size           # the scene does hide something
    assert (r.mask[0, 0][hidden & firm & flat] == 2).all()
    assert (r.mask[0, 0][clear & firm & flat] == 1).all()
    vis = (r.mask == 1) & flat
    e = ((r.out - s.a_img.double()).abs() * vis).sum() / (3 * vis.sum())
    print(f"pair {pair} size {size}: visible {int((r.mask == 1).sum())} occluded {int((r.mask == 2).sum())} error {float(e):.3e}")
    assert float(e) < 2e-2


@pytest.mark.parametrize("name", ["5x7_on_6x9_c4_depth", "16_c3", "sphere_2_32", "behind"])
def test_oracle_gradients_against_central_differences(name):
    case = ro.cases()[name]
    dout = ro.dout_for(case)
    r = ro.run(case, dout)
    g = dout.double()
    vis = r.mask == 1

    def loss_per_pixel(src, depth):
        o = ro.reproject64(src, depth, case.pose, case.zc_tgt, case.zc_src, case.src_depth, case.occ_tol).out
        return (o * g * vis).sum(1, keepdim=True)

    # every target pixel's output depends on its own depth alone: one central difference serves all pixels.  Pixels near a
    # decision or an integer u / v (where a step may change the mask or the cell) are left out.
    h = 1e-7
    src, depth = case.src.double(), case.tgt_depth.double()
    fd = (loss_per_pixel(src, depth + h) - loss_per_pixel(src, depth - h)) / (2 * h)
    sel = vis & ~r.near_grad & torch.isfinite(fd)
    assert sel.sum() > 0.5 * vis.sum() > 0
    scale = r.d_tgt_depth[sel].abs().max()
    print(f"{name}: d_tgt_depth vs central differences {float((fd - r.d_tgt_depth)[sel].abs().max() / scale):.2e} of its maximum")
    assert (fd - r.d_tgt_depth)[sel].abs().max() < 1e-6 * scale
    assert (r.d_tgt_depth[~vis] == 0).all()
    # out is linear in src: a central difference along a random direction is exact up to rounding
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        delta = torch.randn(src.shape, generator=gen, dtype=torch.float64)
        fd = (loss_per_pixel(src + delta, depth).sum() - loss_per_pixel(src - delta, depth).sum()) / 2
        assert abs(float(fd - (r.d_src * delta).sum())) < 1e-10 * float((r.d_src * delta).abs().sum())
    # the analytic du / ddepth of the definition against autograd's
    M = case.pose.double()
    d = ro.ray_dirs(*case.tgt_depth.shape[2:], case.zc_tgt)
    e = torch.einsum("bij,jhw->bihw", M[:, :, :3], d)
    t = torch.where(torch.isfinite(depth) & (depth > 0), depth, torch.ones_like(depth))
    qp = torch.einsum("bij,bjhw->bihw", M[:, :, :3], d.unsqueeze(0) * t) + M[:, :, 3].view(-1, 3, 1, 1)
    Hs, Ws = case.src.shape[2:]
    dudt = (Ws - 1) / 2 * case.zc_src * (e[:, 0:1] * qp[:, 2:3] - qp[:, 0:1] * e[:, 2:3]) / qp[:, 2:3] ** 2
    dvdt = -(Hs - 1) / 2 * case.zc_src * (e[:, 1:2] * qp[:, 2:3] - qp[:, 1:2] * e[:, 2:3]) / qp[:, 2:3] ** 2
    for mine, auto in ((dudt, r.dudt), (dvdt, r.dvdt)):
        assert (mine - auto)[sel].abs().max() <= 1e-12 * max(1.0, float(auto[sel].abs().max()))


@pytest.mark.parametrize("name", list(ro.cases()))
def test_share_of_pixels_inside_a_margin_stays_under_the_cap(name):
    """at most 2 % of an input set's pixels lie within 1e-2 px of a frame test, 2e-4 of the occlusion test or — for the
    gradient comparisons — 1e-3 px of an integer u or v.  If a case exceeds it, move its cameras, not the cap."""
    case = ro.cases()[name]
    r = ro.run(case)
    npx = r.mask.numel()
    share, share_grad = float(r.near.sum()) / npx, float(r.near_grad.sum()) / npx
    counts = [int((r.mask == k).sum()) for k in range(3)]
    print(f"{name}: mask 0/1/2 = {counts}, near a value margin {100 * share:.2f} %, with the integer margin {100 * share_grad:.2f} %")
    assert share <= 0.02 and share_grad <= 0.02
    assert counts[1] > 0
    if name == "behind":
        M, d = case.pose.double(), ro.ray_dirs(16, 16, case.zc_tgt)
        t = case.tgt_depth.double()
        qz = torch.einsum("bj,bjhw->bhw", M[:, 2, :3], d.unsqueeze(0) * t) + M[:, 2, 3].view(-1, 1, 1)
        behind = qz * case.zc_src <= 0
        assert 0 < behind.sum() < behind.numel() and (r.mask[:, 0][behind] == 0).all()


def test_identity_warp_has_full_coverage_with_the_slack():
    """tgt2src = identity, src_depth = tgt_depth: every pixel lands on itself — the last row and column too, which is what the
    1/256 px of slack in the frame test is for"""
    c = ro.random_case(11, 2, 3, 16, 16, 16, 16, True)
    c.pose = torch.eye(3, 4).repeat(2, 1, 1)
    r = ro.reproject64(c.src, c.tgt_depth, c.pose, c.zc_tgt, c.zc_src, c.tgt_depth, 1e-4)
    assert (r.mask == 1).all()
    jj, ii = torch.arange(16.).view(1, 16).expand(16, 16), torch.arange(16.).view(16, 1).expand(16, 16)
    assert (r.uv[:, 0] - jj).abs().max() < 1e-12 and (r.uv[:, 1] - ii).abs().max() < 1e-12
    assert (r.out - c.src.double()).abs().max() < 1e-12


def test_relative_pose_is_the_fp64_composition():
    from cips3d_amd.evaluation import relative_pose
    cams = ro.cameras([1.3, 1.9, math.pi / 2], [1.5, 1.7, math.pi / 2])
    a, b = cams, cams.roll(1, 0)
    p = relative_pose(a, b)
    assert p.dtype == torch.float32 and p.shape == (3, 4 - 1, 4)
    assert torch.equal(p, ro.relative_pose64(a, b))
    # a world point seen from both cameras: the pose takes its target-camera coordinates to its source-camera coordinates
    w = torch.tensor([0.03, -0.02, 0.05], dtype=torch.float64)
    ca, cb = a.double(), b.double()
    pa = torch.einsum("bji,bj->bi", ca[:, :3, :3], w - ca[:, :3, 3])
    pb = torch.einsum("bji,bj->bi", cb[:, :3, :3], w - cb[:, :3, 3])
    got = torch.einsum("bij,bj->bi", p.double()[:, :, :3], pa) + p.double()[:, :, 3]
    assert (got - pb).abs().max() < 1e-6
    with pytest.raises(ValueError):
        relative_pose(a, b[:2])
    with pytest.raises(ValueError):
        relative_pose(a[:, :2], b)
