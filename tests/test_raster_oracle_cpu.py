"""CPU: the fp64 yardstick of the mesh rasteriser (tests/raster_oracle.py) held to what can be known without it — a plane
z = const and a sphere by ray / sphere intersection — to its own invariances, and its input sets to the conditions the GPU
tests rely on: at most 2 % of a set's pixels inside the decision margin, and kappa <= 2 (the assumption under TAU_K)."""
import numpy as np
import pytest
import torch

import raster_oracle as ro

CASES = ro.cases()
NAMES = list(CASES)


def test_every_case_of_the_issue_is_there():
    assert NAMES == ["one_triangle", "sphere", "sphere_rect", "two_spheres", "dense", "subpixel", "big_triangle", "mixed", "cull",
                     "wide_fov"]
    c = CASES
    assert (c["one_triangle"].H, c["one_triangle"].W, c["one_triangle"].faces.shape[0]) == (8, 8, 1)
    assert (c["sphere"].H, c["sphere"].W, c["sphere"].faces.shape[0]) == (16, 16, 256)
    assert (c["sphere_rect"].H, c["sphere_rect"].W) == (20, 33)
    assert c["dense"].world2cam.shape[0] == 3 and c["dense"].faces.shape[0] == 4096 and c["dense"].H == 64
    assert c["subpixel"].faces.shape[0] == 16384 and c["subpixel"].H == 16
    assert c["cull"].cull == 'back' and torch.equal(c["cull"].faces, c["sphere"].faces)
    assert c["wide_fov"].zc == ro.zc_of(60)


@pytest.mark.parametrize("name", NAMES)
def test_margin_cap_and_condition(name):
    """conditions on the INPUTS, not measurements of the kernels"""
    r = ro.reference(name)
    share = float(r.margin.float().mean())
    kappa = ro.condition(CASES[name])
    print(f"{name}: margin {100 * share:.3f} % of the pixels, tau {r.tau_max:.3e} px, kappa {kappa:.2f}, covered {float(r.mask.float().mean()):.3f}")
    assert share <= 0.02
    assert kappa <= 2.0
    assert r.mask.any()
    # the nominal evaluation lies between the two shifted ones
    assert bool(((r.strict.mask <= r.mask) & (r.mask <= r.loose.mask)).all())


def test_properties_of_the_cases():
    r = ro.reference("subpixel")
    hit = torch.zeros(CASES["subpixel"].faces.shape[0], dtype=torch.bool)
    hit[r.face[r.face >= 0]] = True
    assert hit.float().mean() < 0.05                                   # most triangles cover no pixel centre
    assert bool(ro.reference("big_triangle").mask.all())              # it covers the whole frame
    q, u, v, _ = ro.project(CASES["big_triangle"])
    assert np.abs(u).max() > 10 * 64                                   # |u| >> W
    m = ro.reference("mixed")
    assert bool(m.mask.all()) and bool((m.face == 0).any()) and bool((m.face > 0).any())          # both paths win pixels
    t = ro.reference("two_spheres")
    inner = t.mask[:, 1:-1, 1:-1] == 1
    jump = (t.depth[:, 1:-1, 2:] - t.depth[:, 1:-1, :-2]).abs()
    assert float(jump[inner & (t.mask[:, 1:-1, 2:] == 1) & (t.mask[:, 1:-1, :-2] == 1)].max()) > 0.05   # a depth discontinuity
    s, c = ro.reference("sphere"), ro.reference("cull")
    firm = ~(s.margin | c.margin)
    assert torch.equal(s.mask[firm], c.mask[firm]) and torch.equal(s.depth[firm], c.depth[firm])  # the front faces win anyway


def _plane_case(z0, H, W, fov):
    """a two-triangle quad at z = z0 in camera space (identity camera) that covers the frame"""
    e = 3.0 * abs(z0)
    v = torch.tensor([[-e, -e, z0], [e, -e, z0], [e, e, z0], [-e, e, z0]])
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    return ro.make_case(v, f, torch.eye(3, 4).unsqueeze(0), fov, H, W)


def test_a_plane_has_the_depth_of_its_rays():
    case = _plane_case(-2.0, 9, 12, 40)
    r = ro.run(case)
    assert bool(r.mask.all())
    xg, yg = ro.grids(case.H, case.W)
    want = (-2.0 / case.zc) * np.sqrt(xg[None, :] ** 2 + yg[:, None] ** 2 + case.zc ** 2)
    assert np.abs(r.depth[0].numpy() - want).max() <= 1e-12
    assert float((r.lam.sum(-1) - 1).abs().max()) <= 1e-12 and float(r.lam.min()) >= -1e-12
    # points interpolated with lambda lie on the pixel's ray: perspective-correct
    pts = (r.lam[0].unsqueeze(-1) * case.vertices.double()[case.faces.long()[r.face[0]]]).sum(-2).numpy()
    d = np.stack(np.broadcast_arrays(xg[None, :], yg[:, None], case.zc), -1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    # (to the rounding of the fp32 grids: the direction is built from xg, yg, the coverage from the exact pixel index)
    assert np.abs(pts - d * r.depth[0].numpy()[..., None]).max() <= 2 * ro.EPS32 * float(r.depth.max())


def test_a_sphere_meets_ray_sphere_intersection_at_its_vertices_pixels():
    """the ray of each pixel intersected with the true sphere: the mesh is inscribed, so it is hit only inside the analytic
    silhouette, never before the sphere, and at most the facets' sagitta behind it — over the frame and at the pixels the front
    vertices project to"""
    R, c = 0.07, ro.cases()["sphere"]
    case = ro.make_case(*ro.uv_sphere(33, 64, R), c.world2cam, 12, 24, 24)
    r = ro.run(case)
    xg, yg = ro.grids(24, 24)
    d = np.stack(np.broadcast_arrays(xg[None, :], yg[:, None], case.zc), -1)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    M = case.world2cam[0].double().numpy()
    centre = M[:, 3]                                                    # the sphere's centre (world origin) in camera space
    bq = (d * centre).sum(-1)
    disc = bq ** 2 - (centre @ centre - R * R)
    hit = disc > 0
    t = bq - np.sqrt(np.where(hit, disc, 0))
    depth, mask = r.depth[0].numpy(), r.mask[0].numpy() == 1
    assert (mask <= hit).all() and mask.sum() > 0.9 * hit.sum()          # inscribed: inside the analytic silhouette
    sagitta = R * (1 - np.cos(np.pi / 33)) * 1.5
    inner = mask & (disc > (0.5 * R) ** 2)                              # away from the silhouette, where depth is steep
    assert inner.sum() > 100
    assert (depth[inner] >= t[inner] - 1e-12).all() and (depth[inner] - t[inner]).max() <= sagitta
    # the pixels nearest to the projected vertices of the front half
    q, u, v, _ = ro.project(case)
    for i in np.nonzero(-q[0, :, 2] < -centre[2])[0][::7]:
        rr, cc = int(round(v[0, i])), int(round(u[0, i]))
        if 0 <= rr < 24 and 0 <= cc < 24 and inner[rr, cc]:
            assert abs(depth[rr, cc] - t[rr, cc]) <= sagitta


@pytest.mark.parametrize("name", ["sphere", "two_spheres", "mixed"])
def test_permuting_the_faces_changes_face_only_by_the_permutation(name):
    case, r = CASES[name], ro.reference(name)
    T = case.faces.shape[0]
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(3))
    p = ro.run(ro.make_case(case.vertices, case.faces[perm], case.world2cam, 0, case.H, case.W, case.near, case.far, case.cull,
                            zc=case.zc))
    assert torch.equal(p.mask, r.mask) and torch.equal(p.depth, r.depth) and torch.equal(p.margin, r.margin)
    hit = r.face >= 0
    # an exact tie in depth (a pixel on a shared edge) may go to another of the tied faces: compare away from ties
    clear = hit & (r.runner > r.depth)
    assert torch.equal(perm[p.face[clear]], r.face[clear]) and bool((p.face[~hit] == -1).all())
    assert torch.equal(p.lam[clear], r.lam[clear])


def test_dropped_triangles_leave_nothing():
    case = CASES["sphere"]
    V = case.vertices.shape[0]
    nan = torch.tensor([[float('nan'), 0., 0.]])
    behind = torch.tensor([[0., 0., 5.]])                               # behind every orbit camera at radius 1
    extra_v = torch.cat([case.vertices, nan, behind])
    bad = torch.tensor([[0, 0, 1], [0, 1, V], [1, 2, V + 1], [0, 1, V + 2], [0, -1, 2]], dtype=torch.int32)
    only = ro.run(ro.make_case(extra_v, bad, case.world2cam, 0, 16, 16, zc=case.zc, far=7.5))
    assert not only.mask.any() and bool((only.face == -1).all()) and bool((only.depth == 7.5).all()) and not only.lam.any()
    both = ro.run(ro.make_case(extra_v, torch.cat([case.faces, bad]), case.world2cam, 0, 16, 16, zc=case.zc))
    r = ro.reference("sphere")
    assert torch.equal(both.face, r.face) and torch.equal(both.depth, r.depth) and torch.equal(both.lam, r.lam)
    empty = ro.run(ro.make_case(case.vertices, case.faces[:0], case.world2cam, 0, 16, 16, zc=case.zc))
    assert not empty.mask.any() and bool(torch.isinf(empty.depth).all())
