"""The fp64 yardstick of the mesh rasteriser (csrc/raster.hip; the rule: include/cips3d_hip.h, cips_raster_fwd), in numpy, and
the input sets its tests share.  Brute force: every triangle against every pixel of its bounding box (padded), no tiling, no
keys, no shared code with the kernels.

    q = R v + t,  u = (q.x zc / q.z + 1)(W-1)/2,  v = (1 - q.y zc / q.z)(H-1)/2,  valid iff q finite and -q.z >= near
    a triangle is dropped whole for an index outside [0, V), an invalid vertex, a zero / non-finite screen area, or, with
    cull='back', if it faces away: front-facing iff n . q0 < 0 with n = (q1-q0) x (q2-q0) in camera space (the 3-D statement;
    the kernels read it off the sign of the screen area)
    pixel (r, c) is covered iff its signed distance to each of the three edge lines, counted positive inside, is >= shift
    1/z = sum beta_i / q_i.z,  lambda_i = (beta_i / q_i.z) / sum,  depth = (z / zc) |(xg[c], yg[r], zc)|
    winner: the smallest depth, equal depths to the lower face index

THE DECISION MARGIN.  The kernels place a projected vertex with fp32 arithmetic.  With eps = 2^-24, to first order in eps:
  * q.x = fma(R02, z, fma(R01, y, R00 x)) + t.x is four roundings, each of a partial sum no larger than S_x = sum_j |R_0j v_j| +
    |t.x|:  |dq.x| <= 4 eps S_x, and the same for y and z.
  * xs = (q.x zc) / q.z adds two roundings:  |dxs| <= 4 eps S_x |zc| / |q.z| + |xs| (4 eps S_z / |q.z|) + 2 eps |xs|.
  * u = (xs + 1) h with h = (W-1)/2 (exact in fp32) adds two more:  |du| <= h |dxs| + 2 eps |u|,  and h |xs| <= |u| + h.
  Let M = max(W, H, |u|, |v|) of the vertex, Z = max(1, |zc|) and kappa the largest, over the valid vertices of an input set, of
  S_x |zc| h / (|q.z| Z M), the same in y, and S_z / |q.z| (condition(): a property of the INPUTS, 1.3 for an object of radius
  0.15 seen from distance 1, and held to <= 2 by tests/test_raster_oracle_cpu.py).  Then, with h <= M / 2,
      |du| <= eps [4 kappa Z M + (4 kappa + 2) 1.5 M + 2 M] <= (10 kappa + 5) eps Z M <= 25 eps Z M.
  * the edge value (u_hi - u_lo)(r - v_lo) - (v_hi - v_lo)(c - u_lo): four differences, two products, one difference; the two
    products are each at most L * 2M (L the edge's length), so the value is off by at most 12 eps M L: 12 eps M px of distance.
  TAU_K = 25 + 12 = 37:  tau = 37 eps Z max(W, H, |u|, |v|), the largest over a triangle's three vertices, bounds how far an edge
  line of the kernels can lie from the oracle's as seen from a pixel that the decision concerns.
The oracle is evaluated with shift = -tau (every pixel the kernels could cover) and shift = +tau (every pixel they must cover).
A pixel where the two evaluations differ in mask, or in depth by more than the depth bar, is in the margin and left out of the
value comparisons; tests/test_raster_oracle_cpu.py holds every input set to at most 2 % of such pixels.

Away from the margin the winner's plane is known, and moving vertex i by d_i changes an interpolated quantity g at a fixed pixel
by -beta_i grad g . d_i: at most tau (|dg/du| + |dg/dv|) over the three vertices together.  The oracle returns these screen
slopes for depth and for each lambda_i, and the depth of the runner-up (the second smallest depth among the covering
triangles): where that lies within the depth bar of the winner, two triangles meet and either may win."""
from types import SimpleNamespace

import numpy as np
import torch

EPS32 = 2.0 ** -24
TAU_K = 37


def zc_of(fov):
    """the image-plane constant of a field of view in degrees, rounded to fp32 (generator._zc's quantity)"""
    return float(np.float32(-1.0 / np.tan(np.radians(float(fov)) / 2)))


def orbit_world2cam(yaws, pitches, radius=1.0, lookat=(0., 0., 0.)):
    """fp64: cameras on a sphere around lookat, looking at it, up = +y -> world2cam (b,3,4) fp32 (rounded once)"""
    out = []
    for th, ph in zip(yaws, pitches):
        off = radius * np.array([np.sin(ph) * np.cos(th), np.cos(ph), np.sin(ph) * np.sin(th)])
        fwd = -off / np.linalg.norm(off)
        left = np.cross([0., 1., 0.], fwd)
        left /= np.linalg.norm(left)
        up = np.cross(fwd, left)
        up /= np.linalg.norm(up)
        R = np.stack([-left, up, -fwd], axis=1)                      # cam2world's rotation, columns
        o = off + np.asarray(lookat, dtype=np.float64)
        out.append(np.concatenate([R.T, -(R.T @ o)[:, None]], axis=1))
    return torch.from_numpy(np.stack(out).astype(np.float32))


def uv_sphere(bands, lon, radius, center=(0., 0., 0.)):
    """a UV sphere with poles: 2 * lon * (bands - 1) faces wound outwards -> vertices (V,3) fp32, faces (T,3) int32"""
    verts = [[0., 1., 0.]]
    for i in range(1, bands):
        a = np.pi * i / bands
        for j in range(lon):
            b = 2 * np.pi * j / lon
            verts.append([np.sin(a) * np.cos(b), np.cos(a), np.sin(a) * np.sin(b)])
    verts.append([0., -1., 0.])
    ring = lambda i, j: 1 + (i - 1) * lon + j % lon
    faces = []
    for j in range(lon):
        faces.append([0, ring(1, j + 1), ring(1, j)])
        faces.append([len(verts) - 1, ring(bands - 1, j), ring(bands - 1, j + 1)])
    for i in range(1, bands - 1):
        for j in range(lon):
            faces.append([ring(i, j), ring(i, j + 1), ring(i + 1, j)])
            faces.append([ring(i, j + 1), ring(i + 1, j + 1), ring(i + 1, j)])
    v = np.asarray(verts) * radius + np.asarray(center)
    f = np.asarray(faces, dtype=np.int32)
    # outwards: flip what is not
    c = v[f].mean(1) - np.asarray(center)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    flip = (n * c).sum(1) < 0
    f[flip] = f[flip][:, [0, 2, 1]]
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f)


def make_case(vertices, faces, world2cam, fov, H, W, near=1e-4, far=float('inf'), cull=None, zc=None):
    return SimpleNamespace(vertices=vertices, faces=faces, world2cam=world2cam, zc=zc_of(fov) if zc is None else float(zc),
                           H=H, W=W, near=near, far=far, cull=cull)


def merge(*meshes):
    """several (vertices, faces) as one mesh"""
    vs, fs, base = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + base)
        base += v.shape[0]
    return torch.cat(vs), torch.cat(fs).to(torch.int32)


# a triangle that covers the whole frame of a camera at (0, 0, 1) with fov 12, its vertices hundreds of pixels outside it
BIG_TRIANGLE = (torch.tensor([[-3.0, -2.5, -0.35], [3.2, -2.4, -0.25], [0.1, 4.0, -0.3]]), torch.tensor([[0, 1, 2]], dtype=torch.int32))
HALF_PI = np.pi / 2


def cases():
    front = orbit_world2cam([HALF_PI], [HALF_PI])
    tilted = orbit_world2cam([1.3], [1.4])
    sphere = uv_sphere(9, 16, 0.07)
    c = {}
    c["one_triangle"] = make_case(torch.tensor([[-0.06, -0.05, 0.0], [0.07, -0.03, 0.02], [0.01, 0.08, -0.01]]),
                                  torch.tensor([[0, 1, 2]], dtype=torch.int32), front, 12, 8, 8)
    c["sphere"] = make_case(*sphere, tilted, 12, 16, 16)
    c["sphere_rect"] = make_case(*sphere, tilted, 12, 20, 33)
    c["two_spheres"] = make_case(*merge(uv_sphere(9, 16, 0.05, (0.02, 0.0, 0.05)), uv_sphere(9, 16, 0.06, (-0.03, 0.01, -0.05))),
                                 tilted, 12, 32, 32)
    c["dense"] = make_case(*uv_sphere(33, 64, 0.08), orbit_world2cam([1.2, HALF_PI, 1.9], [1.4, HALF_PI, 1.7]), 12, 64, 64)
    c["subpixel"] = make_case(*uv_sphere(65, 128, 0.07), tilted, 12, 16, 16)
    c["big_triangle"] = make_case(*BIG_TRIANGLE, front, 12, 64, 64)
    c["mixed"] = make_case(*merge(BIG_TRIANGLE, sphere), front, 12, 64, 64)
    c["cull"] = make_case(*sphere, tilted, 12, 16, 16, cull='back')
    c["wide_fov"] = make_case(*uv_sphere(9, 16, 0.15, (0.2, 0.08, 0.0)), orbit_world2cam([1.0], [1.2]), 60, 32, 32)
    return c


def grids(H, W):
    """the fp32 pixel grids of the ray set-up, as fp64"""
    return torch.linspace(-1, 1, W).double().numpy(), torch.linspace(1, -1, H).double().numpy()


def project(case):
    """-> q (B,V,3), u, v (B,V), valid (B,V), all fp64 / bool"""
    vt = case.vertices.double().numpy().reshape(-1, 3)
    M = case.world2cam.double().numpy()[:, :3]
    q = np.einsum("bij,vj->bvi", M[:, :, :3], vt) + M[:, None, :, 3]
    with np.errstate(all="ignore"):
        u = (q[..., 0] * case.zc / q[..., 2] + 1) * (case.W - 1) / 2
        v = (1 - q[..., 1] * case.zc / q[..., 2]) * (case.H - 1) / 2
        valid = np.isfinite(q).all(-1) & (-q[..., 2] >= case.near)
    return q, u, v, valid


def condition(case):
    """kappa of the module docstring: how much larger than its result the sums behind a projected vertex are"""
    vt = np.abs(case.vertices.double().numpy().reshape(-1, 3))
    M = np.abs(case.world2cam.double().numpy()[:, :3])
    S = np.einsum("bij,vj->bvi", M[:, :, :3], vt) + M[:, None, :, 3]
    q, u, v, valid = project(case)
    if not valid.any():
        return 0.0
    Z = max(1.0, abs(case.zc))
    with np.errstate(all="ignore"):
        Mx = np.maximum(np.maximum(np.abs(u), np.abs(v)), max(case.W, case.H))
        az = np.abs(q[..., 2])
        kx = S[..., 0] * abs(case.zc) * (case.W - 1) / 2 / (az * Z * Mx)
        ky = S[..., 1] * abs(case.zc) * (case.H - 1) / 2 / (az * Z * Mx)
        kz = S[..., 2] / az
    return float(np.max(np.stack([kx, ky, kz])[:, valid]))


def _raster_camera(case, b, q, u, v, valid, xg, yg):
    """one camera, the three shifts at once -> dict shift -> per-pixel arrays"""
    H, W, T = case.H, case.W, case.faces.shape[0]
    V = case.vertices.shape[0]
    f = case.faces.numpy().astype(np.int64).reshape(-1, 3)
    res = {}
    blank = lambda: dict(face=np.full((H, W), -1, np.int64), lam=np.zeros((H, W, 3)), depth=np.full((H, W), float(case.far)),
                         mask=np.zeros((H, W), np.uint8), slope=np.zeros((H, W)), slope_lam=np.zeros((H, W, 3)),
                         runner=np.full((H, W), np.inf), tau=np.zeros((H, W)))
    for s in (-1, 0, 1):
        res[s] = blank()
    res["tau_max"] = 0.0
    if T == 0 or V == 0:
        return res
    ok = ((f >= 0) & (f < V)).all(1)
    fi = np.where(ok[:, None], f, 0)
    ok &= valid[b][fi].all(1)
    U, Vv, Q = u[b][fi], v[b][fi], q[b][fi]                                  # (T,3), (T,3), (T,3,3)
    with np.errstate(all="ignore"):
        area = (U[:, 1] - U[:, 0]) * (Vv[:, 2] - Vv[:, 0]) - (Vv[:, 1] - Vv[:, 0]) * (U[:, 2] - U[:, 0])
        ok &= np.isfinite(area) & (area != 0) & np.isfinite(U).all(1) & np.isfinite(Vv).all(1)
        if case.cull == 'back':
            n = np.cross(Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 0])
            ok &= (n * Q[:, 0]).sum(1) < 0
    tid = np.nonzero(ok)[0]
    if tid.size == 0:
        return res
    U, Vv, Q, area = U[tid], Vv[tid], Q[tid], area[tid]
    Z = max(1.0, abs(case.zc))
    tau = TAU_K * EPS32 * Z * np.maximum(np.maximum(np.abs(U), np.abs(Vv)).max(1), max(W, H))
    res["tau_max"] = float(tau.max())
    pad = tau + 1e-9
    x0 = np.clip(np.floor(U.min(1) - pad), 0, W - 1).astype(np.int64)
    x1 = np.clip(np.ceil(U.max(1) + pad), 0, W - 1).astype(np.int64)
    y0 = np.clip(np.floor(Vv.min(1) - pad), 0, H - 1).astype(np.int64)
    y1 = np.clip(np.ceil(Vv.max(1) + pad), 0, H - 1).astype(np.int64)
    inside = (U.max(1) + pad >= 0) & (U.min(1) - pad <= W - 1) & (Vv.max(1) + pad >= 0) & (Vv.min(1) - pad <= H - 1)
    bw = np.where(inside, x1 - x0 + 1, 0)
    cnt = bw * np.where(inside, y1 - y0 + 1, 0)
    if cnt.sum() == 0:
        return res
    k = np.repeat(np.arange(tid.size), cnt)                                   # the pairs (triangle k, pixel (r, c))
    off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    r = y0[k] + off // bw[k]
    c = x0[k] + off % bw[k]
    px, py = c.astype(np.float64), r.astype(np.float64)
    sgn = np.sign(area)[k]
    E, dist, dEu, dEv = [], [], [], []
    for i in range(3):
        j, l = (i + 1) % 3, (i + 2) % 3
        ax, ay = U[k, l] - U[k, j], Vv[k, l] - Vv[k, j]
        E.append(ax * (py - Vv[k, j]) - ay * (px - U[k, j]))
        dist.append(sgn * E[i] / np.hypot(ax, ay))
        dEu.append(-ay)
        dEv.append(ax)
    dmin = np.minimum(np.minimum(dist[0], dist[1]), dist[2])
    A = area[k]
    iz = [1.0 / Q[k, i, 2] for i in range(3)]
    g = sum(E[i] / A * iz[i] for i in range(3))                               # 1 / z
    gu = sum(dEu[i] / A * iz[i] for i in range(3))
    gv = sum(dEv[i] / A * iz[i] for i in range(3))
    nrm = np.sqrt(xg[c] ** 2 + yg[r] ** 2 + case.zc ** 2)
    with np.errstate(all="ignore"):
        depth = nrm / (case.zc * g)
        slope = np.abs(depth) * (np.abs(gu) + np.abs(gv)) / np.abs(g)
        lam = [E[i] / A * iz[i] / g for i in range(3)]
        slam = [np.abs((dEu[i] / A * iz[i] - lam[i] * gu) / g) + np.abs((dEv[i] / A * iz[i] - lam[i] * gv) / g) for i in range(3)]
    good = np.isfinite(depth) & (depth > 0)
    pix = r * W + c
    for s in (-1, 0, 1):
        sel = np.nonzero(good & (dmin >= s * tau[k]))[0]
        if sel.size == 0:
            continue
        order = sel[np.lexsort((tid[k][sel], depth[sel], pix[sel]))]          # by pixel, then depth, then face index
        first = np.ones(order.size, bool)
        first[1:] = pix[order][1:] != pix[order][:-1]
        w = order[first]
        o = res[s]
        rr, cc = r[w], c[w]
        o["face"][rr, cc] = tid[k][w]
        o["depth"][rr, cc] = depth[w]
        o["mask"][rr, cc] = 1
        o["slope"][rr, cc] = slope[w]
        o["tau"][rr, cc] = tau[k][w]
        for i in range(3):
            o["lam"][rr, cc, i] = lam[i][w]
            o["slope_lam"][rr, cc, i] = slam[i][w]
        second = np.zeros(order.size, bool)
        second[1:] = first[:-1] & ~first[1:]
        w2 = order[second]
        o["runner"][r[w2], c[w2]] = depth[w2]
    return res


def depth_bar(tau, slope, depth):
    return tau * slope + 16 * EPS32 * np.abs(depth)


_KEYS = ("face", "lam", "depth", "mask", "slope", "slope_lam", "runner", "tau")


def run(case):
    """-> SimpleNamespace of torch tensors over (B,H,W[,3]): face (int64), lam, depth, mask (uint8), slope, slope_lam, runner of
    the nominal evaluation (shift 0), tau: the winning triangle's tau per pixel (tau_max: the largest of all triangles); margin
    (bool): where the evaluations at -tau and +tau differ; loose / strict: the two shifted evaluations' (mask, depth)"""
    q, u, v, valid = project(case)
    xg, yg = grids(case.H, case.W)
    B = case.world2cam.shape[0]
    per = [_raster_camera(case, b, q, u, v, valid, xg, yg) for b in range(B)]
    out = SimpleNamespace(tau_max=max([p["tau_max"] for p in per] + [0.0]))
    for key in _KEYS:
        setattr(out, key, torch.from_numpy(np.stack([p[0][key] for p in per])))
    lo = {key: np.stack([p[-1][key] for p in per]) for key in ("mask", "depth", "slope", "tau")}
    hi = {key: np.stack([p[1][key] for p in per]) for key in ("mask", "depth", "slope", "tau")}
    both = (lo["mask"] == 1) & (hi["mask"] == 1)
    with np.errstate(all="ignore"):
        bar = depth_bar(np.maximum(lo["tau"], hi["tau"]), np.maximum(lo["slope"], hi["slope"]), hi["depth"])
        margin = (lo["mask"] != hi["mask"]) | (both & (np.abs(lo["depth"] - hi["depth"]) > bar))
    out.margin = torch.from_numpy(margin)
    out.loose = SimpleNamespace(mask=torch.from_numpy(lo["mask"]), depth=torch.from_numpy(lo["depth"]))
    out.strict = SimpleNamespace(mask=torch.from_numpy(hi["mask"]), depth=torch.from_numpy(hi["depth"]))
    return out


_RESULTS = {}


def reference(name):
    """the oracle's result for one of cases(), computed once per process and shared: leave it unchanged"""
    if name not in _RESULTS:
        _RESULTS[name] = run(cases()[name])
    return _RESULTS[name]


def compare(case, r, face, bary, depth, mask):
    """The rasteriser's four outputs (tensors on any device) against run(case)'s result r: asserts what holds everywhere and the
    decisions away from the margin, and returns SimpleNamespace(depth, lam: the largest error over its bar away from the
    margin; otherwise: how many margin pixels were decided otherwise than by the nominal oracle; exempt: how many pixels took
    the runner-up, whose depth lies within the bar).
      depth bar   tau slope + 16 eps depth          lambda bar   tau slope_lambda_i + 16 eps |lambda_i|"""
    face, bary, depth, mask = face.cpu(), bary.cpu().double(), depth.cpu().double(), mask.cpu()
    T, far = case.faces.shape[0], float(case.far)
    assert face.dtype == torch.int32 and mask.dtype == torch.uint8
    assert face.shape == r.face.shape and bary.shape == r.lam.shape and depth.shape == r.depth.shape and mask.shape == r.mask.shape
    # everywhere, the margins included
    assert bool(((face >= -1) & (face < max(T, 1))).all()) and (T > 0 or bool((face == -1).all()))
    assert bool((mask <= 1).all()) and torch.equal(mask == 1, face >= 0)
    assert bool(torch.isfinite(bary).all())
    assert bool((torch.isfinite(depth) | (depth == far)).all())
    assert bool((depth[mask == 0] == far).all()) and not bool(bary[mask == 0].any())
    firm = ~r.margin
    assert torch.equal(mask[firm], r.mask[firm])
    hit = firm & (r.mask == 1)
    bar = torch.from_numpy(depth_bar(r.tau.numpy(), r.slope.numpy(), r.depth.numpy()))
    tie = (r.runner - r.depth) <= bar
    same = face.long() == r.face
    assert bool(same[hit & ~tie].all())
    sel = hit & same
    # a pixel that took the runner-up has the runner-up's depth
    q_depth = torch.cat([((depth - r.depth).abs() / bar)[sel], ((depth - r.runner).abs() / bar)[hit & ~same]])
    bar_lam = r.tau.unsqueeze(-1) * r.slope_lam + 16 * EPS32 * r.lam.abs()
    q_lam = ((bary - r.lam).abs() / bar_lam.clamp_min(1e-300))[sel]
    mx = lambda t: float(t.max()) if t.numel() else 0.0
    return SimpleNamespace(depth=mx(q_depth), lam=mx(q_lam), otherwise=int((mask != r.mask)[r.margin].sum()),
                           exempt=int((hit & ~same).sum()), margin=int(r.margin.sum()))
