"""Test infrastructure (like render_regimes.py): marching tetrahedra on the Kuhn decomposition of a lattice, stated in vectorised
numpy.  This is the normative statement of the rules of DESIGN.md section 3 "Meshes"; the HIP kernels (csrc/mesh.hip) are compared
against it, faces exactly and positions to rounding.

Lattice: point p = (i * ny + j) * nz + k is (gx[i], gy[j], gz[k]); inside iff sigma > level (NaN is outside).
Tetrahedra: cell (i, j, k) splits into six, one per permutation pi of the axes in itertools.permutations order, with the path
v0 = (i, j, k), v1 = v0 + e_pi0, v2 = v1 + e_pi1, v3 = v2 + e_pi2.  Every tetrahedron edge runs from a lattice point p to p + d,
d a non-zero 0/1 vector: edge class c = 4 dx + 2 dy + dz - 1 of its lower point p.
Vertices: one per edge whose ends differ in inside / outside, ordered by (p, c); positions in fp64 from the fp32 inputs.
Triangles: ordered by cell, tetrahedron, piece; wound so that (P1 - P0) x (P2 - P0) points from inside to outside, decided from
the integer geometry of the tetrahedron alone."""
import itertools

import numpy as np

PERMS = tuple(itertools.permutations((0, 1, 2)))
UNIT = np.eye(3, dtype=np.int64)


def path(perm):
    """the four lattice offsets v0..v3 of the tetrahedron of `perm`"""
    v = [np.zeros(3, dtype=np.int64)]
    for a in perm:
        v.append(v[-1] + UNIT[a])
    return v


def edge_class(d):
    return 4 * int(d[0]) + 2 * int(d[1]) + int(d[2]) - 1


def tet_triangles(perm, inside):
    """the triangles of one tetrahedron for the inside flags of v0..v3 -> list of triangles, each three edges (a, b), a < b path
    indices.  The winding comes from integer determinants of the path offsets."""
    v = path(perm)
    ins = [m for m in range(4) if inside[m]]
    out = [m for m in range(4) if not inside[m]]
    if not ins or not out:
        return []
    e = lambda a, b: (min(a, b), max(a, b))
    if len(ins) == 1 or len(out) == 1:
        A = ins[0] if len(ins) == 1 else out[0]
        R = [m for m in range(4) if m != A]
        det = int(round(np.linalg.det(np.stack([v[r] - v[A] for r in R]).astype(np.float64))))
        assert det in (-1, 1)
        # (A R0, A R1, A R2) has its normal pointing away from A iff det > 0; it must point away from an inside A and towards an
        # outside one
        tri = [e(A, R[0]), e(A, R[1]), e(A, R[2])]
        if (det > 0) != (len(ins) == 1):
            tri = [tri[0], tri[2], tri[1]]
        return [tri]
    A, B = ins
    C, D = out
    # quad (AC, AD, BD, BC): at t = 1/2 the normal of (AC, AD, BD) is (D - C) x (B - A) / 4, and it must have a positive
    # component along the direction from the inside pair to the outside pair, (C + D - A - B) / 2 = (C - A) + (u - w) / 2
    det = int(round(np.linalg.det(np.stack([v[D] - v[C], v[B] - v[A], v[C] - v[A]]).astype(np.float64))))
    assert det in (-1, 1)
    t0 = [e(A, C), e(A, D), e(B, D)]
    t1 = [e(A, C), e(B, D), e(B, C)]
    if det < 0:
        t0 = [t0[0], t0[2], t0[1]]
        t1 = [t1[0], t1[2], t1[1]]
    return [t0, t1]


def _case_table():
    """(6, 16, 2, 3, 2) corner offsets (as corner bits 4dx+2dy+dz of the edge's lower point) and edge classes; (6, 16) counts"""
    own = np.zeros((6, 16, 2, 3), dtype=np.int64)
    cls = np.zeros((6, 16, 2, 3), dtype=np.int64)
    cnt = np.zeros((6, 16), dtype=np.int64)
    for t, perm in enumerate(PERMS):
        v = path(perm)
        for case in range(16):
            tris = tet_triangles(perm, [(case >> m) & 1 for m in range(4)])
            cnt[t, case] = len(tris)
            for n, tri in enumerate(tris):
                for s, (a, b) in enumerate(tri):
                    own[t, case, n, s] = 4 * v[a][0] + 2 * v[a][1] + v[a][2]
                    cls[t, case, n, s] = edge_class(v[b] - v[a])
    return own, cls, cnt


_OWN, _CLS, _CNT = _case_table()


def marching_tetrahedra(sigma, gx, gy, gz, level):
    """sigma (nx, ny, nz) fp32, gx / gy / gz fp32 strictly increasing -> vertices (V, 3) fp64, faces (T, 3) int64,
    and per vertex its (p, c) (V, 2) int64"""
    sigma = np.asarray(sigma, dtype=np.float32)
    g = [np.asarray(a, dtype=np.float32) for a in (gx, gy, gz)]
    nx, ny, nz = sigma.shape
    assert (nx, ny, nz) == tuple(len(a) for a in g) and min(nx, ny, nz) >= 2
    level = np.float32(level)
    with np.errstate(invalid="ignore"):
        inside = sigma > level
    P = nx * ny * nz
    # ---- vertices: edge class c of point p crosses iff p + d is on the lattice and the two ends differ
    cross = np.zeros((nx, ny, nz, 7), dtype=bool)
    for c in range(7):
        dx, dy, dz = ((c + 1) >> 2) & 1, ((c + 1) >> 1) & 1, (c + 1) & 1
        a = inside[:nx - dx, :ny - dy, :nz - dz]
        b = inside[dx:, dy:, dz:]
        cross[:nx - dx, :ny - dy, :nz - dz, c] = a != b
    flat = cross.reshape(-1)
    vid = (np.cumsum(flat) - flat).reshape(nx, ny, nz, 7)          # id of the vertex of (p, c) where it exists
    pc = np.nonzero(flat)[0]
    p, c = pc // 7, pc % 7
    i, j, k = p // (ny * nz), (p // nz) % ny, p % nz
    d = np.stack([((c + 1) >> 2) & 1, ((c + 1) >> 1) & 1, (c + 1) & 1], -1)
    sp = sigma[i, j, k].astype(np.float64)
    sq = sigma[i + d[:, 0], j + d[:, 1], k + d[:, 2]].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (np.float64(level) - sp) / (sq - sp)
        verts = np.empty((len(p), 3), dtype=np.float64)
        for a, idx in enumerate((i, j, k)):
            g0 = g[a][idx].astype(np.float64)
            g1 = g[a][idx + d[:, a]].astype(np.float64)
            verts[:, a] = np.where(d[:, a] == 1, g0 + t * (g1 - g0), g0)
    # ---- triangles: per cell, tetrahedron, piece
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    corner = {}
    for bits in range(8):
        dx, dy, dz = (bits >> 2) & 1, (bits >> 1) & 1, bits & 1
        corner[bits] = (slice(dx, dx + cx), slice(dy, dy + cy), slice(dz, dz + cz))
    faces = np.full((cx, cy, cz, 6, 2, 3), -1, dtype=np.int64)
    vid_at = np.stack([vid[corner[b]] for b in range(8)], 0)     # (8, cx, cy, cz, 7): the ids owned by each cell corner
    ci, cj, ck = np.meshgrid(np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij")
    for tt, perm in enumerate(PERMS):
        v = path(perm)
        case = np.zeros((cx, cy, cz), dtype=np.int64)
        for m in range(4):
            bits = 4 * v[m][0] + 2 * v[m][1] + v[m][2]
            case |= inside[corner[int(bits)]].astype(np.int64) << m
        for n in range(2):
            valid = _CNT[tt][case] > n
            for s in range(3):
                own = _OWN[tt][case, n, s]
                cl = _CLS[tt][case, n, s]
                ids = vid_at[own, ci, cj, ck, cl]
                faces[:, :, :, tt, n, s] = np.where(valid, ids, -1)
    faces = faces.reshape(-1, 3)
    faces = faces[faces[:, 0] >= 0]
    return verts, faces, np.stack([p, c], -1)


def rotate_smallest_first(faces):
    """each row rotated (not reflected) so that its smallest index comes first"""
    faces = np.asarray(faces)
    if len(faces) == 0:
        return faces
    k = np.argmin(faces, axis=1)
    r = np.arange(len(faces))
    return np.stack([faces[r, k], faces[r, (k + 1) % 3], faces[r, (k + 2) % 3]], -1)


def sphere_volume(n=None, shape=None, coords=None, center=(0.03, -0.02, 0.05), radius=0.7):
    """radius - |x - center| as fp32 with its coordinate arrays: on linspace(-1, 1, n)^3, on linspace(-1, 1, shape[a]) per axis,
    or on the three given coordinate arrays"""
    if coords is None:
        coords = [np.linspace(-1.0, 1.0, m) for m in (shape or (n, n, n))]
    g = [np.asarray(a).astype(np.float32) for a in coords]
    X, Y, Z = np.meshgrid(*[a.astype(np.float64) for a in g], indexing="ij")
    r = np.sqrt((X - center[0]) ** 2 + (Y - center[1]) ** 2 + (Z - center[2]) ** 2)
    return (radius - r).astype(np.float32), g


def mesh_invariants(verts, faces):
    """-> dict(closed, euler, all_used, volume, area) of an indexed triangle mesh"""
    e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    key = e[:, 0] * (len(verts) + 1) + e[:, 1]
    rkey = e[:, 1] * (len(verts) + 1) + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    closed = bool((counts == 1).all() and np.array_equal(np.sort(rkey), uniq))
    E = len(uniq) // 2
    p0, p1, p2 = (verts[faces[:, s]] for s in range(3))
    cr = np.cross(p1 - p0, p2 - p0)
    return dict(closed=closed, euler=len(verts) - E + len(faces), all_used=len(np.unique(faces)) == len(verts),
                volume=float((p0 * cr).sum() / 6.0), area=float(np.linalg.norm(cr, axis=1).sum() / 2.0))
