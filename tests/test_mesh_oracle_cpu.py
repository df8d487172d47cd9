"""CPU: the numpy statement of the meshing rules (mesh_oracle.py) — what the HIP kernels are compared against — gives a closed,
consistently oriented sphere of the right size, and its winding rule, which reads integer lattice geometry only, agrees with the
float normal in every case of every tetrahedron."""
import math

import numpy as np
import pytest

import mesh_oracle as mo


# N -> (V, T, volume / exact, area / exact): the values the rules give for 0.7 - |x - (0.03, -0.02, 0.05)| on
# linspace(-1, 1, N)^3 at level 0.  The mesh is inscribed in the sphere (every vertex lies on a chord of the distance field's
# level set, to interpolation error), so both ratios are below 1 and rise towards it with N.
SPHERE = {9: (416, 828, 0.9365, 0.9668), 17: (1760, 3516, 0.9840, 0.9918)}


@pytest.mark.parametrize("n", sorted(SPHERE))
def test_oracle_sphere_is_a_closed_oriented_manifold_of_the_right_size(n):
    sigma, g = mo.sphere_volume(n)
    verts, faces, pc = mo.marching_tetrahedra(sigma, *g, 0.0)
    V, T, vol, area = SPHERE[n]
    assert (len(verts), len(faces)) == (V, T)
    inv = mo.mesh_invariants(verts, faces)
    assert inv["closed"]              # every directed edge once, and its reverse once
    assert inv["euler"] == 2
    assert inv["all_used"]
    assert inv["volume"] > 0          # normals point out of the inside (sigma > level) region
    assert abs(inv["volume"] / (4.0 / 3.0 * math.pi * 0.7 ** 3) - vol) <= 0.005
    assert abs(inv["area"] / (4.0 * math.pi * 0.7 ** 2) - area) <= 0.005
    # vertices come in (p, c) order
    key = pc[:, 0] * 7 + pc[:, 1]
    assert (np.diff(key) > 0).all()


def test_winding_rule_agrees_with_the_float_normal_in_all_96_cases():
    """2 x 2 x 2 lattice, every tetrahedron (6) and every inside / outside pattern of its four vertices (16): with t = 1/2 on
    every edge, each triangle's normal (P1 - P0) x (P2 - P0) points from the inside vertices' centroid to the outside ones'"""
    seen = 0
    for t, perm in enumerate(mo.PERMS):
        v = [p.astype(np.float64) for p in mo.path(perm)]
        for case in range(16):
            inside = [(case >> m) & 1 for m in range(4)]
            tris = mo.tet_triangles(perm, inside)
            n_in = sum(inside)
            assert len(tris) == min(n_in, 4 - n_in)
            if not tris:
                continue
            cin = np.mean([v[m] for m in range(4) if inside[m]], axis=0)
            cout = np.mean([v[m] for m in range(4) if not inside[m]], axis=0)
            for tri in tris:
                assert all(a < b and inside[a] != inside[b] for a, b in tri)
                P = [(v[a] + v[b]) / 2 for a, b in tri]
                normal = np.cross(P[1] - P[0], P[2] - P[0])
                assert np.linalg.norm(normal) > 0
                assert normal @ (cout - cin) > 0, (perm, case, tri)
                seen += 1
            if len(tris) == 2:      # the two pieces share the diagonal AC - BD, traversed in opposite directions
                e0 = {(tris[0][s], tris[0][(s + 1) % 3]) for s in range(3)}
                e1 = {(tris[1][(s + 1) % 3], tris[1][s]) for s in range(3)}
                assert len(e0 & e1) == 1
    assert seen == 6 * (8 * 1 + 6 * 2)


def test_the_same_cases_through_the_vectorised_path():
    """marching_tetrahedra on the single cell for all 256 corner patterns: the triangle count is the sum over the six
    tetrahedra, every face index is a valid vertex, and the mesh of a one-corner pattern is that corner's six-triangle fan"""
    g = [np.array([0.0, 1.0], dtype=np.float32)] * 3
    for bits in range(256):
        sigma = np.array([1.0 if (bits >> c) & 1 else -1.0 for c in range(8)], dtype=np.float32).reshape(2, 2, 2)
        verts, faces, pc = mo.marching_tetrahedra(sigma, *g, 0.0)
        want = 0
        for perm in mo.PERMS:
            corners = [int(4 * p[0] + 2 * p[1] + p[2]) for p in mo.path(perm)]
            want += len(mo.tet_triangles(perm, [(bits >> c) & 1 for c in corners]))
        assert len(faces) == want
        if len(faces):
            assert faces.min() >= 0 and faces.max() < len(verts)
            assert np.allclose(verts[np.isfinite(verts)], np.clip(verts[np.isfinite(verts)], 0, 1))
    sigma = -np.ones((2, 2, 2), dtype=np.float32)
    sigma[0, 0, 0] = 1.0
    verts, faces, pc = mo.marching_tetrahedra(sigma, *g, 0.0)
    assert len(verts) == 7 and len(faces) == 6 and (pc[:, 0] == 0).all() and pc[:, 1].tolist() == list(range(7))
