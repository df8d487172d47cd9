"""GPU: ops.mesh_from_volume (cips_mesh_count / cips_mesh_emit, csrc/mesh.hip) against the numpy statement of the rules
(mesh_oracle.py): faces exactly and in order, positions bit for bit on the axes an edge does not move along and to rounding on
the others, outputs written completely and nowhere else, the same bits on a second call.

Volumes: the distance-to-a-sphere field of test_mesh_oracle_cpu.py and seeded normal noise — the densest surface there is: every
case of every tetrahedron occurs, and nearly every lattice point owns vertices."""
import functools

import numpy as np
import pytest
import torch

import mesh_oracle as mo

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
PAD = 16


def dev():
    return torch.device("cuda")


def _coords(shape, uniform, seed):
    if uniform:
        return [np.linspace(-1.0, 1.0, m).astype(np.float32) for m in shape]
    g = torch.Generator().manual_seed(seed)           # no regularity the kernel could lean on; strictly increasing
    out = []
    for m in shape:
        c = torch.sort(torch.rand(m, generator=g) * 2 - 1).values.numpy().astype(np.float32)
        assert (np.diff(c) > 0).all()
        out.append(c)
    return out


def _noise(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).numpy()


# name -> (shape, volume kind, uniform coordinates, level).  A workgroup takes a run of 1 024 lattice points, each of its four
# waves 256 consecutive ones in four groups of 64; the scan's first level takes 512 runs per chunk:
#   cell      a single cell, 8 points in one ragged group
#   odd       non-cubic, non-uniform coordinates (a swapped axis shows), less than one wave
#   cube17    4 913 points: five runs, the last with a ragged group and empty waves
#   longrow   a row of 300 > 64 points: a group's lanes sit in up to two rows, and rows cross group, wave and run boundaries
#   scan2     526 500 points = 515 runs > 512: the scan's second level adds a chunk offset, on dense counts
#   cube96    884 736 points = 864 runs, mostly empty ones around a sphere
CASES = {
    "cell-noise": ((2, 2, 2), "noise", True, 0.0),
    "odd-noise": ((5, 3, 7), "noise", False, 0.1),
    "odd-sphere": ((5, 3, 7), "sphere", False, 0.0),
    "cube17-sphere": ((17, 17, 17), "sphere", True, 0.0),
    "cube17-noise": ((17, 17, 17), "noise", True, -0.2),
    "longrow-sphere": ((9, 9, 300), "sphere", True, 0.0),
    "longrow-noise": ((9, 9, 300), "noise", False, 0.0),
    "scan2-noise": ((9, 9, 6500), "noise", True, 0.3),
    "cube96-sphere": ((96, 96, 96), "sphere", True, 0.0),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(sigma, coordinates, level, oracle vertices, faces, (p, c)) — computed once, never modified"""
    shape, kind, uniform, level = CASES[name]
    g = _coords(shape, uniform, seed=len(name))
    sigma = mo.sphere_volume(coords=g)[0] if kind == "sphere" else _noise(shape, seed=7 + len(name))
    verts, faces, pc = mo.marching_tetrahedra(sigma, *g, level)
    for a in (sigma, verts, faces, pc, *g):
        a.setflags(write=False)
    return sigma, g, level, verts, faces, pc


def _padded(nv, nt, nan_head=True):
    v = torch.full((nv + PAD, 3), float("nan") if nan_head else SENTINEL, device=dev())
    v[nv:] = SENTINEL
    f = torch.full((nt + PAD, 3), -7, dtype=torch.int32, device=dev())
    return v, f


def _check_mesh(vertices, faces, sigma_shape, g, verts_ref, faces_ref, pc):
    """one image's mesh against the oracle's"""
    assert vertices.dtype == torch.float32 and faces.dtype == torch.int32
    assert tuple(vertices.shape) == (len(verts_ref), 3) and tuple(faces.shape) == (len(faces_ref), 3)
    own_f = mo.rotate_smallest_first(faces.cpu().numpy().astype(np.int64))
    assert torch.equal(torch.from_numpy(own_f), torch.from_numpy(mo.rotate_smallest_first(faces_ref)))
    if not len(verts_ref):
        return
    own_v = vertices.cpu().numpy()
    nx, ny, nz = sigma_shape
    p, c = pc[:, 0], pc[:, 1]
    idx = (p // (ny * nz), (p // nz) % ny, p % nz)
    for a in range(3):
        moves = (((c + 1) >> (2 - a)) & 1).astype(bool)
        g0 = g[a][idx[a]]
        # an axis the edge does not move along: the lattice coordinate bit for bit
        assert np.array_equal(own_v[~moves, a].view(np.int32), g0[~moves].view(np.int32)), a
        # elsewhere: three roundings in t and two in the coordinate, each at most 2^-24 of a magnitude below step + max|g|
        # (8: either fma contraction); NaN where the oracle has NaN (non-finite sigma)
        step = (g[a][np.minimum(idx[a] + 1, len(g[a]) - 1)] - g0).astype(np.float64)
        bound = 8 * 2.0 ** -24 * (step + np.abs(g[a]).max())
        ref, own = verts_ref[moves, a], own_v[moves, a].astype(np.float64)
        assert np.array_equal(np.isnan(ref), np.isnan(own)), a
        ok = ~np.isnan(ref)
        assert (np.abs(own - ref)[ok] <= bound[moves][ok]).all(), (a, float(np.abs(own - ref)[ok].max()))


@pytest.mark.parametrize("name", list(CASES))
def test_mesh_equals_the_oracle(name):
    from cips3d_amd import ops
    sigma, g, level, verts_ref, faces_ref, pc = _case(name)
    assert len(verts_ref) > 0 and len(faces_ref) > 0                 # not vacuous
    s = torch.from_numpy(sigma.copy()).to(dev()).unsqueeze(0)
    gd = [torch.from_numpy(a.copy()).to(dev()) for a in g]
    vbuf, fbuf = _padded(len(verts_ref), len(faces_ref))
    (vertices, faces), = ops.mesh_from_volume(s, *gd, level, out=(vbuf, fbuf))
    torch.cuda.synchronize()
    assert vertices.data_ptr() == vbuf.data_ptr() and faces.data_ptr() == fbuf.data_ptr()       # views of the packed outputs
    _check_mesh(vertices, faces, sigma.shape, g, verts_ref, faces_ref, pc)
    assert not torch.isnan(vbuf[:len(verts_ref)]).any()              # every element written (the buffer was NaN) ...
    assert bool((fbuf[:len(faces_ref)] >= 0).all())
    assert bool((vbuf[len(verts_ref):] == SENTINEL).all()) and bool((fbuf[len(faces_ref):] == -7).all())   # ... none behind
    (v2, f2), = ops.mesh_from_volume(s, *gd, level)                  # a second call, fresh outputs: the same bits
    assert torch.equal(v2.view(torch.int32), vertices.view(torch.int32)) and torch.equal(f2, faces)
    assert v2.grad_fn is None and not v2.requires_grad


def test_batch_with_an_empty_image_in_the_middle():
    """B = 3: noise, a volume without a crossing, the sphere — per-image offsets into the packed outputs, indices local to each
    image, (0, 3) tensors for the empty one"""
    from cips3d_amd import ops
    n = 17
    sphere, g = mo.sphere_volume(n)
    vols = [_noise((n, n, n), 21), np.full((n, n, n), -1.0, dtype=np.float32), sphere]
    refs = [mo.marching_tetrahedra(v, *g, 0.0) for v in vols]
    assert len(refs[0][0]) > 0 and len(refs[1][0]) == 0 and len(refs[1][1]) == 0 and len(refs[2][0]) > 0
    s = torch.from_numpy(np.stack(vols)).to(dev())
    gd = [torch.from_numpy(a.copy()).to(dev()) for a in g]
    nv, nt = sum(len(r[0]) for r in refs), sum(len(r[1]) for r in refs)
    vbuf, fbuf = _padded(nv, nt)
    meshes = ops.mesh_from_volume(s, *gd, 0.0, out=(vbuf, fbuf))
    torch.cuda.synchronize()
    assert len(meshes) == 3
    for (vertices, faces), (verts_ref, faces_ref, pc) in zip(meshes, refs):
        _check_mesh(vertices, faces, (n, n, n), g, verts_ref, faces_ref, pc)
    assert tuple(meshes[1][0].shape) == (0, 3) and tuple(meshes[1][1].shape) == (0, 3)
    assert meshes[2][0].data_ptr() == vbuf.data_ptr() + 12 * len(refs[0][0])        # packed one after the other
    assert not torch.isnan(vbuf[:nv]).any() and bool((fbuf[:nt] >= 0).all())
    assert bool((vbuf[nv:] == SENTINEL).all()) and bool((fbuf[nt:] == -7).all())
    # all images empty: no emit launch, (0, 3) tensors
    empty = ops.mesh_from_volume(s[1:2].contiguous(), *gd, 0.0)
    assert tuple(empty[0][0].shape) == (0, 3) and tuple(empty[0][1].shape) == (0, 3) and empty[0][1].dtype == torch.int32


def test_non_finite_values_and_values_equal_to_the_level():
    """NaN counts as outside (sigma > level is false), a value equal to the level as outside too: its vertices land on the
    lattice point (t = 0 or 1) and the degenerate triangles keep the winding the integer rule gives them.  Non-finite sigma
    makes positions meaningless (NaN here and in the oracle alike) but the counts, the faces and the bounds hold."""
    from cips3d_amd import ops
    shape, level = (11, 9, 13), 0.25
    sigma = _noise(shape, 33).copy()
    pick = torch.randperm(sigma.size, generator=torch.Generator().manual_seed(34)).numpy()
    flat = sigma.reshape(-1)
    flat[pick[:60]] = np.nan
    flat[pick[60:160]] = level
    flat[pick[160:180]] = np.inf
    flat[pick[180:200]] = -np.inf
    g = _coords(shape, False, 35)
    verts_ref, faces_ref, pc = mo.marching_tetrahedra(sigma, *g, level)
    assert np.isnan(verts_ref).any() and len(faces_ref) > 0
    on_point = (verts_ref == np.stack([g[a][(pc[:, 0] // d) % m] for a, (d, m) in
                                       enumerate(((shape[1] * shape[2], shape[0]), (shape[2], shape[1]), (1, shape[2])))], -1)).all(1)
    assert on_point.any()                                            # vertices at t = 0 exist
    s = torch.from_numpy(sigma).to(dev()).unsqueeze(0)
    gd = [torch.from_numpy(a.copy()).to(dev()) for a in g]
    vbuf, fbuf = _padded(len(verts_ref), len(faces_ref), nan_head=False)
    (vertices, faces), = ops.mesh_from_volume(s, *gd, level, out=(vbuf, fbuf))
    torch.cuda.synchronize()
    _check_mesh(vertices, faces, shape, g, verts_ref, faces_ref, pc)
    assert not bool((vbuf[:len(verts_ref)] == SENTINEL).any()) and bool((fbuf[:len(faces_ref)] >= 0).all())
    assert bool((vbuf[len(verts_ref):] == SENTINEL).all()) and bool((fbuf[len(faces_ref):] == -7).all())
    (v2, f2), = ops.mesh_from_volume(s, *gd, level)
    assert torch.equal(v2.view(torch.int32), vertices.view(torch.int32)) and torch.equal(f2, faces)


def test_inputs_are_checked():
    from cips3d_amd import ops
    sigma, g = mo.sphere_volume(5)
    s = torch.from_numpy(sigma).unsqueeze(0)
    gd = [torch.from_numpy(a) for a in g]
    with pytest.raises(RuntimeError, match="GPU"):
        ops.mesh_from_volume(s, *gd, 0.0)
    s, gd = s.to(dev()), [a.to(dev()) for a in gd]
    with pytest.raises(RuntimeError, match="fp32"):
        ops.mesh_from_volume(s.double(), *gd, 0.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.mesh_from_volume(s.transpose(1, 3), *gd, 0.0)
    with pytest.raises(ValueError, match="increasing"):
        ops.mesh_from_volume(s, gd[0].flip(0).contiguous(), gd[1], gd[2], 0.0)
    with pytest.raises(ValueError, match="increasing"):
        ops.mesh_from_volume(s, gd[0], torch.cat([gd[1][:2], gd[1][1:4]]), gd[2], 0.0)      # a repeated coordinate
    with pytest.raises(ValueError):
        ops.mesh_from_volume(s[0], *gd, 0.0)
    with pytest.raises(ValueError):
        ops.mesh_from_volume(s, gd[0][:4].contiguous(), gd[1], gd[2], 0.0)
    with pytest.raises(ValueError, match="out of range"):
        ops.mesh_from_volume(s[:, :1].contiguous(), gd[0][:1].contiguous(), gd[1], gd[2], 0.0)
    with pytest.raises(ValueError, match="out must be"):
        ops.mesh_from_volume(s, *gd, 0.0, out=_padded(0, 0)[:1] + (torch.empty(1, 3, dtype=torch.int32, device=dev()),))
