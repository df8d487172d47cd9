"""GPU: evaluation.render_mesh and evaluation.orbit_cameras on the meshes of GeneratorNerfINR.extract_mesh — a random small
generator, resolution 17, auxiliary colours — against the fp64 yardstick (tests/raster_oracle.py) run on the downloaded mesh,
through shade_surface and save_image, and next to GeneratorNerfINR.surface of the same level and camera.

The agreement of render_mesh(extract_mesh(level)) with surface(level) is PRINTED, not asserted: how far marching tetrahedra at
N = 17 lie from the true level set of a random SIREN is not derivable.

MEASURED on an MI355X (`pytest -s` prints every figure):
  the two meshes (V 2832 / 2376, T 5328 / 4454; 91 % and 76 % of the 3 x 16^2 pixels covered, kappa 1.5): depth within 0.12 of its
  bar, lambda within 0.004; 18 and 10 margin pixels of 768, none decided otherwise than by the nominal oracle
  orbit_cameras and surface()'s cam2world: 4e-8 .. 7e-8 from the fp64 composition (bar 1.9e-6)
  against surface(level) from rays 0.7 .. 1.3 (six views): the masks agree on 70 - 94 % of the pixels, and where both hit the
  median |depth difference| is 11 - 18 lattice cells: the untrained field has density outside the lattice's cube, which the ray
  meets first.  Of the 0 - 22 pixels per view whose crossing lies inside the cube the mesh is hit at every one, and the depths
  agree to a median of 0.02 - 0.07 lattice cells (profiles/raster.txt; at N = 256: 0.017 cells)
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import raster_oracle as ro
from conftest import seeded_generator

pytestmark = pytest.mark.gpu
FOV, N, L = 12, 17, 0.3
YAWS, PITCHES = [1.2, math.pi / 2, 1.9], [1.45, math.pi / 2, 1.7]


def dev():
    return torch.device("cuda")


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _zs(seed, b=2):
    g = torch.Generator().manual_seed(seed)
    return {"z_nerf": torch.randn(b, 256, generator=g).to(dev()), "z_inr": torch.randn(b, 512, generator=g).to(dev())}


def _meshes(G, zs):
    level = float(G.density_grid(zs, resolution=N, cube_length=L).median())
    meshes = G.extract_mesh(zs, level, resolution=N, cube_length=L, colors='aux')
    assert all(m.vertices.shape[0] > 0 and m.faces.shape[0] > 0 for m in meshes)
    return level, meshes


def test_render_mesh_against_the_oracle_and_through_the_picture_tools(x3, tmp_path):
    from cips3d_amd import evaluation
    from cips3d_amd.generator import _zc
    G = seeded_generator(8, device=dev())
    _, meshes = _meshes(G, _zs(82))
    cams = evaluation.orbit_cameras(YAWS, PITCHES, device=dev())
    for i, mesh in enumerate(meshes):
        out = evaluation.render_mesh(mesh, cams, FOV, 16)
        assert out.depth.shape == (3, 1, 16, 16) and out.mask.shape == (3, 1, 16, 16) and out.mask.dtype == torch.uint8
        assert out.points.shape == out.normals.shape == out.rgb.shape == (3, 3, 16, 16) and out.cam2world is cams
        case = ro.make_case(mesh.vertices.cpu(), mesh.faces.cpu(), evaluation.world2cam(cams).cpu(), FOV, 16, 16, zc=_zc(FOV))
        r = ro.run(case)
        q = ro.compare(case, r, out.face, out.bary, out.depth[:, 0], out.mask[:, 0])
        print(f"mesh {i} (V {mesh.vertices.shape[0]}, T {mesh.faces.shape[0]}): depth {q.depth:.4f} of its bar, lambda {q.lam:.4f}; "
              f"{q.margin} margin pixels of {r.margin.numel()} ({q.otherwise} decided otherwise), {q.exempt} took the runner-up, "
              f"kappa {ro.condition(case):.2f}, covered {float(r.mask.float().mean()):.3f}")
        assert q.depth <= 1 and q.lam <= 1
        assert out.mask.any() and (out.mask == 0).any()
        hit = (out.mask == 1).expand(-1, 3, -1, -1)
        # normals: unit where hit, exact zeros on the background; colours: inside the hull of the vertex colours, -1 outside
        assert float((out.normals.norm(dim=1, keepdim=True)[out.mask == 1] - 1).abs().max()) <= 1e-5 and not out.normals[~hit].any()
        assert bool((out.rgb[~hit] == -1).all()) and not out.points[~hit].any()
        assert float(out.rgb[hit].min()) >= float(mesh.colors.min()) - 1e-6 and float(out.rgb[hit].max()) <= float(mesh.colors.max()) + 1e-6
        # points: the interpolated vertices lie at `depth` from the camera
        dist = (out.points - cams[:, :3, 3].view(3, 3, 1, 1)).norm(dim=1, keepdim=True)
        assert float((dist - out.depth)[out.mask == 1].abs().max()) <= 1e-5
        for albedo in (False, True):
            img = evaluation.shade_surface(out, albedo=albedo)
            assert img.shape == (3, 3, 16, 16) and bool(torch.isfinite(img).all()) and bool((img[~hit] == -1).all())
            assert float(img.min()) >= -1 and float(img.max()) <= 1 and float(img[hit].max()) > -1
        path = tmp_path / f"mesh{i}.png"
        evaluation.save_image(img, str(path), nrow=3, normalize=True, value_range=(-1, 1))
        assert path.stat().st_size > 0


def test_without_vertex_normals_the_normals_are_the_face_normals(x3):
    from cips3d_amd import evaluation
    G = seeded_generator(8, device=dev())
    _, meshes = _meshes(G, _zs(82, b=1))
    mesh = meshes[0]
    cams = evaluation.orbit_cameras(YAWS[:2], PITCHES[:2], device=dev())
    full = evaluation.render_mesh(mesh, cams, FOV, 16)
    bare = evaluation.render_mesh(SimpleNamespace(vertices=mesh.vertices, faces=mesh.faces, normals=None), cams, FOV, 16)
    assert not hasattr(bare, "rgb")
    assert torch.equal(bare.face, full.face) and torch.equal(bare.depth, full.depth) and torch.equal(bare.points, full.points)
    tri = mesh.vertices.double()[mesh.faces.long()]
    fn = torch.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=-1)
    fn = fn / fn.norm(dim=-1, keepdim=True)
    want = fn[bare.face.clamp_min(0).long()].permute(0, 3, 1, 2)
    hit = (bare.mask == 1).expand(-1, 3, -1, -1)
    assert float((bare.normals.double() - want)[hit].abs().max()) <= 1e-5 and not bare.normals[~hit].any()
    # seen from outside, a front face's normal points at the camera: extract_mesh winds towards lower density
    view = (cams[:, :3, 3].view(2, 3, 1, 1) - bare.points)
    culled = evaluation.render_mesh(mesh, cams, FOV, 16, cull='back')
    front = (culled.mask == 1) & (culled.face == bare.face).unsqueeze(1)
    assert front.any() and bool(((bare.normals * view).sum(1, keepdim=True)[front] > 0).all())


def test_an_empty_mesh_is_the_background():
    from cips3d_amd import evaluation
    d = dev()
    cams = evaluation.orbit_cameras([1.0, 2.0], device=d)
    empty = SimpleNamespace(vertices=torch.zeros(0, 3, device=d), faces=torch.zeros(0, 3, dtype=torch.int32, device=d),
                            normals=torch.zeros(0, 3, device=d), colors=torch.zeros(0, 3, device=d))
    for mesh in (empty, SimpleNamespace(vertices=empty.vertices, faces=empty.faces)):
        out = evaluation.render_mesh(mesh, cams, FOV, 8, far=3.0)
        assert not out.mask.any() and bool((out.depth == 3.0).all()) and bool((out.face == -1).all())
        assert not out.normals.any() and not out.points.any() and not out.bary.any()
    assert bool((evaluation.render_mesh(empty, cams, FOV, 8).rgb == -1).all())
    assert bool((evaluation.shade_surface(evaluation.render_mesh(empty, cams, FOV, 8)) == -1).all())


def test_orbit_cameras_are_the_generators_cameras(x3):
    from cips3d_amd import evaluation
    G = seeded_generator(8, device=dev())
    zs = _zs(82, b=1)
    for yaw, pitch in zip(YAWS, PITCHES):
        sf = G.surface(zs, 1.0, img_size=4, fov=FOV, ray_start=0.88, ray_end=1.12, num_steps=3, h_stddev=0., v_stddev=0.,
                       h_mean=yaw, v_mean=pitch, refine=1, normals=False, sample_dist='gaussian')
        cam = evaluation.orbit_cameras([yaw], [pitch], device=dev())
        want = torch.from_numpy(np.linalg.inv(
            torch.cat([ro.orbit_world2cam([yaw], [pitch])[0].double(), torch.tensor([[0., 0., 0., 1.]]).double()]).numpy()))
        e_gen, e_orbit = float((sf.cam2world[0].cpu().double() - want).abs().max()), float((cam[0].cpu().double() - want).abs().max())
        print(f"yaw {yaw:.3f} pitch {pitch:.3f}: surface's cam2world is {e_gen:.2e} from the fp64 composition, orbit_cameras' {e_orbit:.2e}")
        # entries of size <= 1: the fp32 angles are off by up to eps |angle| <= 2 eps each (4 eps in an entry), and the origin,
        # two normalisations, two cross products, their second normalisations and the matrix product are seven steps of three
        # to four fp32 roundings (28 eps): 32 eps against fp64, and twice that between the two fp32 routes
        assert e_gen <= 32 * ro.EPS32 and e_orbit <= 32 * ro.EPS32
        assert float((cam - sf.cam2world).abs().max()) <= 64 * ro.EPS32


def test_mesh_against_surface_is_printed(x3):
    """the first comparison of the two views of one level set: the share of pixels whose masks agree and the median |depth
    difference| in lattice cells (L / (N - 1)).  Printed, not asserted."""
    from cips3d_amd import evaluation
    G = seeded_generator(8, device=dev())
    zs = _zs(82)
    level, meshes = _meshes(G, zs)
    for yaw, pitch in zip(YAWS, PITCHES):
        # rays from 0.7 to 1.3: they start outside the lattice's cube (half diagonal 0.26), at the spacing of 24 steps over 0.24
        sf = G.surface(zs, level, img_size=16, fov=FOV, ray_start=0.7, ray_end=1.3, num_steps=61, h_stddev=0., v_stddev=0.,
                       h_mean=yaw, v_mean=pitch, sample_dist='gaussian')
        for b, mesh in enumerate(meshes):
            out = evaluation.render_mesh(mesh, sf.cam2world[b:b + 1], FOV, 16, far=1.3)
            hit_s, hit_m = sf.mask[b:b + 1] == 1, out.mask == 1
            agree = float(((sf.mask[b:b + 1] != 0) == hit_m).float().mean())
            both = hit_s & hit_m
            dd = (sf.depth[b:b + 1] - out.depth)[both].abs() / (L / (N - 1))
            med = float(dd.median()) if dd.numel() else float('nan')
            # where the ray cast's crossing lies inside the lattice's cube (the untrained field has density outside it too)
            inside = hit_s & (sf.points[b:b + 1].abs().amax(1, keepdim=True) <= L / 2)
            in_hit = float(hit_m[inside].float().mean()) if inside.any() else float('nan')
            in_dd = (sf.depth[b:b + 1] - out.depth)[inside & hit_m].abs() / (L / (N - 1))
            in_med = float(in_dd.median()) if in_dd.numel() else float('nan')
            print(f"yaw {yaw:.3f} pitch {pitch:.3f} image {b}: masks agree on {100 * agree:.1f} % of the pixels; median |depth difference| "
                  f"{med:.3f} lattice cells over {int(both.sum())} pixels (surface inside-starts: {int((sf.mask[b] == 2).sum())}); of the "
                  f"{int(inside.sum())} crossings inside the cube the mesh is hit at {100 * in_hit:.1f} %, median {in_med:.3f} cells")
            assert out.depth.shape == sf.depth[b:b + 1].shape
