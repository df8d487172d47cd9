"""GPU: colours on the generator's geometry — GeneratorNerfINR.extract_mesh(colors=...) and .surface_colored(...) against
point_colors at the vertices / surface points, with geometry and RNG draws left as the colourless calls leave them, the PLY file
of a coloured mesh, evaluation.shade_surface(albedo=True), and the generator_v1 and freeze variants."""
import numpy as np
import pytest
import torch

from color_refs import quantise_u8, read_ply
from conftest import max_rel, seeded_generator
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu
FOV, T0, T1 = 12, 0.88, 1.12
KW = dict(img_size=16, fov=FOV, ray_start=T0, ray_end=T1, num_steps=12, h_stddev=0.3, v_stddev=0.155, sample_dist="gaussian")


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _zs(seed, b=2):
    g = torch.Generator().manual_seed(seed)
    return {"z_nerf": torch.randn(b, 256, generator=g).to(dev()), "z_inr": torch.randn(b, 512, generator=g).to(dev())}


def _rng_state():
    return torch.get_rng_state().clone(), torch.cuda.get_rng_state().clone()


def _same_state(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _colors_at_vertices(G, zs, meshes, center, **kw):
    """point_colors at every mesh's vertices in ONE call on the same latents (the mapping networks see the batch they saw in
    extract_mesh): image b's vertices in row b, padded with the lattice centre -> list of (V_b, 3)"""
    pts = torch.tensor(center, device=dev()).repeat(len(meshes), max(m.vertices.shape[0] for m in meshes), 1)
    for b, m in enumerate(meshes):
        pts[b, :m.vertices.shape[0]] = m.vertices
    rgb = G.point_colors(zs, pts, **kw)
    return [rgb[b, :m.vertices.shape[0]] for b, m in enumerate(meshes)]


@pytest.mark.parametrize("psi", [1.0, 0.7])
def test_extract_mesh_aux_colours(psi, x3, tmp_path):
    """resolution 24, two images, the level of the existing mesh tests (the volume's median): colours are point_colors at the
    vertices with that image's latents; vertices, faces, normals and the RNG state are those of the colourless call; a level
    above the volume's maximum gives empty meshes with (0, 3) colours; the PLY file carries the colours"""
    from cips3d_amd.evaluation import save_ply
    G = seeded_generator(8, device=dev())
    zs = _zs(82)
    N, L, c = 24, 0.3, (0.01, -0.02, 0.0)
    torch.manual_seed(5)
    vol = G.density_grid(zs, resolution=N, cube_length=L, center=c, psi=psi)
    level = float(vol.median())
    torch.manual_seed(5)
    plain = G.extract_mesh(zs, level, resolution=N, cube_length=L, center=c, psi=psi)
    after_plain = _rng_state()
    assert all(not hasattr(m, "colors") for m in plain)
    torch.manual_seed(5)
    meshes = G.extract_mesh(zs, level, resolution=N, cube_length=L, center=c, psi=psi, colors='aux')
    assert _same_state(_rng_state(), after_plain)
    assert len(meshes) == 2 and all(m.vertices.shape[0] > 0 for m in meshes)
    torch.manual_seed(5)                                                        # psi < 1: the same 10 000 draws again
    ref = _colors_at_vertices(G, zs, meshes, c, psi=psi)
    for m, p, r in zip(meshes, plain, ref):
        assert torch.equal(m.vertices, p.vertices) and torch.equal(m.faces, p.faces) and torch.equal(m.normals, p.normals)
        assert m.colors.shape == m.vertices.shape and m.colors.dtype == torch.float32 and m.colors.grad_fn is None
        assert torch.isfinite(r).all() and torch.equal(m.colors, r)
        assert float(m.colors.abs().max()) <= 1.0 and float(m.colors.std()) > 0
    assert not torch.equal(meshes[0].colors[:8], meshes[1].colors[:8])          # each image its own latents
    empty = G.extract_mesh(zs, float(vol.max()) + 1.0, resolution=N, cube_length=L, center=c, colors='aux')
    assert all(m.vertices.shape == (0, 3) and m.colors.shape == (0, 3) and m.colors.dtype == torch.float32 for m in empty)
    if psi == 1.0:
        m = meshes[0]
        p = str(tmp_path / "mesh.ply")
        save_ply(p, m.vertices, m.faces, m.normals, m.colors)
        names, cols, face = read_ply(p)
        assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
        assert np.array_equal(np.stack([cols[k] for k in "xyz"], 1), m.vertices.cpu().numpy())
        assert np.array_equal(np.stack([cols[k] for k in ("red", "green", "blue")], 1), quantise_u8(m.colors.cpu().numpy()))
        assert np.array_equal(face, m.faces.cpu().numpy())
        with pytest.raises(ValueError):
            G.extract_mesh(zs, level, resolution=N, colors='head')              # img_size missing
        with pytest.raises(ValueError):
            G.extract_mesh(zs, level, resolution=N, colors='vertex')


def test_extract_mesh_head_colours(x3):
    """'head': the geometry of the colourless call (psi = 1: the same NeRF styles) and point_colors(mode='head') at the vertices"""
    G = seeded_generator(8, device=dev())
    zs = _zs(82)
    N, c = 17, (0., 0., 0.)
    level = float(G.density_grid(zs, resolution=N).median())
    plain = G.extract_mesh(zs, level, resolution=N)
    meshes = G.extract_mesh(zs, level, resolution=N, colors='head', img_size=32)
    ref = _colors_at_vertices(G, zs, meshes, c, mode='head', img_size=32)
    for m, p, r in zip(meshes, plain, ref):
        assert torch.equal(m.vertices, p.vertices) and torch.equal(m.faces, p.faces) and torch.equal(m.normals, p.normals)
        assert m.colors.shape == m.vertices.shape and float(m.colors.abs().max()) <= 1.0 and torch.isfinite(m.colors).all()
        # the head's GEMMs see another row count here than in the padded reference call and may take another form (split-bf16
        # or fp32 MFMA by P % 32): not bits, the head's parity bar (TOL of tests/test_gpu_generator.py)
        assert max_rel(m.colors, r) < 1e-3


def _level_of(G, zs):
    """a level that cuts the volume the camera looks at: the median density of a coarse lattice (tests/test_gpu_surface.py)"""
    return float(np.float32(G.density_grid(zs, 9, cube_length=0.2).median().item()))


def _rows(v):                     # (b,c,H,W) -> (b,n,c)
    return v.permute(0, 2, 3, 1).reshape(v.shape[0], -1, v.shape[1])


def test_surface_aux_colours_and_albedo_shading(x3):
    """16 x 16 rays of 12 steps: rgb is the colour at .points where the mask is set and exactly -1 elsewhere; every other field
    and the RNG state are the colourless call's; only the NeRF mapping network runs; shade_surface(albedo=True)"""
    from cips3d_amd.evaluation import shade_surface
    d = dev()
    G = seeded_generator(13, device=d)
    zs = _zs(131)
    level = _level_of(G, zs)
    torch.manual_seed(7)
    plain = G.surface(zs, level, **KW, refine=5)
    after_plain = _rng_state()
    assert not hasattr(plain, "rgb")
    calls, inr = [], G._map_inr
    G._map_inr = lambda z: (calls.append(1), inr(z))[1]
    try:
        torch.manual_seed(7)
        sf = G.surface_colored(zs, level, **KW, refine=5, colors='aux')
    finally:
        del G._map_inr
    assert not calls and _same_state(_rng_state(), after_plain)
    for nm in ("depth", "mask", "points", "sigma", "normals", "pitch_yaw"):
        assert torch.equal(getattr(sf, nm), getattr(plain, nm)), nm
    b, H = 2, KW["img_size"]
    assert sf.rgb.shape == (b, 3, H, H) and sf.rgb.dtype == torch.float32 and sf.rgb.grad_fn is None
    mask, rgb = _rows(sf.mask).squeeze(-1), _rows(sf.rgb)
    assert bool((mask != 0).any()) and bool((mask == 0).any()), "the level must cut the view"
    ref = G.point_colors(zs, _rows(sf.points).contiguous())
    assert torch.isfinite(ref).all() and torch.equal(rgb[mask != 0], ref[mask != 0])
    assert bool((rgb[mask == 0] == -1).all())

    torch.manual_seed(7)
    none = G.surface_colored(zs, level, **KW, refine=5, colors=None)             # surface() itself
    assert not hasattr(none, "rgb") and torch.equal(none.depth, plain.depth) and _same_state(_rng_state(), after_plain)

    grey = shade_surface(plain)
    assert torch.equal(shade_surface(sf), grey)                                 # the default call is unchanged by .rgb
    img = shade_surface(sf, albedo=True)
    assert img.shape == (b, 3, H, H) and float(img.min()) >= -1 and float(img.max()) <= 1
    assert bool((_rows(img)[mask == 0] == -1).all())
    lit = (_rows(grey)[..., :1] + 1) * 0.5                                       # the Lambert factor of every pixel
    want = ((rgb + 1) * 0.5 * lit * 2 - 1)[mask != 0]
    assert float((_rows(img)[mask != 0] - want).abs().max()) < 1e-6
    assert not torch.equal(img[:, 0], img[:, 1])                                 # a colour picture

    # 'head': the INR head at the depth of the image size, which must reach the first ToRGB (32)
    kw32 = dict(KW, img_size=32, num_steps=6)
    torch.manual_seed(7)
    plain32 = G.surface(zs, level, **kw32, refine=5)
    torch.manual_seed(7)                                                         # psi = 1: the styles draw nothing
    sf_h = G.surface_colored(zs, level, **kw32, refine=5, colors='head')
    mask_h = _rows(sf_h.mask).squeeze(-1)
    assert torch.equal(sf_h.depth, plain32.depth) and torch.equal(sf_h.normals, plain32.normals)
    assert sf_h.rgb.shape == (b, 3, 32, 32) and float(sf_h.rgb.abs().max()) <= 1.0
    ref_h = G.point_colors(zs, _rows(sf_h.points).contiguous(), mode='head', img_size=32)
    assert bool((mask_h != 0).any()) and torch.equal(_rows(sf_h.rgb)[mask_h != 0], ref_h[mask_h != 0])
    assert bool((_rows(sf_h.rgb)[mask_h == 0] == -1).all())
    with pytest.raises(ValueError):
        G.surface_colored(zs, level, **KW, colors='head')                        # 16 < 32: a head without a ToRGB
    with pytest.raises(ValueError):
        G.surface_colored(zs, level, **KW, colors='lambert')


@pytest.mark.parametrize("variant", ["v1", "freeze"])
def test_variants_colour_their_geometry(variant, x3):
    """generator_v1 (its colour style is a head of the INR mapping network: both mapping networks run) and the freeze variant,
    'aux' mode: point_colors against ops.siren_rgb on the documented styles, a coloured mesh and a coloured surface"""
    from test_generator_v1_cpu import seeded_generator_v1
    ops = x3
    d = dev()
    G = seeded_generator_v1(9, device=d) if variant == "v1" else seeded_generator(9, freeze=True, device=d)
    zs = _zs(91)
    pts = ((torch.rand(2, 77, 3, generator=torch.Generator().manual_seed(92)) - 0.5) * 0.3).to(d)
    rgb = G.point_colors(zs, pts)
    with torch.no_grad():
        styles = G.mapping_network(**zs) if variant == "v1" else G._map_nerf(zs["z_nerf"])
        ref = ops.siren_rgb(pts, G.aux_to_rbg[0].weight, G.aux_to_rbg[0].bias, *G.siren._siren_args(styles))
    assert rgb.shape == (2, 77, 3) and rgb.grad_fn is None and torch.isfinite(ref).all() and torch.equal(rgb, ref)
    vol, sigma = G.color_grid(zs, resolution=5, return_sigma=True)
    assert vol.shape == (2, 5, 5, 5, 3) and torch.equal(sigma, G.density_grid(zs, resolution=5))
    N = 17
    level = float(G.density_grid(zs, resolution=N).median())
    plain = G.extract_mesh(zs, level, resolution=N)
    meshes = G.extract_mesh(zs, level, resolution=N, colors='aux')
    for m, p, r in zip(meshes, plain, _colors_at_vertices(G, zs, meshes, (0., 0., 0.))):
        assert m.vertices.shape[0] > 0 and torch.equal(m.vertices, p.vertices) and torch.equal(m.faces, p.faces)
        assert torch.equal(m.colors, r) and float(m.colors.abs().max()) <= 1.0
    kw = dict(KW, img_size=8, num_steps=6)
    sf = G.surface_colored(zs, _level_of(G, zs), **kw)                           # colors='aux' is the default
    mask = _rows(sf.mask).squeeze(-1)
    ref = G.point_colors(zs, _rows(sf.points).contiguous())
    assert torch.equal(_rows(sf.rgb)[mask != 0], ref[mask != 0]) and bool((_rows(sf.rgb)[mask == 0] == -1).all())
