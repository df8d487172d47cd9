"""CPU: evaluation.save_ply with vertex colours — round trip through a numpy PLY parser, the quantisation rule, the file without
colours byte for byte what the writer produced before colours existed, and the refusal of colours of the wrong shape; and
evaluation.shade_surface(albedo=True) on a hand-made surface."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from color_refs import quantise_u8, read_ply


def _mesh(V=37, T=50, seed=3):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(V, 3, generator=g)
    n = torch.nn.functional.normalize(torch.randn(V, 3, generator=g), dim=-1)
    f = torch.randint(0, V, (T, 3), generator=g, dtype=torch.int32)
    c = torch.rand(V, 3, generator=g) * 2.4 - 1.2                     # beyond [-1, 1] on both sides: the clamp shows
    c[0] = torch.tensor([-1.0, 0.0, 1.0])
    c[1] = torch.tensor([-0.99, 0.99999994, -0.99999994])              # next to the ends of the range: 1.775, 255.5-, 0.5+
    return v, f, n, c


def _ply_without_colours(vertices, faces, normals=None):
    """the bytes of the writer as it was before colours: header, float rows, (uchar 3, int x 3) rows"""
    v = np.ascontiguousarray(vertices.numpy().astype("<f4"))
    f = np.ascontiguousarray(faces.numpy().astype("<i4"))
    cols, props = [v], ["property float x", "property float y", "property float z"]
    if normals is not None:
        cols.append(np.ascontiguousarray(normals.numpy().astype("<f4")))
        props += ["property float nx", "property float ny", "property float nz"]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", *props, f"element face {len(f)}",
              "property list uchar int vertex_indices", "end_header"]
    rows = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    rows["n"] = 3
    rows["i"] = f
    return ("\n".join(header) + "\n").encode("ascii") + np.ascontiguousarray(np.concatenate(cols, 1)).tobytes() + rows.tobytes()


@pytest.mark.parametrize("with_normals", [True, False])
def test_save_ply_colours_round_trip(tmp_path, with_normals):
    from cips3d_amd.evaluation import save_ply
    v, f, n, c = _mesh()
    p = str(tmp_path / "mesh.ply")
    save_ply(p, v, f, n if with_normals else None, colors=c)
    names, cols, face = read_ply(p)
    assert names == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + ["red", "green", "blue"]
    assert np.array_equal(np.stack([cols[k] for k in "xyz"], 1), v.numpy())
    if with_normals:
        assert np.array_equal(np.stack([cols[k] for k in ("nx", "ny", "nz")], 1), n.numpy())
    got = np.stack([cols[k] for k in ("red", "green", "blue")], 1)
    assert got.dtype == np.uint8 and np.array_equal(got, quantise_u8(c.numpy()))
    assert got[0].tolist() == [0, 128, 255] and got[1].tolist() == [1, 255, 0]          # 127.5 + 0.5 truncates to 128
    assert got.min() == 0 and got.max() == 255                                           # values beyond the range are clamped
    assert np.array_equal(face, f.numpy())
    # numpy arrays are taken too, and an empty mesh writes an empty, well-formed file
    save_ply(p, v.numpy(), f.numpy(), colors=c.numpy())
    assert np.array_equal(np.stack([read_ply(p)[1][k] for k in ("red", "green", "blue")], 1), got)
    save_ply(p, torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), colors=torch.zeros(0, 3))
    names, cols, face = read_ply(p)
    assert names[-3:] == ["red", "green", "blue"] and len(cols["red"]) == 0 and len(face) == 0


def test_save_ply_without_colours_is_byte_identical_to_the_earlier_writer(tmp_path):
    from cips3d_amd.evaluation import save_ply
    v, f, n, _ = _mesh(seed=4)
    p = str(tmp_path / "mesh.ply")
    save_ply(p, v, f, n)
    assert open(p, "rb").read() == _ply_without_colours(v, f, n)
    save_ply(p, v, f)
    assert open(p, "rb").read() == _ply_without_colours(v, f)
    save_ply(p, v, f, n, colors=None)
    assert open(p, "rb").read() == _ply_without_colours(v, f, n)


def test_save_ply_refuses_colours_of_the_wrong_shape(tmp_path):
    from cips3d_amd.evaluation import save_ply
    v, f, n, c = _mesh()
    p = str(tmp_path / "mesh.ply")
    for bad in (c[:-1], c[:, :2], c.reshape(-1), torch.cat([c, c[:, :1]], 1)):
        with pytest.raises(ValueError):
            save_ply(p, v, f, n, colors=bad)


def test_shade_surface_albedo_on_a_hand_made_surface():
    """CPU tensors: shade_surface is tensor arithmetic.  A lit white pixel, a lit coloured pixel, a pixel facing away (ambient
    only) and a background pixel."""
    from cips3d_amd.evaluation import shade_surface
    nrm = torch.tensor([[0., 0., 1.], [0., 0., 1.], [0., 0., -1.], [0., 0., 0.]]).t().reshape(1, 3, 2, 2)
    rgb = torch.tensor([[1., 1., 1.], [1., 0., -1.], [1., 1., 1.], [-1., -1., -1.]]).t().reshape(1, 3, 2, 2)
    mask = torch.tensor([1, 1, 2, 0], dtype=torch.uint8).reshape(1, 1, 2, 2)
    s = SimpleNamespace(normals=nrm, mask=mask, rgb=rgb)
    grey = shade_surface(s)
    assert torch.equal(grey, shade_surface(SimpleNamespace(normals=nrm, mask=mask)))               # the default ignores .rgb
    assert torch.equal(shade_surface(SimpleNamespace(normals=nrm, mask=mask), albedo=True), grey)  # and albedo needs one
    out = shade_surface(s, albedo=True, ambient=0.2).reshape(3, 4).t()
    assert out.shape == (4, 3)
    assert torch.allclose(out[0], torch.tensor([1., 1., 1.]))                  # white albedo, fully lit
    assert torch.allclose(out[1], torch.tensor([1., 0., -1.]))                 # fully lit: the colour itself
    assert torch.allclose(out[2], torch.full((3,), 0.2 * 2 - 1))               # facing away: ambient times white
    assert torch.equal(out[3], torch.full((3,), -1.))                          # background
    assert torch.allclose(grey.reshape(3, 4).t()[0], out[0]) and float(out.min()) >= -1 and float(out.max()) <= 1
