"""Plain-torch reference of the point colour (cips3d_amd.ops.siren_rgb, cips_siren_rgb_x3) for its tests: the 32 colour features of
tests/siren_refs.siren_ref through a 32 -> 3 linear map and, optionally, tanh — in the dtype of the call, fp64 for the kernel's
accuracy test.  The PLY parser the colour tests share lives here too (a copy of tests/test_gpu_mesh_generator.py's, which is a
`gpu` module and not imported from CPU tests), extended by uchar vertex properties."""
import numpy as np
import torch
import torch.nn.functional as F

from siren_refs import siren_ref


def rgb_ref(points, tensors, W, b, tanh=True, dtype=torch.float64):
    """points (B,P,3), tensors: the 16 SIREN tensors in siren_refs.NAMES order, W (3,32), b (3) -> rgb (B,P,3) in `dtype` on the
    CPU: rgb = [tanh](W feat + b) of siren_ref's features"""
    cast = lambda v: v.detach().to(device="cpu", dtype=dtype)
    with torch.no_grad():
        out = siren_ref(cast(points), [cast(v) for v in tensors])
        y = F.linear(out[..., :32], cast(W), cast(b))
        return torch.tanh(y) if tanh else y


def one_hot_projection(channels):
    """W (3,32) whose row j is the unit vector of channels[j], b = 0: output channel j of the kernel is feature channels[j]"""
    W = torch.zeros(3, 32)
    for j, c in enumerate(channels):
        W[j, c] = 1.0
    return W, torch.zeros(3)


def quantise_u8(c):
    """evaluation.image_to_u8's rule for value_range (-1, 1) on a numpy array, every step rounded to fp32 on its own: what
    save_ply documents for its colours"""
    c = np.asarray(c, dtype=np.float32)
    one, half = np.float32(1.0), np.float32(0.5)
    q = (np.clip(c, -one, one) - (-one)) * half
    return np.clip(q * np.float32(255.0) + half, np.float32(0.0), np.float32(255.0)).astype(np.uint8)


def read_ply(path):
    """a numpy parser for the binary little-endian PLY files save_ply writes -> names, {name: column}, faces (T,3)"""
    blob = open(path, "rb").read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    lines = blob[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    elements, props = [], {}
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            elements.append((w[1], int(w[2])))
            props[w[1]] = []
        elif w[:1] == ["property"]:
            props[elements[-1][0]].append(w[1:])
    assert [e[0] for e in elements] == ["vertex", "face"]
    assert all(p[0] in ("float", "uchar") for p in props["vertex"]) and props["face"] == [["list", "uchar", "int", "vertex_indices"]]
    nv, nf = elements[0][1], elements[1][1]
    names = [p[1] for p in props["vertex"]]
    vdt = np.dtype([(p[1], "<f4" if p[0] == "float" else "u1") for p in props["vertex"]])
    assert vdt.itemsize == sum(4 if p[0] == "float" else 1 for p in props["vertex"])          # packed, as PLY has it
    vert = np.frombuffer(blob, dtype=vdt, count=nv, offset=end)
    off = end + vert.nbytes
    face = np.frombuffer(blob, dtype=np.dtype([("n", "u1"), ("i", "<i4", (3,))]), count=nf, offset=off)
    assert off + face.nbytes == len(blob)
    assert (face["n"] == 3).all()
    return names, {n: vert[n] for n in names}, face["i"]
