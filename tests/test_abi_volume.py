"""CPU: the C-ABI of the baked-volume kernels (csrc/volume.hip) and the refusals of ops.bake_volume / ops.render_volume /
evaluation.render_volume — what can be checked without a GPU.  Both entry points validate before any HIP call, so a malformed
call returns hipErrorInvalidValue on a machine that has no device."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

INVALID = 1                      # hipErrorInvalidValue
SYMBOLS = ("cips_volume_bake", "cips_volume_render")
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from cips3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbols_are_exported_and_bound_and_the_version_stays(lib):
    from cips3d_amd import _lib, build
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    declared = {
        "cips_volume_bake": [vp] * 4 + [i32] * 4 + [vp],
        "cips_volume_render": [vp] * 8 + [f32, i32, i32] + [vp] * 3 + [i32] * 8 + [vp],
    }
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert _lib.SIGNATURES[s] == (i32, declared[s])
        assert getattr(lib, s).argtypes == declared[s] and getattr(lib, s).restype == i32
    assert lib.cips_version() == 9
    assert "volume.hip" in build.SOURCES
    header = open(build.HERE + "/../include/cips3d_hip.h").read()
    assert "int cips_volume_bake(" in header and "int cips_volume_render(" in header
    assert "IGNORED" in header[header.index("cips_volume_render:"):]          # what the C level does with skip under softplus


_RAW = (C.c_char * (64 * 4 + 16))()


def _dummy():
    """64 floats, 16-byte aligned (never dereferenced by a refused call; lo / hi ARE read on the host: see _render)"""
    base = C.addressof(_RAW)
    return _RAW, C.c_void_p(base + (-base) % 16)


BAKE_POINTERS = ("sigma", "rgb", "packed", "occ")


def _bake(lib, **over):
    keep, p = _dummy()
    a = dict({k: p for k in BAKE_POINTERS}, Bv=2, nx=5, ny=6, nz=7)
    a.update(over)
    return lib.cips_volume_bake(a["sigma"], a["rgb"], a["packed"], a["occ"], a["Bv"], a["nx"], a["ny"], a["nz"], None)


RENDER_POINTERS = ("packed", "occ", "lo", "hi", "xg", "yg", "zg", "cam2world", "rgb", "depth", "opacity")


def _render(lib, **over):
    """a well-formed call on host dummies with overrides; lo / hi are host arrays by contract"""
    keep, p = _dummy()
    lo, hi = (C.c_float * 3)(-0.15, -0.12, -0.1), (C.c_float * 3)(0.15, 0.12, 0.14)
    a = dict({k: p for k in RENDER_POINTERS}, zc=-9.5, clamp_mode=0, flags=4, b=2, Bv=2, nx=5, ny=6, nz=7, H=4, W=6, S=3)
    a.update(lo=C.cast(lo, C.c_void_p), hi=C.cast(hi, C.c_void_p))
    for k in ("lo", "hi"):
        if isinstance(over.get(k), (tuple, list)):
            over = dict(over)
            arr = (C.c_float * 3)(*over[k])
            keep = (keep, arr)
            over[k] = C.cast(arr, C.c_void_p)
    a.update(over)
    return lib.cips_volume_render(a["packed"], a["occ"], a["lo"], a["hi"], a["xg"], a["yg"], a["zg"], a["cam2world"], a["zc"],
                                  a["clamp_mode"], a["flags"], a["rgb"], a["depth"], a["opacity"], a["b"], a["Bv"], a["nx"], a["ny"],
                                  a["nz"], a["H"], a["W"], a["S"], None)


def _misaligned():
    keep, p = _dummy()
    return C.c_void_p(p.value + 4)


IDS = dict(ids=lambda o: ",".join(f"{k}={v if not isinstance(v, C.c_void_p) else 'ptr'}" for k, v in o.items()))
LATTICES = [dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=0), dict(ny=-4), dict(nx=2048, ny=2048, nz=512)]


@pytest.mark.parametrize("over", [{k: None} for k in BAKE_POINTERS] + LATTICES + [dict(Bv=-1), dict(packed=_misaligned())], **IDS)
def test_malformed_bake_calls_are_refused_without_a_device(lib, over):
    assert _bake(lib, **over) == INVALID


@pytest.mark.parametrize("over", [{k: None} for k in RENDER_POINTERS] + LATTICES + [
    dict(H=1), dict(W=1), dict(H=0), dict(W=-3), dict(S=1), dict(S=0), dict(b=-1), dict(Bv=-1),
    dict(Bv=3), dict(Bv=0), dict(b=3, Bv=2),
    dict(lo=(NAN, -0.12, -0.1)), dict(lo=(-0.15, -INF, -0.1)), dict(hi=(0.15, 0.12, INF)), dict(hi=(0.15, NAN, 0.14)),
    dict(hi=(-0.15, 0.12, 0.14)), dict(hi=(0.15, 0.12, -0.1)), dict(lo=(-0.15, 0.5, -0.1)),
    dict(zc=0.0), dict(zc=1.5), dict(zc=NAN), dict(zc=-INF), dict(zc=INF),
    dict(clamp_mode=2), dict(clamp_mode=-1), dict(flags=8), dict(flags=-1),
    dict(packed=_misaligned()),
    dict(b=4, Bv=4, H=1 << 15, W=1 << 15), dict(H=1 << 12, W=1 << 12, S=1 << 8)], **IDS)
def test_malformed_render_calls_are_refused_without_a_device(lib, over):
    assert _render(lib, **over) == INVALID


def test_occ_may_be_missing_only_without_the_skip(lib):
    assert _render(lib, occ=None, flags=4) == INVALID
    assert _render(lib, occ=None, flags=3, b=0, Bv=1) == 0


def test_nothing_to_do_launches_nothing(lib):
    # no device here: a launch would not return 0
    assert _render(lib, b=0, Bv=1) == 0 and _render(lib, b=0, Bv=0) == 0 and _bake(lib, Bv=0) == 0
    assert _render(lib, b=0, Bv=1, S=1) == INVALID                           # validation comes first


def _parts():
    return torch.zeros(2, 5, 6, 7, 4), torch.zeros(2, 1, 1, 1), torch.eye(4).repeat(2, 1, 1)


def test_bake_volume_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import ops
    sigma, rgb = torch.zeros(2, 5, 6, 7), torch.zeros(2, 5, 6, 7, 3)
    with pytest.raises(ValueError, match="GPU"):
        ops.bake_volume(sigma, rgb)
    for bad in [(sigma[0], rgb), (sigma, rgb[..., :2]), (sigma, rgb[:1]), (sigma.double(), rgb), (sigma, rgb.double()),
                (sigma.tolist(), rgb), (sigma[:, :1], rgb[:, :1]), (sigma[..., :1], rgb[:, :, :, :1])]:
        with pytest.raises(ValueError, match="bake_volume"):
            ops.bake_volume(*bad)


def test_render_volume_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import ops
    packed, occ, cams = _parts()
    lo, hi = (-0.15, -0.12, -0.1), (0.15, 0.12, 0.14)
    zg = torch.linspace(0.8, 1.2, 3)
    with pytest.raises(ValueError, match="GPU"):
        ops.render_volume(packed, occ, lo, hi, cams, -9.5, 4, 6, zg=zg)
    with pytest.raises(ValueError, match="GPU"):
        ops.render_volume(packed, occ, lo, hi, cams, -9.5, 4, 6, ray_start=0.8, ray_end=1.2, num_steps=3)
    good = dict(packed=packed, occ=occ, lo=lo, hi=hi, cam2world=cams, zc=-9.5, H=4, W=6, zg=zg)
    for kw, what in [(dict(packed=packed[..., :3]), "packed"), (dict(packed=packed[0]), "packed"), (dict(packed=packed.double()), "packed"),
                     (dict(packed=packed[:, :1]), "lattice"), (dict(occ=occ[:1]), "occ"), (dict(occ=torch.zeros(2, 2, 1, 1)), "occ"),
                     (dict(occ=occ.double()), "occ"), (dict(occ=None), "occ"), (dict(cam2world=cams[:, :3]), "cam2world"),
                     (dict(cam2world=cams[0]), "cam2world"), (dict(cam2world=cams.repeat(2, 1, 1)[:3]), "volumes"),
                     (dict(lo=(0., 0.)), "lo and hi"), (dict(hi=None), "lo and hi"), (dict(lo=(NAN, 0., 0.)), "box"),
                     (dict(hi=(0.15, -0.12, 0.14)), "box"), (dict(hi=(0.15, 0.12, INF)), "box"),
                     (dict(H=1), "H, W"), (dict(W=1), "H, W"), (dict(zc=0.0), "zc"), (dict(zc=2.0), "zc"), (dict(zc=NAN), "zc"),
                     (dict(zc=-INF), "zc"), (dict(zg=zg[:1]), "sample depths"), (dict(zg=zg.double()), "zg"),
                     (dict(zg=zg.view(1, 3)), "zg"), (dict(zg=None), "zg, or"), (dict(zg=None, ray_start=0.8, ray_end=1.2, num_steps=1), "num_steps"),
                     (dict(clamp_mode="elu"), "clamp_mode"), (dict(clamp_mode="softplus"), "skip"),
                     (dict(H=1 << 15, W=1 << 15), "int32")]:
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError, match="render_volume") as e:
            ops.render_volume(**a)
        assert what in str(e.value), (kw, str(e.value))


def test_evaluation_render_volume_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import evaluation
    packed, occ, cams = _parts()
    vol = SimpleNamespace(rgbs=packed, occupancy=occ, lo=(-0.15, -0.12, -0.1), hi=(0.15, 0.12, 0.14))
    with pytest.raises(ValueError, match="GPU"):
        evaluation.render_volume(vol, cams, 12, 8, 0.88, 1.12, 6)
    with pytest.raises(ValueError, match="skip"):
        evaluation.render_volume(vol, cams, 12, 8, 0.88, 1.12, 6, clamp_mode='softplus')
    with pytest.raises(ValueError, match="num_steps"):
        evaluation.render_volume(vol, cams, 12, 8, 0.88, 1.12, 1)
    with pytest.raises(ValueError, match="H, W"):
        evaluation.render_volume(vol, cams, 12, 1, 0.88, 1.12, 6)
    vol.hi = (0.15, 0.12)
    with pytest.raises(ValueError, match="lo and hi"):
        evaluation.render_volume(vol, cams, 12, 8, 0.88, 1.12, 6)


def test_generators_have_bake():
    from cips3d_amd import generator, generator_v1
    assert callable(generator.GeneratorNerfINR.bake) and generator_v1.GeneratorNerfINR.bake is generator.GeneratorNerfINR.bake
