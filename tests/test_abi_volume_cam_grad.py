"""CPU: the C-ABI of the baked-volume renderer's camera gradient (cips_volume_render_bwd_cam, csrc/volume.hip) and the Python
surface around it — what can be checked without a GPU.  The entry point validates before any HIP call, so a malformed call
returns hipErrorInvalidValue on a machine that has no device."""
import ctypes as C
import inspect
from types import SimpleNamespace

import pytest
import torch

INVALID = 1                      # hipErrorInvalidValue
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    from cips3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbols_are_exported_and_bound(lib):
    from cips3d_amd import _lib, build
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_longlong, C.c_float
    declared = {
        "cips_volume_render_bwd_cam": (i32, [vp] * 8 + [f32, i32, i32] + [vp] * 5 + [i32] * 8 + [vp]),
        "cips_volume_render_bwd_cam_scratch": (i64, [i32] * 4),
    }
    header = open(build.HERE + "/../include/cips3d_hip.h").read()
    for s, (res, args) in declared.items():
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert _lib.SIGNATURES[s] == (res, args)
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype == res
        assert f" {s}(" in header
    assert len(declared["cips_volume_render_bwd_cam"][1]) == 25
    assert "same bits" in header.lower() and "dcam2world" in header
    # the siblings' signatures have not moved
    assert _lib.SIGNATURES["cips_volume_render"] == (i32, [vp] * 8 + [f32, i32, i32] + [vp] * 3 + [i32] * 8 + [vp])
    assert _lib.SIGNATURES["cips_volume_render_bwd"] == (i32, [vp] * 8 + [f32, i32, i32] + [vp] * 5 + [i32] * 8 + [vp])


def test_scratch_is_the_records_and_one_partial_per_tile(lib):
    f, rec = lib.cips_volume_render_bwd_cam_scratch, lib.cips_volume_render_bwd_scratch
    for b, H, W, S, tiles in [(1, 16, 16, 12, 4), (2, 9, 10, 12, 4), (3, 5, 7, 2, 1), (8, 256, 256, 48, 1024), (1, 17, 8, 2, 3),
                              (1, 40, 8, 2, 5), (1, 2, 2, 2, 1)]:
        assert f(b, H, W, S) == rec(b, H, W, S) + b * tiles * 48, (b, H, W, S)
        assert f(b, H, W, S) > 0 and f(b, H, W, S) % 16 == 0
    assert f(0, 16, 16, 12) == 0
    for bad in [(-1, 16, 16, 12), (1, 1, 16, 12), (1, 16, 1, 12), (1, 16, 16, 1), (4, 1 << 15, 1 << 15, 2),
                (1, 1 << 12, 1 << 12, 1 << 8), (1 << 28, 2, 2, 1 << 28)]:          # the last: 2^68 bytes of records
        assert f(*bad) == -1, bad


def test_scratch_is_monotone(lib):
    f = lib.cips_volume_render_bwd_cam_scratch
    base = (2, 9, 10, 12)
    for axis in range(4):
        sizes = []
        for step in range(0, 40, 3):
            a = list(base)
            a[axis] += step
            sizes.append(f(*a))
        assert all(s > 0 for s in sizes) and all(x <= y for x, y in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], axis


_RAW = (C.c_char * (64 * 4 + 16))()


def _dummy():
    """64 floats, 16-byte aligned (never dereferenced by a refused call; lo / hi ARE read on the host)"""
    base = C.addressof(_RAW)
    return _RAW, C.c_void_p(base + (-base) % 16)


def _misaligned():
    keep, p = _dummy()
    return C.c_void_p(p.value + 4)


POINTERS = ("packed", "occ", "lo", "hi", "xg", "yg", "zg", "cam2world", "drgb", "ddepth", "dopacity", "dcam2world", "scratch")
REQUIRED = tuple(k for k in POINTERS if k not in ("ddepth", "dopacity"))


def _cam(lib, **over):
    """a well-formed call on host dummies with overrides; lo / hi are host arrays by contract"""
    keep, p = _dummy()
    lo, hi = (C.c_float * 3)(-0.15, -0.12, -0.1), (C.c_float * 3)(0.15, 0.12, 0.14)
    a = dict({k: p for k in POINTERS}, zc=-9.5, clamp_mode=0, flags=4, b=2, Bv=2, nx=5, ny=6, nz=7, H=4, W=6, S=3)
    a.update(lo=C.cast(lo, C.c_void_p), hi=C.cast(hi, C.c_void_p))
    for k in ("lo", "hi"):
        if isinstance(over.get(k), (tuple, list)):
            over = dict(over)
            arr = (C.c_float * 3)(*over[k])
            keep = (keep, arr)
            over[k] = C.cast(arr, C.c_void_p)
    a.update(over)
    return lib.cips_volume_render_bwd_cam(a["packed"], a["occ"], a["lo"], a["hi"], a["xg"], a["yg"], a["zg"], a["cam2world"],
                                          a["zc"], a["clamp_mode"], a["flags"], a["drgb"], a["ddepth"], a["dopacity"],
                                          a["dcam2world"], a["scratch"], a["b"], a["Bv"], a["nx"], a["ny"], a["nz"], a["H"],
                                          a["W"], a["S"], None)


IDS = dict(ids=lambda o: ",".join(f"{k}={v if not isinstance(v, C.c_void_p) else 'ptr'}" for k, v in o.items()))
LATTICES = [dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=0), dict(ny=-4), dict(nx=2048, ny=2048, nz=512)]


@pytest.mark.parametrize("over", [{k: None} for k in REQUIRED] + LATTICES + [
    dict(H=1), dict(W=1), dict(H=0), dict(W=-3), dict(S=1), dict(S=0), dict(b=-1), dict(Bv=-1),
    dict(Bv=3), dict(Bv=0), dict(b=3, Bv=2),
    dict(lo=(NAN, -0.12, -0.1)), dict(lo=(-0.15, -INF, -0.1)), dict(hi=(0.15, 0.12, INF)), dict(hi=(0.15, NAN, 0.14)),
    dict(hi=(-0.15, 0.12, 0.14)), dict(hi=(0.15, 0.12, -0.1)), dict(lo=(-0.15, 0.5, -0.1)),
    dict(zc=0.0), dict(zc=1.5), dict(zc=NAN), dict(zc=-INF), dict(zc=INF),
    dict(clamp_mode=2), dict(clamp_mode=-1), dict(flags=8), dict(flags=-1),
    dict(packed=_misaligned()), dict(scratch=_misaligned()),
    dict(b=4, Bv=4, H=1 << 15, W=1 << 15), dict(H=1 << 12, W=1 << 12, S=1 << 8),
    dict(b=1 << 28, Bv=1, H=2, W=2, S=1 << 28)], **IDS)
def test_malformed_calls_are_refused_without_a_device(lib, over):
    assert _cam(lib, **over) == INVALID


def test_occ_may_be_missing_only_without_the_skip_and_no_camera_launches_nothing(lib):
    assert _cam(lib, occ=None, flags=4) == INVALID and _cam(lib, occ=None, flags=7) == INVALID
    # no device here: a launch would not return 0
    for kw in (dict(), dict(occ=None, flags=3), dict(ddepth=None), dict(dopacity=None), dict(ddepth=None, dopacity=None)):
        assert _cam(lib, b=0, Bv=0, **kw) == 0, kw
        assert _cam(lib, b=0, Bv=1, **kw) == 0, kw
    assert _cam(lib, b=0, Bv=0, S=1) == INVALID                              # validation comes first


def test_render_volume_documents_and_refuses_as_before():
    from cips3d_amd import ops
    doc = ops.render_volume.__doc__
    assert "cips_volume_render_bwd_cam" in doc and "row 3" in doc and "no double backward" in doc
    cams = torch.eye(4).repeat(2, 1, 1).requires_grad_(True)
    with pytest.raises(ValueError, match="GPU"):                              # a camera that asks for a gradient: no CPU path
        ops.render_volume(torch.zeros(2, 5, 6, 7, 4), torch.zeros(2, 1, 1, 1), (-0.15, -0.12, -0.1), (0.15, 0.12, 0.14), cams,
                          -9.5, 4, 6, zg=torch.linspace(0.8, 1.2, 3))


def _fit_args():
    vol = SimpleNamespace(rgbs=torch.zeros(1, 5, 6, 7, 4), occupancy=torch.zeros(1, 1, 1, 1), lo=(-0.15, -0.12, -0.1),
                          hi=(0.15, 0.12, 0.14), resolution=None)
    return vol, torch.zeros(3, 3, 8, 8)


def test_fit_cameras_signature_and_refusals():
    from cips3d_amd import evaluation
    p = inspect.signature(evaluation.fit_cameras).parameters
    assert list(p)[:6] == ["volume", "targets", "fov", "ray_start", "ray_end", "num_steps"]
    for k in ("yaws", "pitches", "steps", "lr"):
        assert p[k].default is inspect.Parameter.empty and p[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert p["radius"].default == 1.0 and tuple(p["lookat"].default) == (0., 0., 0.) and p["fit_radius"].default is False
    assert p["target_depth"].default is None and p["target_mask"].default is None and p["clamp_mode"].default == 'relu'
    assert p["last_back"].default is False and p["white_back"].default is False
    vol, targets = _fit_args()
    base = (12, 0.88, 1.12, 6)
    ang = dict(yaws=[1.0, 1.5, 2.0], pitches=[1.5, 1.5, 1.5])
    with pytest.raises(TypeError, match="steps"):
        evaluation.fit_cameras(vol, targets, *base, **ang, lr=0.1)
    with pytest.raises(TypeError, match="lr"):
        evaluation.fit_cameras(vol, targets, *base, **ang, steps=3)
    with pytest.raises(ValueError, match="GPU"):
        evaluation.fit_cameras(vol, targets, *base, **ang, steps=3, lr=0.1)
    depth = torch.zeros(3, 1, 8, 8)
    two = SimpleNamespace(**{**vars(vol), "rgbs": torch.zeros(2, 5, 6, 7, 4)})
    for a, kw, what in [((vol, targets), dict(**ang, steps=0, lr=0.1), "steps"), ((vol, targets), dict(**ang, steps=3, lr=0.), "lr"),
                        ((vol, targets[:, :2]), dict(**ang, steps=3, lr=0.1), "targets"),
                        ((two, targets), dict(**ang, steps=3, lr=0.1), "volumes"),
                        ((vol, targets), dict(yaws=[1.0, 1.5], pitches=[1.5, 1.5, 1.5], steps=3, lr=0.1), "yaws"),
                        ((vol, targets), dict(**ang, steps=3, lr=0.1, radius=0.), "radius"),
                        ((vol, targets), dict(**ang, steps=3, lr=0.1, lookat=(0., 0.)), "lookat"),
                        ((vol, targets), dict(**ang, steps=3, lr=0.1, clamp_mode="elu"), "clamp_mode"),
                        ((vol, targets), dict(**ang, steps=3, lr=0.1, depth_weight=1.), "target_depth"),
                        ((vol, targets), dict(**ang, steps=3, lr=0.1, mask_weight=1.), "target_mask"),
                        ((vol, targets), dict(**ang, steps=3, lr=0.1, target_depth=depth[:2], depth_weight=1.), "target_depth")]:
        with pytest.raises(ValueError, match="fit_cameras") as e:
            evaluation.fit_cameras(*a, *base, **kw)
        assert what in str(e.value), (kw, str(e.value))
