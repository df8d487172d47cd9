"""CPU: the C-ABI of the baked-volume backward and of the occupancy refresh (csrc/volume.hip), and the refusals of
ops.volume_occupancy, ops.render_volume with autograd and evaluation.fit_volume — what can be checked without a GPU.  The entry
points validate before any HIP call, so a malformed call returns hipErrorInvalidValue on a machine that has no device."""
import ctypes as C
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


def test_symbols_are_exported_and_bound_and_the_version_stays(lib):
    from cips3d_amd import _lib, build
    vp, i32, i64, f32 = C.c_void_p, C.c_int, C.c_longlong, C.c_float
    declared = {
        "cips_volume_render_bwd": (i32, [vp] * 8 + [f32, i32, i32] + [vp] * 5 + [i32] * 8 + [vp]),
        "cips_volume_occupancy": (i32, [vp, vp] + [i32] * 4 + [vp]),
        "cips_volume_render_bwd_scratch": (i64, [i32] * 4),
    }
    for s, (res, args) in declared.items():
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert _lib.SIGNATURES[s] == (res, args)
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype == res
    assert len(declared["cips_volume_render_bwd"][1]) == 25 and len(declared["cips_volume_occupancy"][1]) == 7
    assert lib.cips_version() == 9
    header = open(build.HERE + "/../include/cips3d_hip.h").read()
    for s in declared:
        assert f" {s}(" in header
    # the forward's signature has not moved
    assert _lib.SIGNATURES["cips_volume_render"] == (i32, [vp] * 8 + [f32, i32, i32] + [vp] * 3 + [i32] * 8 + [vp])


def test_scratch_size_is_one_record_per_sample_and_thread(lib):
    f = lib.cips_volume_render_bwd_scratch
    assert f(1, 16, 16, 12) == 12 * 256 * 16                  # 4 tiles: one block
    assert f(2, 9, 10, 12) == 12 * 2 * 256 * 16               # 2 x 2 tiles per image
    assert f(3, 5, 7, 2) == 2 * 3 * 256 * 16
    assert f(8, 256, 256, 48) == 48 * 8 * 65536 * 16          # every lane on the image: S * b * H * W records
    assert f(1, 17, 8, 2) == 2 * 256 * 16 and f(1, 40, 8, 2) == 2 * 2 * 256 * 16
    assert f(0, 16, 16, 12) == 0
    for bad in [(-1, 16, 16, 12), (1, 1, 16, 12), (1, 16, 1, 12), (1, 16, 16, 1), (4, 1 << 15, 1 << 15, 2), (1, 1 << 12, 1 << 12, 1 << 8)]:
        assert f(*bad) == -1, bad


_RAW = (C.c_char * (64 * 4 + 16))()


def _dummy():
    """64 floats, 16-byte aligned (never dereferenced by a refused call; lo / hi ARE read on the host)"""
    base = C.addressof(_RAW)
    return _RAW, C.c_void_p(base + (-base) % 16)


def _misaligned():
    keep, p = _dummy()
    return C.c_void_p(p.value + 4)


BWD_POINTERS = ("packed", "occ", "lo", "hi", "xg", "yg", "zg", "cam2world", "drgb", "ddepth", "dopacity", "dpacked", "scratch")
REQUIRED = tuple(k for k in BWD_POINTERS if k not in ("ddepth", "dopacity"))


def _bwd(lib, **over):
    """a well-formed call on host dummies with overrides; lo / hi are host arrays by contract"""
    keep, p = _dummy()
    lo, hi = (C.c_float * 3)(-0.15, -0.12, -0.1), (C.c_float * 3)(0.15, 0.12, 0.14)
    a = dict({k: p for k in BWD_POINTERS}, zc=-9.5, clamp_mode=0, flags=4, b=2, Bv=2, nx=5, ny=6, nz=7, H=4, W=6, S=3)
    a.update(lo=C.cast(lo, C.c_void_p), hi=C.cast(hi, C.c_void_p))
    for k in ("lo", "hi"):
        if isinstance(over.get(k), (tuple, list)):
            over = dict(over)
            arr = (C.c_float * 3)(*over[k])
            keep = (keep, arr)
            over[k] = C.cast(arr, C.c_void_p)
    a.update(over)
    return lib.cips_volume_render_bwd(a["packed"], a["occ"], a["lo"], a["hi"], a["xg"], a["yg"], a["zg"], a["cam2world"], a["zc"],
                                      a["clamp_mode"], a["flags"], a["drgb"], a["ddepth"], a["dopacity"], a["dpacked"], a["scratch"],
                                      a["b"], a["Bv"], a["nx"], a["ny"], a["nz"], a["H"], a["W"], a["S"], None)


def _occ(lib, **over):
    keep, p = _dummy()
    a = dict(packed=p, occ=p, Bv=2, nx=5, ny=6, nz=7)
    a.update(over)
    return lib.cips_volume_occupancy(a["packed"], a["occ"], a["Bv"], a["nx"], a["ny"], a["nz"], None)


IDS = dict(ids=lambda o: ",".join(f"{k}={v if not isinstance(v, C.c_void_p) else 'ptr'}" for k, v in o.items()))
LATTICES = [dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=0), dict(ny=-4), dict(nx=2048, ny=2048, nz=512)]


@pytest.mark.parametrize("over", [{k: None} for k in REQUIRED] + LATTICES + [
    dict(H=1), dict(W=1), dict(H=0), dict(W=-3), dict(S=1), dict(S=0), dict(b=-1), dict(Bv=-1),
    dict(Bv=3), dict(Bv=0), dict(b=3, Bv=2),
    dict(lo=(NAN, -0.12, -0.1)), dict(lo=(-0.15, -INF, -0.1)), dict(hi=(0.15, 0.12, INF)), dict(hi=(0.15, NAN, 0.14)),
    dict(hi=(-0.15, 0.12, 0.14)), dict(hi=(0.15, 0.12, -0.1)), dict(lo=(-0.15, 0.5, -0.1)),
    dict(zc=0.0), dict(zc=1.5), dict(zc=NAN), dict(zc=-INF), dict(zc=INF),
    dict(clamp_mode=2), dict(clamp_mode=-1), dict(flags=16), dict(flags=-1),
    dict(packed=_misaligned()), dict(dpacked=_misaligned()), dict(scratch=_misaligned()),
    dict(b=4, Bv=4, H=1 << 15, W=1 << 15), dict(H=1 << 12, W=1 << 12, S=1 << 8)], **IDS)
def test_malformed_backward_calls_are_refused_without_a_device(lib, over):
    assert _bwd(lib, **over) == INVALID


def test_backward_occ_may_be_missing_only_without_the_skip_and_nothing_to_do_launches_nothing(lib):
    assert _bwd(lib, occ=None, flags=4) == INVALID and _bwd(lib, occ=None, flags=12) == INVALID
    # no device here: a memset or a launch would not return 0.  No volume, no camera: nothing to zero, nothing to launch
    for kw in (dict(), dict(occ=None, flags=3), dict(ddepth=None), dict(dopacity=None), dict(ddepth=None, dopacity=None, flags=8)):
        assert _bwd(lib, b=0, Bv=0, **kw) == 0, kw
    assert _bwd(lib, b=0, Bv=0, S=1) == INVALID                              # validation comes first


@pytest.mark.parametrize("over", [dict(packed=None), dict(occ=None), dict(packed=_misaligned()), dict(Bv=-1)] + LATTICES, **IDS)
def test_malformed_occupancy_calls_are_refused_without_a_device(lib, over):
    assert _occ(lib, **over) == INVALID


def test_occupancy_of_no_volume_launches_nothing(lib):
    assert _occ(lib, Bv=0) == 0 and _occ(lib, Bv=0, nx=1) == INVALID


def test_volume_occupancy_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import ops
    packed = torch.zeros(2, 5, 6, 7, 4)
    with pytest.raises(ValueError, match="GPU"):
        ops.volume_occupancy(packed)
    for bad in [packed[..., :3], packed[0], packed.double(), packed.tolist(), packed[:, :1], packed[:, :, :, :1]]:
        with pytest.raises(ValueError, match="volume_occupancy"):
            ops.volume_occupancy(bad)


def test_render_volume_with_autograd_refuses_as_without():
    from cips3d_amd import ops
    packed = torch.zeros(2, 5, 6, 7, 4, requires_grad=True)
    with pytest.raises(ValueError, match="GPU"):
        ops.render_volume(packed, torch.zeros(2, 1, 1, 1), (-0.15, -0.12, -0.1), (0.15, 0.12, 0.14), torch.eye(4).repeat(2, 1, 1),
                          -9.5, 4, 6, zg=torch.linspace(0.8, 1.2, 3))
    assert hasattr(ops, "VolumeRenderFunction") and "atomic" in ops.render_volume.__doc__ and "cam2world" in ops.render_volume.__doc__


def _fit_args():
    vol = SimpleNamespace(rgbs=torch.zeros(1, 5, 6, 7, 4), occupancy=torch.zeros(1, 1, 1, 1), lo=(-0.15, -0.12, -0.1),
                          hi=(0.15, 0.12, 0.14), resolution=None)
    return vol, torch.zeros(3, 3, 8, 8), torch.eye(4).repeat(3, 1, 1)


def test_fit_volume_refuses_malformed_arguments():
    from cips3d_amd import evaluation
    vol, targets, cams = _fit_args()
    base = (12, 0.88, 1.12, 6)
    with pytest.raises(TypeError, match="steps"):
        evaluation.fit_volume(vol, targets, cams, *base, lr=0.1)
    with pytest.raises(TypeError, match="lr"):
        evaluation.fit_volume(vol, targets, cams, *base, steps=3)
    with pytest.raises(TypeError):
        evaluation.fit_volume(vol, targets, cams, *base, 3, 0.1)            # steps and lr by keyword only
    with pytest.raises(ValueError, match="GPU"):
        evaluation.fit_volume(vol, targets, cams, *base, steps=3, lr=0.1)
    two = SimpleNamespace(**{**vars(vol), "rgbs": torch.zeros(2, 5, 6, 7, 4)})
    depth = torch.zeros(3, 1, 8, 8)
    for a, kw, what in [((vol, targets, cams), dict(steps=0, lr=0.1), "steps"), ((vol, targets, cams), dict(steps=3, lr=0.), "lr"),
                        ((vol, targets, cams), dict(steps=3, lr=NAN), "lr"),
                        ((vol, targets[:, :2], cams), dict(steps=3, lr=0.1), "targets"),
                        ((vol, targets[..., :4], cams), dict(steps=3, lr=0.1), "targets"),
                        ((vol, targets.double(), cams), dict(steps=3, lr=0.1), "targets"),
                        ((vol, targets, cams[:2]), dict(steps=3, lr=0.1), "cam2world"),
                        ((two, targets, cams), dict(steps=3, lr=0.1), "volumes"),
                        ((SimpleNamespace(**{**vars(vol), "rgbs": vol.rgbs[..., :3]}), targets, cams), dict(steps=3, lr=0.1), "rgbs"),
                        ((vol, targets, cams), dict(steps=3, lr=0.1, clamp_mode="elu"), "clamp_mode"),
                        ((vol, targets, cams), dict(steps=3, lr=0.1, depth_weight=1.), "target_depth"),
                        ((vol, targets, cams), dict(steps=3, lr=0.1, opacity_weight=1.), "target_opacity"),
                        ((vol, targets, cams), dict(steps=3, lr=0.1, depth_weight=-1., target_depth=depth), "depth_weight"),
                        ((vol, targets, cams), dict(steps=3, lr=0.1, target_depth=depth[:2], depth_weight=1.), "target_depth"),
                        ((vol, targets, cams), dict(steps=3, lr=0.1, target_opacity=depth[:, :, :4], opacity_weight=1.), "target_opacity")]:
        with pytest.raises(ValueError, match="fit_volume") as e:
            evaluation.fit_volume(*a, *base, **kw)
        assert what in str(e.value), (kw, str(e.value))


def test_evaluation_render_volume_takes_grad():
    import inspect
    from cips3d_amd import evaluation
    p = inspect.signature(evaluation.render_volume).parameters
    assert p["grad"].default is False and list(p)[-1] == "grad"
    f = inspect.signature(evaluation.fit_volume).parameters
    assert f["steps"].default is inspect.Parameter.empty and f["lr"].default is inspect.Parameter.empty
    assert f["steps"].kind is inspect.Parameter.KEYWORD_ONLY
