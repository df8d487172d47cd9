"""CPU: the C-ABI of the feature-volume kernels (csrc/volume.hip) and the refusals of ops.bake_feature_volume /
ops.render_feature_volume — what can be checked without a GPU.  The entry points validate before any HIP call, so a malformed
call returns hipErrorInvalidValue on a machine that has no device.  Every refusal the header lists is here."""
import ctypes as C

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
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    declared = {
        "cips_feature_volume_bake": [vp] * 4 + [i32] * 4 + [vp],
        "cips_feature_volume_bake_slab": [vp] * 4 + [i32] * 6 + [vp],
        "cips_feature_volume_render": [vp] * 9 + [f32, i32, i32] + [vp] * 3 + [i32] * 8 + [vp],
    }
    header = open(build.HERE + "/../include/cips3d_hip.h").read()
    for s, args in declared.items():
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert _lib.SIGNATURES[s] == (i32, args)
        assert getattr(lib, s).argtypes == args and getattr(lib, s).restype == i32
        assert f"int {s}(" in header
    rule = header[header.index("cips_feature_volume_render:"):]
    assert "taken to be finite" in header[header.index("Baked FEATURE volumes"):] and "IGNORED" in rule and "b == 0" in rule


_RAW = (C.c_char * (64 * 4 + 16))()


def _dummy():
    """64 floats, 16-byte aligned (never dereferenced by a refused call; lo / hi ARE read on the host)"""
    base = C.addressof(_RAW)
    return C.c_void_p(base + (-base) % 16)


def _misaligned():
    return C.c_void_p(_dummy().value + 4)


BAKE_POINTERS = ("sigma", "feat_rows", "planes", "occ")


def _bake(lib, **over):
    p = _dummy()
    a = dict({k: p for k in BAKE_POINTERS}, Bv=2, nx=5, ny=6, nz=7)
    a.update(over)
    head = (a["sigma"], a["feat_rows"], a["planes"], a["occ"], a["Bv"], a["nx"], a["ny"], a["nz"])
    if "x0" in a or "sx" in a:
        return lib.cips_feature_volume_bake_slab(*head, a.get("x0", 0), a.get("sx", a["nx"]), None)
    return lib.cips_feature_volume_bake(*head, None)


RENDER_POINTERS = ("sigma", "planes", "occ", "lo", "hi", "xg", "yg", "zg", "cam2world", "fea", "depth", "opacity")
_KEEP = []


def _render(lib, **over):
    """a well-formed call on host dummies with overrides; lo / hi are host arrays by contract"""
    p = _dummy()
    box = dict(lo=(-0.15, -0.12, -0.1), hi=(0.15, 0.12, 0.14))
    a = dict({k: p for k in RENDER_POINTERS}, zc=-9.5, clamp_mode=0, flags=4, b=2, Bv=2, nx=5, ny=6, nz=7, H=4, W=6, S=3)
    a.update(box)
    a.update(over)
    for k in ("lo", "hi"):
        if isinstance(a[k], (tuple, list)):
            arr = (C.c_float * 3)(*a[k])
            _KEEP.append(arr)
            a[k] = C.cast(arr, C.c_void_p)
    return lib.cips_feature_volume_render(a["sigma"], a["planes"], a["occ"], a["lo"], a["hi"], a["xg"], a["yg"], a["zg"],
                                          a["cam2world"], a["zc"], a["clamp_mode"], a["flags"], a["fea"], a["depth"], a["opacity"],
                                          a["b"], a["Bv"], a["nx"], a["ny"], a["nz"], a["H"], a["W"], a["S"], None)


IDS = dict(ids=lambda o: ",".join(f"{k}={v if not isinstance(v, C.c_void_p) else 'ptr'}" for k, v in o.items()))
LATTICES = [dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=0), dict(ny=-4), dict(nx=2048, ny=2048, nz=512)]


@pytest.mark.parametrize("over", [{k: None} for k in BAKE_POINTERS] + LATTICES + [
    dict(Bv=-1), dict(planes=_misaligned()), dict(feat_rows=_misaligned()),
    dict(Bv=1 << 12, nx=1024, ny=1024, nz=1024),                                     # the pack grid, beyond int32
    dict(x0=-1, sx=2), dict(x0=0, sx=0), dict(x0=4, sx=2), dict(x0=5, sx=1), dict(x0=0, sx=6), dict(x0=0x7fffffff, sx=2)], **IDS)
def test_malformed_bake_calls_are_refused_without_a_device(lib, over):
    assert _bake(lib, **over) == INVALID


@pytest.mark.parametrize("over", [{k: None} for k in RENDER_POINTERS] + LATTICES + [
    dict(H=1), dict(W=1), dict(H=0), dict(W=-3), dict(S=1), dict(S=0), dict(b=-1), dict(Bv=-1),
    dict(Bv=3), dict(Bv=0), dict(b=3, Bv=2),
    dict(lo=(NAN, -0.12, -0.1)), dict(lo=(-0.15, -INF, -0.1)), dict(hi=(0.15, 0.12, INF)), dict(hi=(0.15, NAN, 0.14)),
    dict(hi=(-0.15, 0.12, 0.14)), dict(hi=(0.15, 0.12, -0.1)), dict(lo=(-0.15, 0.5, -0.1)),
    dict(zc=0.0), dict(zc=1.5), dict(zc=NAN), dict(zc=-INF), dict(zc=INF),
    dict(clamp_mode=2), dict(clamp_mode=-1), dict(flags=8), dict(flags=-1),
    dict(planes=_misaligned()), dict(fea=_misaligned()),
    dict(b=4, Bv=4, H=1 << 15, W=1 << 15), dict(H=1 << 12, W=1 << 12, S=1 << 8)], **IDS)
def test_malformed_render_calls_are_refused_without_a_device(lib, over):
    assert _render(lib, **over) == INVALID


def test_occ_may_be_missing_only_without_the_skip(lib):
    assert _render(lib, occ=None, flags=4) == INVALID
    assert _render(lib, occ=None, flags=3, b=0, Bv=1) == 0


def test_nothing_to_do_launches_nothing(lib):
    # no device here: a launch would not return 0
    assert _render(lib, b=0, Bv=1) == 0 and _render(lib, b=0, Bv=0) == 0
    assert _bake(lib, Bv=0) == 0 and _bake(lib, Bv=0, x0=1, sx=2) == 0
    assert _render(lib, b=0, Bv=1, S=1) == INVALID and _bake(lib, Bv=0, nx=1) == INVALID        # validation comes first


def test_bake_feature_volume_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import ops
    sigma, feat = torch.zeros(2, 5, 6, 7), torch.zeros(2, 5, 6, 7, 32)
    for f in (feat, feat.view(2, 210, 32)):
        with pytest.raises(ValueError, match="GPU"):
            ops.bake_feature_volume(sigma, f)
    for bad in [(sigma[0], feat), (sigma, feat[..., :31]), (sigma, feat[:1]), (sigma.double(), feat), (sigma, feat.double()),
                (sigma.tolist(), feat), (sigma[:, :1], feat[:, :1]), (sigma, feat.view(2, 210, 32)[:, :209]), (sigma, None)]:
        with pytest.raises(ValueError, match="bake_feature_volume"):
            ops.bake_feature_volume(*bad)


def test_render_feature_volume_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import ops
    sigma, planes, occ, cams = torch.zeros(2, 5, 6, 7), torch.zeros(2, 8, 5, 6, 7, 4), torch.zeros(2, 1, 1, 1), torch.eye(4).repeat(2, 1, 1)
    lo, hi = (-0.15, -0.12, -0.1), (0.15, 0.12, 0.14)
    zg = torch.linspace(0.8, 1.2, 3)
    with pytest.raises(ValueError, match="GPU"):
        ops.render_feature_volume(sigma, planes, occ, lo, hi, cams, -9.5, 4, 6, zg=zg)
    with pytest.raises(ValueError, match="GPU"):
        ops.render_feature_volume(sigma, planes, occ, lo, hi, cams, -9.5, 4, 6, ray_start=0.8, ray_end=1.2, num_steps=3)
    good = dict(sigma=sigma, planes=planes, occ=occ, lo=lo, hi=hi, cam2world=cams, zc=-9.5, H=4, W=6, zg=zg)
    for kw, what in [(dict(planes=planes[..., :3]), "planes"), (dict(planes=planes[0]), "planes"), (dict(planes=planes.double()), "planes"),
                     (dict(planes=planes[:, :7]), "planes"), (dict(sigma=sigma[0]), "sigma"), (dict(sigma=sigma.double()), "sigma"),
                     (dict(sigma=sigma[:, :1], planes=planes[:, :, :1]), "lattice"), (dict(occ=occ[:1]), "occ"),
                     (dict(occ=torch.zeros(2, 2, 1, 1)), "occ"), (dict(occ=occ.double()), "occ"), (dict(occ=None), "occ"),
                     (dict(cam2world=cams[:, :3]), "cam2world"), (dict(cam2world=cams[0]), "cam2world"),
                     (dict(cam2world=cams.repeat(2, 1, 1)[:3]), "volumes"),
                     (dict(lo=(0., 0.)), "lo and hi"), (dict(hi=None), "lo and hi"), (dict(lo=(NAN, 0., 0.)), "box"),
                     (dict(hi=(0.15, -0.12, 0.14)), "box"), (dict(hi=(0.15, 0.12, INF)), "box"),
                     (dict(H=1), "H, W"), (dict(W=1), "H, W"), (dict(zc=0.0), "zc"), (dict(zc=2.0), "zc"), (dict(zc=NAN), "zc"),
                     (dict(zc=-INF), "zc"), (dict(zg=zg[:1]), "sample depths"), (dict(zg=zg.double()), "zg"),
                     (dict(zg=zg.view(1, 3)), "zg"), (dict(zg=None), "zg, or"),
                     (dict(zg=None, ray_start=0.8, ray_end=1.2, num_steps=1), "num_steps"),
                     (dict(clamp_mode="elu"), "clamp_mode"), (dict(clamp_mode="softplus"), "skip"),
                     (dict(H=1 << 15, W=1 << 15), "int32")]:
        a = dict(good)
        a.update(kw)
        with pytest.raises(ValueError, match="render_feature_volume") as e:
            ops.render_feature_volume(**a)
        assert what in str(e.value), (kw, str(e.value))


@pytest.mark.parametrize("which", ["sigma", "planes", "cam2world"])
def test_an_input_that_requires_grad_is_refused(which):
    """forward only: a gradient request gets an answer, not a silent constant"""
    from cips3d_amd import ops
    t = dict(sigma=torch.zeros(2, 5, 6, 7), planes=torch.zeros(2, 8, 5, 6, 7, 4), cam2world=torch.eye(4).repeat(2, 1, 1))
    t[which].requires_grad_(True)
    with pytest.raises(ValueError, match="gradients are not built"):
        ops.render_feature_volume(t["sigma"], t["planes"], torch.zeros(2, 1, 1, 1), (-0.15, -0.12, -0.1), (0.15, 0.12, 0.14),
                                  t["cam2world"], -9.5, 4, 6, zg=torch.linspace(0.8, 1.2, 3))


def test_generators_and_evaluation_have_the_entry_points():
    from cips3d_amd import evaluation, generator, generator_v1
    assert callable(generator.GeneratorNerfINR.bake_features) and callable(evaluation.render_feature_volume)
    assert generator_v1.GeneratorNerfINR.bake_features is generator.GeneratorNerfINR.bake_features
