"""CPU: the C-ABI of the pyramid fit loss and the refusals of the style-space entry points — everything about the image
projection feature that can be checked without a GPU.  The entry points validate before any HIP call, so a malformed call
returns hipErrorInvalidValue on a machine that has no device."""
import ctypes as C

import pytest
import torch

from conftest import seeded_generator

INVALID = 1                      # hipErrorInvalidValue
SYMBOLS = ("cips_pyramid_loss_scratch", "cips_pyramid_loss_fwd", "cips_pyramid_loss_bwd")


@pytest.fixture(scope="module")
def lib():
    from cips3d_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_symbols_are_exported_and_bound_and_the_version_stays(lib):
    from cips3d_amd import _lib
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
        assert getattr(lib, s).argtypes == _lib.SIGNATURES[s][1]
    assert lib.cips_version() == 9
    from cips3d_amd import build
    assert "fit_loss.hip" in build.SOURCES


def _fwd_args(**over):
    """a well-formed forward call on host dummies (never dereferenced: every case here is refused first) with overrides"""
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    a = dict(pred=p, target=p, weight=None, lw=(C.c_double * 8)(*([1.0] * 8)), L=3, kind=0, eps=1e-3, loss=p, grad=p, scratch=p,
             nscr=1 << 40, B=2, C=3, H=8, W=12, stream=None)
    a.update(over)
    a["_keep"] = buf
    return a


def _fwd(lib, **over):
    a = _fwd_args(**over)
    return lib.cips_pyramid_loss_fwd(a["pred"], a["target"], a["weight"], a["lw"], a["L"], a["kind"], a["eps"], a["loss"],
                                     a["grad"], a["scratch"], a["nscr"], a["B"], a["C"], a["H"], a["W"], a["stream"])


@pytest.mark.parametrize("over", [
    dict(pred=None), dict(target=None), dict(lw=None), dict(loss=None), dict(grad=None), dict(scratch=None),
    dict(B=0), dict(B=-1), dict(C=0), dict(H=0), dict(W=0), dict(W=-4),
    dict(L=0), dict(L=9), dict(L=-1),
    dict(H=10, L=3), dict(W=10, L=3), dict(H=64, W=64 + 32, L=7), dict(H=192, W=128, L=8),
    dict(kind=1, eps=0.0), dict(kind=1, eps=-1e-3), dict(kind=1, eps=float("nan")), dict(kind=2),
    dict(nscr=0),
], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_malformed_forward_calls_are_refused_without_a_device(lib, over):
    assert _fwd(lib, **over) == INVALID


def test_scratch_size_and_malformed_backward_calls(lib):
    assert lib.cips_pyramid_loss_scratch(2, 3, 8, 12, 3) == 2 * 1                       # one 32x32 tile per image
    assert lib.cips_pyramid_loss_scratch(2, 3, 40, 72, 4) == 2 * 2 * 3
    # L > 6: per image the tiles' partial sums, level-5 means of d (C planes) and w, levels 6 and 7, the per-tile constants
    t = 4 * 4
    assert lib.cips_pyramid_loss_scratch(1, 3, 128, 128, 8) == t + 3 * t + t + (3 * 4 + 4 + 3 * 1 + 1 + 3 * t)
    for bad in [(0, 3, 8, 8, 1), (1, 0, 8, 8, 1), (1, 3, 0, 8, 1), (1, 3, 8, 0, 1), (1, 3, 8, 8, 0), (1, 3, 8, 8, 9), (1, 3, 6, 8, 3)]:
        assert lib.cips_pyramid_loss_scratch(*bad) == -1, bad
    buf = (C.c_float * 4)()
    p = C.cast(buf, C.c_void_p)
    for args in [(None, p, p, 1, 4), (p, None, p, 1, 4), (p, p, None, 1, 4), (p, p, p, 0, 4), (p, p, p, 1, 0), (p, p, p, 1, -3)]:
        assert lib.cips_pyramid_loss_bwd(*args, None) == INVALID, args


def test_pyramid_loss_refuses_cpu_tensors_and_malformed_arguments():
    from cips3d_amd import ops
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.pyramid_loss(x, x)
    with pytest.raises(ValueError):
        ops.pyramid_loss(x, x, level_weights=())
    with pytest.raises(ValueError):
        ops.pyramid_loss(x, x, level_weights=(1.,) * 9)
    with pytest.raises(ValueError):
        ops.pyramid_loss(x, x, level_weights=(1.,) * 5)          # 8 is not a multiple of 16
    with pytest.raises(ValueError):
        ops.pyramid_loss(x, x, kind="l1")
    with pytest.raises(ValueError):
        ops.pyramid_loss(x, x, kind="charbonnier", eps=0.)
    with pytest.raises(ValueError):
        ops.pyramid_loss(x, x[:, :1])
    with pytest.raises(ValueError):
        ops.pyramid_loss(x, x, weight=torch.ones(1, 3, 8, 8))


KW = dict(img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=4, h_stddev=0.3, v_stddev=0.155, hierarchical_sample=False,
          sample_dist="gaussian")


@pytest.mark.parametrize("freeze", [False, True])
def test_style_entry_points_refuse_on_a_cpu_module(freeze):
    G = seeded_generator(11, freeze=freeze)
    names = G.style_names
    assert names[:3] == ("nerf_w0", "nerf_w1", "nerf_rgb") and len(names) == 3 + 18 and names[3] == "inr_w4_0"
    good = {n: torch.zeros(2, 128 if n.startswith("nerf") else 512) for n in names}
    for call in (G.forward_styles, G.render_styles):
        with pytest.raises(ValueError, match="nerf_w1"):
            call({n: t for n, t in good.items() if n != "nerf_w1"}, **KW)
        with pytest.raises(ValueError, match="inr_w2_0"):
            call({**good, "inr_w2_0": torch.zeros(2, 512)}, **KW)
        with pytest.raises(ValueError, match="inr_w8_1"):
            call({**good, "inr_w8_1": torch.zeros(3, 512)}, **KW)            # a wrong batch
        with pytest.raises(ValueError, match="nerf_rgb"):
            call({**good, "nerf_rgb": torch.zeros(2, 512)}, **KW)            # a wrong width
        with pytest.raises(RuntimeError, match="GPU only"):
            call(good, **KW)
    for bad in (dict(grad_points=16), dict(forward_points=16), dict(grad_points=64)):
        with pytest.raises(ValueError, match="whole images"):
            G.render_styles(good, **KW, **bad)
    # ... as render() does, with its errors
    zs = {"z_nerf": torch.zeros(2, 256), "z_inr": torch.zeros(2, 512)}
    with pytest.raises(ValueError, match="whole images"):
        G.render(zs, **KW, grad_points=16)
    with pytest.raises(RuntimeError, match="GPU only"):
        G.render(zs, **KW)


def test_generator_v1_lists_its_own_style_order():
    from cips3d_amd import generator_v1
    from conftest import G_CFG
    torch.manual_seed(3)
    G = generator_v1.GeneratorNerfINR(**G_CFG, device="cpu")
    names = G.style_names
    assert names[:4] == ("nerf_w0", "nerf_w1", "nerf_rgb", "inr_w4_0") and len(names) == 21
    assert hasattr(G, "styles") and hasattr(G, "forward_styles") and hasattr(G, "render_styles")
