"""GPU: the point-colour path — the kernel that projects the SIREN's 32 colour features to three channels in its registers
(cips_siren_rgb_x3, cips_siren_rgb_x3_grid) against the full forward kernel, whose features it has to reproduce BIT FOR BIT under
a one-hot projection (the same chain, and adding exact zeros is exact: a difference is a layout or staging bug, not noise), its
accuracy class against fp64, and the Python entry points on top of it (ops.siren_rgb, ops.siren_rgb_grid, NeRFNetwork.color,
GeneratorNerfINR.point_colors and color_grid)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from color_refs import one_hot_projection, rgb_ref
from conftest import max_rel, seeded_generator
from oracle import cips3d_oracle as orc
from test_gpu_kernels import _siren_inputs, dev

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
TOL = 1e-3               # tests/test_gpu_generator.py's


def _styles(st):
    return {"nerf_w0": st, "nerf_w1": st, "nerf_rgb": st}


def _lattice_points(gx, gy, gz, B):
    return torch.stack(torch.meshgrid(gx, gy, gz, indexing='ij'), -1).reshape(1, -1, 3).expand(B, -1, 3)


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _guarded(n, device):
    """a NaN-filled buffer of n floats with 64 trailing sentinels"""
    out = torch.full((n + 64,), float("nan"), device=device)
    out[n:] = SENTINEL
    return out


def _raw_rgb(ops, t, pts, W, b, tanh, want_sigma):
    """cips_siren_rgb_x3 through ctypes into guarded buffers -> rgb (B,P,3), its tail, sigma (B,P) or None, its tail or None"""
    from cips3d_amd import _lib
    B, P, _ = pts.shape
    rgb = _guarded(B * P * 3, pts.device)
    sig = _guarded(B * P, pts.device) if want_sigma else None
    sw = ops._siren_struct(t)
    _lib.check(_lib.load().cips_siren_rgb_x3(C.byref(sw), ops._p(pts), ops._p(W), ops._p(b), int(tanh), ops._p(rgb), ops._p(sig),
                                             B, P, ops._stream()), "cips_siren_rgb_x3")
    torch.cuda.synchronize()
    return (rgb[:B * P * 3].view(B, P, 3), rgb[B * P * 3:], sig[:B * P].view(B, P) if want_sigma else None,
            sig[B * P:] if want_sigma else None)


@pytest.mark.parametrize("trig", [0, 1, 3])
@pytest.mark.parametrize("b,P", [(2, 32 * 7 + 5), (3, 4096 + 64), (1, 512 * 3 + 1)])
def test_one_hot_projection_returns_the_forward_features_bit_for_bit(trig, b, P, x3, monkeypatch):
    """a ragged wave, a crossed chunk boundary, more than one image's FiLM vectors, the minimum chunk; both trig_mode bits.
    Eleven launches of three unit rows cover the 32 channels (the last repeats channel 0); every element of rgb is written and
    nothing behind the last; sigma, asked for in the first launch, is the forward's, and is optional in the others."""
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    G, pts, style = _siren_inputs(5, b, P)
    Gd, pts = G.to(dev()), pts.to(dev())
    with torch.no_grad():
        args = Gd.siren._siren_args(_styles(style.to(dev())))
        feat, sigma = ops.SirenFunction.apply(pts, *args)
    t = ops._siren_prep(args)
    assert torch.isfinite(feat).all() and torch.isfinite(sigma).all()
    for k in range(11):
        ch = [(3 * k + j) % 32 for j in range(3)]
        W, bias = (v.to(dev()) for v in one_hot_projection(ch))
        rgb, tail, sig, sig_tail = _raw_rgb(ops, t, pts, W, bias, False, want_sigma=(k == 0))
        assert torch.equal(rgb, feat[..., ch]), ch                     # every element written (the buffer was NaN) ...
        assert bool((tail == SENTINEL).all()), ch                      # ... and nothing behind the last one
        if k == 0:
            assert torch.equal(sig, sigma) and bool((sig_tail == SENTINEL).all())
            own, own_sig = ops.siren_rgb(pts, W, bias, *args, tanh=False, sigma=True)
            assert own.shape == (b, P, 3) and own.grad_fn is None and not own.requires_grad and own_sig.grad_fn is None
            assert torch.equal(own, rgb) and torch.equal(own_sig, sigma)
    # tanh is applied to the same sum: the last launch's channels again, through the wrapper.  The kernel's tanhf and torch's
    # are each good to 2 ulp of a value of at most 1: 4 * 2^-24 apart at the most
    assert float((ops.siren_rgb(pts, W, bias, *args, tanh=True) - torch.tanh(rgb)).abs().max()) <= 2.0 ** -22


@pytest.mark.parametrize("n", [(5, 3, 7), (17, 17, 17)])
def test_grid_form_equals_the_points_form_bit_for_bit(n, x3):
    """105 points (less than a chunk, non-cubic: a swapped axis shows) and 4913 (several chunks, ragged last), two images;
    irregular coordinates, no regularity the kernel could lean on"""
    ops = x3
    B = 2
    G, _, style = _siren_inputs(6, B, 1)
    g = torch.Generator().manual_seed(61)
    gx, gy, gz = (((torch.rand(k, generator=g) - 0.5) * 0.3).to(dev()) for k in n)
    Gd = G.to(dev())
    W, bias = Gd.aux_to_rbg[0].weight.detach(), Gd.aux_to_rbg[0].bias.detach()
    with torch.no_grad():
        args = Gd.siren._siren_args(_styles(style.to(dev())))
    own, own_sig = ops.siren_rgb_grid(gx, gy, gz, W, bias, *args, sigma=True)
    ref, ref_sig = ops.siren_rgb(_lattice_points(gx, gy, gz, B), W, bias, *args, sigma=True)
    assert own.shape == (B, *n, 3) and own_sig.shape == (B, *n) and own.grad_fn is None
    assert torch.isfinite(ref).all() and not torch.equal(ref[0], ref[1])
    assert torch.equal(own.reshape(B, -1, 3), ref) and torch.equal(own_sig.reshape(B, -1), ref_sig)
    assert torch.equal(ops.siren_rgb_grid(gx, gy, gz, W, bias, *args), own)                  # without sigma: the same colours
    assert torch.equal(own_sig, ops.siren_sigma_grid(gx, gy, gz, *args))                     # the sigma-only kernel's bits
    with pytest.raises(ValueError):
        ops.siren_rgb(_lattice_points(gx, gy, gz, B), W[:, :31], bias, *args)


def test_point_colour_is_fp32_class(x3):
    """tests/test_gpu_density.py::test_sigma_only_is_fp32_class's inputs and criterion, not re-tuned: with aux_to_rbg's own weights
    and tanh, the rms error against an fp64 evaluation is at most twice the composed path's own + 2e-7.  The composed path: the
    forward kernel's features, fp32 F.linear, torch.tanh."""
    ops = x3
    b, P = 2, 4096 * 2 + 160
    G, pts, style = _siren_inputs(11, b, P)
    Gd = G.to(dev())
    W, bias = Gd.aux_to_rbg[0].weight.detach(), Gd.aux_to_rbg[0].bias.detach()
    with torch.no_grad():
        args = Gd.siren._siren_args(_styles(style.to(dev())))
        feat, _ = ops.SirenFunction.apply(pts.to(dev()), *args)
        composed = torch.tanh(F.linear(feat, W, bias)).cpu().double()
    own = Gd.siren.color(pts.to(dev()), _styles(style.to(dev())), W, bias, tanh=True)
    assert own.grad_fn is None and own.shape == (b, P, 3)
    ref64 = rgb_ref(pts, ops._siren_prep(args).values(), W, bias, True)

    def rms(a):
        return float((a - ref64).pow(2).mean().sqrt() / ref64.pow(2).mean().sqrt())
    c_s, p_s = rms(composed), rms(own.cpu().double())
    print(f"point colour rms error vs fp64: composed (forward kernel, fp32 linear, tanh) {c_s:.2e} kernel {p_s:.2e}")
    assert p_s <= 2 * c_s + 2e-7


def _zs(seed, b=2):
    g = torch.Generator().manual_seed(seed)
    return {"z_nerf": torch.randn(b, 256, generator=g).to(dev()), "z_inr": torch.randn(b, 512, generator=g).to(dev())}


def _points(seed, b, P):
    return ((torch.rand(b, P, 3, generator=torch.Generator().manual_seed(seed)) - 0.5) * 0.3).to(dev())


def test_point_colors_aux_public_api(x3):
    """equal to ops.siren_rgb with the module's auxiliary layer on the documented styles; psi < 1 truncates towards the average of
    the same 10 000 draws density_grid makes; the INR mapping network never runs; the modes and their arguments are checked"""
    ops = x3
    d = dev()
    G = seeded_generator(8, device=d)
    zs, pts = _zs(81), _points(82, 2, 300)
    W, bias = G.aux_to_rbg[0].weight, G.aux_to_rbg[0].bias
    calls, inr = [], G._map_inr
    G._map_inr = lambda z: (calls.append(1), inr(z))[1]
    try:
        rgb = G.point_colors(zs, pts)
        torch.manual_seed(17)
        rgb_t = G.point_colors(zs, pts, psi=0.5)
    finally:
        del G._map_inr
    assert not calls
    assert rgb.shape == (2, 300, 3) and rgb.dtype == torch.float32 and not rgb.requires_grad and rgb.grad_fn is None
    assert float(rgb.abs().max()) <= 1.0
    with torch.no_grad():
        styles = G._map_nerf(zs["z_nerf"])
        ref = ops.siren_rgb(pts, W, bias, *G.siren._siren_args(styles))
        torch.manual_seed(17)
        vol_t = G.density_grid(zs, resolution=2, psi=0.5)              # its draws: the state it leaves is checked below
        state = torch.cuda.get_rng_state().clone()
        torch.manual_seed(17)
        avg = G.generate_avg_frequencies(device=d)
        trunc = G.get_truncated_freq_phase(styles, {k: avg[k] for k in styles}, 0.5)
        ref_t = ops.siren_rgb(pts, W, bias, *G.siren._siren_args(trunc))
    assert torch.isfinite(ref).all() and torch.equal(rgb, ref)
    assert torch.equal(rgb_t, ref_t) and not torch.equal(rgb_t, rgb)
    torch.manual_seed(17)
    G.point_colors(zs, pts, psi=0.5)
    assert torch.equal(torch.cuda.get_rng_state(), state) and vol_t.shape == (2, 2, 2, 2)
    with pytest.raises(ValueError):
        G.point_colors(zs, pts, mode='head')                           # img_size selects the head's depth
    with pytest.raises(ValueError):
        G.point_colors(zs, pts, mode='rgb')


@pytest.mark.parametrize("img_size,blocks", [(32, 4), (1024, 9)])
def test_point_colors_head_against_the_oracle(img_size, blocks, x3):
    """P = 300 is no multiple of 32: the head's fp32 MFMA path.  The reference: orc.siren's features through orc.inr_head on the
    CPU.  The oracle's head always runs the nine blocks of img_size 1024; the head of depth 32 stops behind block "32", the
    first with a ToRGB, so its image is tanh of that block's ToRGB on the oracle's own block output."""
    d = dev()
    G = seeded_generator(8)
    zs, pts = _zs(83), _points(84, 2, 300)
    sd = {k: v.detach() for k, v in G.named_parameters()}
    with torch.no_grad():
        w_nerf, w_inr = orc.mapping_nerf(sd, zs["z_nerf"].cpu()), orc.mapping_inr(sd, zs["z_inr"].cpu())
        feat = orc.siren(sd, pts.cpu(), w_nerf)[..., :32]
        full, outs = orc.inr_head(sd, feat, w_inr, return_all=True)
        name = orc.INR_NAMES[blocks - 1]
        ref = full if blocks == 9 else torch.tanh(F.linear(outs[blocks - 1], sd[f"inr_net.to_rgbs.{name}.linear.weight"],
                                                           sd[f"inr_net.to_rgbs.{name}.linear.bias"]))
    Gd = G.to(d)
    Gd.device = d
    own = Gd.point_colors(zs, pts, mode='head', img_size=img_size)
    assert own.shape == (2, 300, 3) and own.grad_fn is None and float(own.abs().max()) <= 1.0
    e = max_rel(own, ref)
    print(f"point_colors head, img_size {img_size}: max_rel {e:.2e}")
    assert e < TOL


def test_color_grid_public_api(x3):
    d = dev()
    G = seeded_generator(8, device=d)
    zs = _zs(85)
    N, L, c = 9, 0.3, (0.01, -0.02, 0.0)
    from cips3d_amd.evaluation import density_lattice
    rgb = G.color_grid(zs, resolution=N, cube_length=L, center=c)
    rgb2, sigma = G.color_grid(zs, resolution=N, cube_length=L, center=c, return_sigma=True)
    assert rgb.shape == (2, N, N, N, 3) and rgb.dtype == torch.float32 and rgb.grad_fn is None and sigma.shape == (2, N, N, N)
    assert torch.equal(rgb, rgb2)
    assert torch.equal(sigma, G.density_grid(zs, resolution=N, cube_length=L, center=c))
    pts = _lattice_points(*(a.to(d) for a in density_lattice(N, L, c)), 2)
    ref = G.point_colors(zs, pts)
    assert torch.isfinite(ref).all() and torch.equal(rgb.reshape(2, -1, 3), ref) and not torch.equal(ref[0], ref[1])
    torch.manual_seed(23)
    rgb_t, sigma_t = G.color_grid(zs, resolution=N, cube_length=L, center=c, psi=0.6, return_sigma=True)
    torch.manual_seed(23)
    assert torch.equal(sigma_t, G.density_grid(zs, resolution=N, cube_length=L, center=c, psi=0.6))
    assert not torch.equal(rgb_t, rgb)


def test_color_fallbacks(monkeypatch):
    """other widths run the tensor-operation path; SIREN_FWD_MODE "f32" composes the exact-fp32 forward with an fp32 linear"""
    from cips3d_amd import ops
    from cips3d_amd.generator import NeRFNetwork
    d = dev()
    g = torch.Generator().manual_seed(10)
    b, P = 2, 300
    pts = ((torch.rand(b, P, 3, generator=g) - 0.5) * 0.3).to(d)
    W, bias = (torch.randn(3, 32, generator=g) * 0.1).to(d), (torch.randn(3, generator=g) * 0.1).to(d)
    torch.manual_seed(10)
    net = NeRFNetwork(hidden_dim=64, rgb_dim=32, style_dim=128).to(d)
    assert not net.fused
    sd = _styles(torch.randn(b, 128, generator=g).to(d))
    gx, gy, gz = (((torch.rand(k, generator=g) - 0.5) * 0.3).to(d) for k in (4, 3, 5))
    with torch.no_grad():
        out = net(pts, sd)
        ref = torch.tanh(F.linear(out[..., :32].contiguous(), W, bias))
        out_l = net(_lattice_points(gx, gy, gz, b), sd)
        ref_l = F.linear(out_l[..., :32].contiguous(), W, bias)
    own = net.color(pts, sd, W, bias)
    assert own.shape == (b, P, 3) and not own.requires_grad and torch.isfinite(ref).all() and torch.equal(own, ref)
    own_l, sig_l = net.color_lattice(gx, gy, gz, sd, W, bias, tanh=False, sigma=True)
    assert torch.equal(own_l.reshape(b, -1, 3), ref_l) and torch.equal(sig_l.reshape(b, -1), out_l[..., 32])

    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "f32")
    G, _, style = _siren_inputs(12, b, P)
    Gd = G.to(d)
    sd = _styles(style.to(d))
    with torch.no_grad():
        out = Gd.siren(pts, sd)
        out_l = Gd.siren(_lattice_points(gx, gy, gz, b), sd)
    own = Gd.siren.color(pts, sd, W, bias)
    assert own.grad_fn is None and torch.equal(own, torch.tanh(F.linear(out[..., :32].contiguous(), W, bias)))
    own_l, sig_l = Gd.siren.color_lattice(gx, gy, gz, sd, W, bias, sigma=True)
    assert torch.equal(own_l.reshape(b, -1, 3), torch.tanh(F.linear(out_l[..., :32].contiguous(), W, bias)))
    assert torch.equal(sig_l.reshape(b, -1), out_l[..., 32])
