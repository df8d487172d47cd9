"""GPU: the density path — the sigma-only SIREN kernel (cips_siren_sigma_x3, cips_siren_sigma_x3_grid) against the full forward
kernel, whose sigma it has to reproduce BIT FOR BIT (the same fmaf / MFMA sequence in a build without fast-math: a difference is
a staging or ordering bug, not noise), and the Python entry points on top of it (ops.siren_sigma, ops.siren_sigma_grid,
NeRFNetwork.density, GeneratorNerfINR.density_grid)."""
import ctypes as C

import pytest
import torch

from conftest import seeded_generator
from oracle import cips3d_oracle as orc
from test_gpu_kernels import _siren_fp64, _siren_inputs, dev

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5


def _styles(st):
    return {"nerf_w0": st, "nerf_w1": st, "nerf_rgb": st}


def _lattice_points(gx, gy, gz, B):
    return torch.stack(torch.meshgrid(gx, gy, gz, indexing='ij'), -1).reshape(1, -1, 3).expand(B, -1, 3)


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _raw_sigma(ops, t, pts, null_colour=False):
    """cips_siren_sigma_x3 through ctypes into a NaN-filled buffer with 64 trailing sentinel floats -> (sigma (B,P), tail)"""
    from cips3d_amd import _lib
    B, P, _ = pts.shape
    out = torch.full((B * P + 64,), float("nan"), device=pts.device)
    out[B * P:] = SENTINEL
    sw = ops._siren_struct(t)
    if null_colour:
        for n in ("wc", "bc", "wf", "bf", "gc", "pc"):
            setattr(sw, n, None)
    _lib.check(_lib.load().cips_siren_sigma_x3(C.byref(sw), ops._p(pts), ops._p(out), B, P, ops._stream()), "cips_siren_sigma_x3")
    torch.cuda.synchronize()
    return out[:B * P].view(B, P), out[B * P:]


@pytest.mark.parametrize("trig", [0, 1, 3])
@pytest.mark.parametrize("b,P", [(2, 32 * 7 + 5), (3, 4096 + 64), (1, 512 * 3 + 1)])
def test_sigma_only_equals_the_full_forward_bit_for_bit(trig, b, P, x3, monkeypatch):
    """a ragged wave, a crossed chunk boundary, more than one image's FiLM vectors, the minimum chunk; both trig_mode bits"""
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    G, pts, style = _siren_inputs(5, b, P)
    Gd, pts = G.to(dev()), pts.to(dev())
    with torch.no_grad():
        args = Gd.siren._siren_args(_styles(style.to(dev())))
        ref = ops.SirenFunction.apply(pts, *args)[1]
        own = ops.siren_sigma(pts, *args)
    raw, tail = _raw_sigma(ops, ops._siren_prep(args), pts)
    assert own.shape == (b, P) and own.grad_fn is None and not own.requires_grad
    assert torch.isfinite(ref).all()
    assert torch.equal(own, ref)
    assert torch.equal(raw, ref)                       # every element written (the buffer was NaN) ...
    assert bool((tail == SENTINEL).all())              # ... and nothing behind the last one


@pytest.mark.parametrize("n", [(5, 3, 7), (17, 17, 17)])
def test_grid_form_equals_the_points_form_bit_for_bit(n, x3):
    """105 points (less than a chunk, non-cubic: a swapped axis shows) and 4913 (several chunks, ragged last), two images"""
    ops = x3
    B = 2
    G, _, style = _siren_inputs(6, B, 1)
    g = torch.Generator().manual_seed(61)
    gx, gy, gz = (((torch.rand(k, generator=g) - 0.5) * 0.3).to(dev()) for k in n)      # no regularity the kernel could lean on
    Gd = G.to(dev())
    with torch.no_grad():
        args = Gd.siren._siren_args(_styles(style.to(dev())))
    own = ops.siren_sigma_grid(gx, gy, gz, *args)
    ref = ops.siren_sigma(_lattice_points(gx, gy, gz, B), *args)
    assert own.shape == (B, *n) and own.grad_fn is None
    assert torch.isfinite(ref).all() and not torch.equal(ref[0], ref[1])
    assert torch.equal(own.reshape(B, -1), ref)


def test_colour_pointers_are_not_read(x3):
    ops = x3
    b, P = 2, 4096 + 64
    G, pts, style = _siren_inputs(7, b, P)
    Gd, pts = G.to(dev()), pts.to(dev())
    with torch.no_grad():
        t = ops._siren_prep(Gd.siren._siren_args(_styles(style.to(dev()))))
    full, _ = _raw_sigma(ops, t, pts)
    bare, tail = _raw_sigma(ops, t, pts, null_colour=True)
    assert torch.isfinite(full).all() and torch.equal(bare, full) and bool((tail == SENTINEL).all())


def test_sigma_only_is_fp32_class(x3):
    """test_gpu_kernels.py::test_siren_forward_x3_sigma_is_fp32_class's inputs at scale_w = 1 and its criterion, not re-tuned:
    the rms error of sigma against an fp64 evaluation is at most twice the fp32 oracle's own + 2e-7"""
    ops = x3
    b, P = 2, 4096 * 2 + 160
    G, pts, style = _siren_inputs(11, b, P)
    ref64 = _siren_fp64(G, pts, style)[..., 32]
    with torch.no_grad():
        ref32 = orc.siren(dict(G.named_parameters()), pts, style)[..., 32]
    Gd = G.to(dev())
    own = Gd.siren.density(pts.to(dev()), _styles(style.to(dev()))).cpu().double()

    def rms(a):
        return float((a - ref64).pow(2).mean().sqrt() / ref64.pow(2).mean().sqrt())
    o_s, p_s = rms(ref32.double()), rms(own)
    print(f"sigma-only rms error vs fp64: oracle(fp32) {o_s:.2e} kernel {p_s:.2e}")
    assert p_s <= 2 * o_s + 2e-7


def test_density_grid_public_api(x3):
    """shape, no gradient, equal to the SIREN's own sigma on the documented lattice and styles; psi < 1 truncates towards the
    average of the same 10 000 draws generate_avg_frequencies makes; the INR mapping network never runs"""
    from cips3d_amd.evaluation import density_lattice
    d = dev()
    G = seeded_generator(8, device=d)
    g = torch.Generator().manual_seed(81)
    zs = {"z_nerf": torch.randn(2, 256, generator=g).to(d), "z_inr": torch.randn(2, 512, generator=g).to(d)}
    N, L, c = 9, 0.3, (0.01, -0.02, 0.0)
    calls, inr = [], G._map_inr
    G._map_inr = lambda z: (calls.append(1), inr(z))[1]
    try:
        vol = G.density_grid(zs, resolution=N, cube_length=L, center=c)
        torch.manual_seed(17)
        vol_t = G.density_grid(zs, resolution=N, cube_length=L, center=c, psi=0.5)
    finally:
        del G._map_inr
    assert not calls
    assert vol.shape == (2, N, N, N) and vol.dtype == torch.float32 and not vol.requires_grad and vol.grad_fn is None
    pts = _lattice_points(*(a.to(d) for a in density_lattice(N, L, c)), 2)
    with torch.no_grad():
        styles = G._map_nerf(zs["z_nerf"])
        ref = G.siren(pts, styles)[..., 32]
        torch.manual_seed(17)
        avg = G.generate_avg_frequencies(device=d)
        trunc = G.get_truncated_freq_phase(styles, {k: avg[k] for k in styles}, 0.5)
        ref_t = G.siren(pts, trunc)[..., 32]
    assert torch.isfinite(ref).all() and torch.equal(vol.reshape(2, -1), ref)
    assert torch.equal(vol_t.reshape(2, -1), ref_t) and not torch.equal(vol_t, vol)


def test_density_grid_of_the_v1_generator(x3):
    """generator_v1 inherits the method; its NeRF mapping network has no nerf_rgb head, which sigma does not depend on"""
    from cips3d_amd.evaluation import density_lattice
    from test_generator_v1_cpu import seeded_generator_v1
    d = dev()
    G = seeded_generator_v1(9, device=d)
    g = torch.Generator().manual_seed(91)
    zs = {"z_nerf": torch.randn(2, 256, generator=g).to(d), "z_inr": torch.randn(2, 512, generator=g).to(d)}
    vol = G.density_grid(zs, resolution=5)
    pts = _lattice_points(*(a.to(d) for a in density_lattice(5, 0.3, (0., 0., 0.))), 2)
    with torch.no_grad():
        ref = G.siren(pts, G.mapping_network(**zs))[..., 32]
    assert vol.shape == (2, 5, 5, 5) and torch.isfinite(ref).all() and torch.equal(vol.reshape(2, -1), ref)


def test_density_fallbacks(monkeypatch):
    """other widths run the tensor-operation path; SIREN_FWD_MODE "f32" returns the exact-fp32 forward's sigma, lattice form too"""
    from cips3d_amd import ops
    from cips3d_amd.generator import NeRFNetwork
    d = dev()
    g = torch.Generator().manual_seed(10)
    b, P = 2, 300
    pts = ((torch.rand(b, P, 3, generator=g) - 0.5) * 0.3).to(d)
    torch.manual_seed(10)
    net = NeRFNetwork(hidden_dim=64, rgb_dim=32, style_dim=128).to(d)
    assert not net.fused
    sd = _styles(torch.randn(b, 128, generator=g).to(d))
    with torch.no_grad():
        ref = net(pts, sd)[..., -1]
    own = net.density(pts, sd)
    assert own.shape == (b, P) and not own.requires_grad and torch.isfinite(ref).all() and torch.equal(own, ref)
    gx, gy, gz = (((torch.rand(k, generator=g) - 0.5) * 0.3).to(d) for k in (4, 3, 5))
    with torch.no_grad():
        ref = net(_lattice_points(gx, gy, gz, b), sd)[..., -1]
    assert torch.equal(net.density_lattice(gx, gy, gz, sd).reshape(b, -1), ref)

    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "f32")
    G, _, style = _siren_inputs(12, b, P)
    Gd = G.to(d)
    sd = _styles(style.to(d))
    with torch.no_grad():
        ref = Gd.siren(pts, sd)[..., 32]
        ref_l = Gd.siren(_lattice_points(gx, gy, gz, b), sd)[..., 32]
    own = Gd.siren.density(pts, sd)
    assert own.grad_fn is None and torch.isfinite(ref).all() and torch.equal(own, ref)
    assert torch.equal(Gd.siren.density_lattice(gx, gy, gz, sd).reshape(b, -1), ref_l)
