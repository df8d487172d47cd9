"""GPU: the density gradient — siren_sigma_grad_x3_kernel (cips_siren_sigma_grad_x3, cips_siren_sigma_grad_x3_grid): its sigma
against the sigma-only kernel BIT FOR BIT, its gradient against fp64 autograd of the oracle (the yardstick that
tests/test_density_gradient_oracle_cpu.py validates), the two scale factors the kernel removes at its output, and the Python
entry points on top of it (ops.siren_sigma_grad(_grid), NeRFNetwork.density_gradient(_lattice), GeneratorNerfINR.density_grid
(return_gradient=True), .density_gradient, .geometry)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import max_rel, seeded_generator
from oracle import cips3d_oracle as orc
from test_gpu_kernels import _siren_inputs, dev

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
SHAPES = [(2, 32 * 7 + 5), (3, 4096 + 64), (1, 512 * 3 + 1)]     # ragged wave; crossed chunk, three images; minimum chunk
BAR = 1e-4            # the project's standing bar for free-running SIREN gradients (DESIGN sections 0 / 4)


def _styles(st):
    return {"nerf_w0": st, "nerf_w1": st, "nerf_rgb": st}


def _lattice_points(gx, gy, gz, B):
    return torch.stack(torch.meshgrid(gx, gy, gz, indexing='ij'), -1).reshape(1, -1, 3).expand(B, -1, 3)


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _oracle_grad(G, pts, style, dtype):
    """d sigma / d points of the oracle by autograd, in `dtype`, on the CPU -> (b,P,3) fp64"""
    sd = {k: v.detach().to(dtype) for k, v in G.named_parameters()}
    p = pts.to(dtype).clone().requires_grad_(True)
    grad, = torch.autograd.grad(orc.siren(sd, p, style.to(dtype))[..., 32].sum(), p)
    return grad.double()


_REF = {}


def _case(seed, b, P):
    """inputs and references of one shape, computed once and shared: G (CPU), pts, style, ref64, ref32"""
    key = (seed, b, P)
    if key not in _REF:
        G, pts, style = _siren_inputs(seed, b, P)
        _REF[key] = (G, pts, style, _oracle_grad(G, pts, style, torch.float64), _oracle_grad(G, pts, style, torch.float32))
    return _REF[key]


def _errors(own, ref64):
    """per image max |own - ref64| / max |ref64| -> the worst image's; and the smallest cosine between own and ref64 of any point"""
    own = own.detach().double().cpu()
    e = max(float((own[i] - ref64[i]).abs().max() / ref64[i].abs().max()) for i in range(ref64.shape[0]))
    cos = (own * ref64).sum(-1) / (own.norm(dim=-1) * ref64.norm(dim=-1))
    return e, float(cos.min())


def _raw(ops, t, pts, want_sigma=True, null_colour=False):
    """cips_siren_sigma_grad_x3 through ctypes into NaN-filled buffers with 64 trailing sentinel floats each
    -> sigma (B,P) or None, grad (B,P,3), the two tails"""
    from cips3d_amd import _lib
    B, P, _ = pts.shape
    sig = torch.full((B * P + 64,), float("nan"), device=pts.device)
    grad = torch.full((B * P * 3 + 64,), float("nan"), device=pts.device)
    sig[B * P:] = SENTINEL
    grad[B * P * 3:] = SENTINEL
    sw = ops._siren_struct(t)
    if null_colour:
        for n in ("wc", "bc", "wf", "bf", "gc", "pc"):
            setattr(sw, n, None)
    _lib.check(_lib.load().cips_siren_sigma_grad_x3(C.byref(sw), ops._p(pts), ops._p(sig) if want_sigma else None, ops._p(grad),
                                                    B, P, ops._stream()), "cips_siren_sigma_grad_x3")
    torch.cuda.synchronize()
    return sig[:B * P].view(B, P), grad[:B * P * 3].view(B, P, 3), sig[B * P:], grad[B * P * 3:]


@pytest.mark.parametrize("trig", [0, 1, 3])
@pytest.mark.parametrize("b,P", SHAPES)
def test_sigma_is_the_sigma_kernels_bit_for_bit_and_the_buffers_are_written_exactly(trig, b, P, x3, monkeypatch):
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    G, pts, style = _siren_inputs(5, b, P)
    Gd, pts = G.to(dev()), pts.to(dev())
    with torch.no_grad():
        args = Gd.siren._siren_args(_styles(style.to(dev())))
    ref = ops.siren_sigma(pts, *args)
    sig, grad = ops.siren_sigma_grad(pts, *args)
    assert sig.shape == (b, P) and grad.shape == (b, P, 3) and sig.dtype == grad.dtype == torch.float32
    assert sig.grad_fn is None and grad.grad_fn is None and not sig.requires_grad and not grad.requires_grad
    assert torch.isfinite(ref).all() and torch.equal(sig, ref)
    t = ops._siren_prep(args)
    r_sig, r_grad, t_sig, t_grad = _raw(ops, t, pts)
    assert torch.equal(r_sig, ref) and torch.equal(r_grad, grad) and torch.isfinite(r_grad).all()      # every element written ...
    assert bool((t_sig == SENTINEL).all()) and bool((t_grad == SENTINEL).all())                        # ... nothing behind
    n_sig, n_grad, t_sig, t_grad = _raw(ops, t, pts, want_sigma=False)
    assert bool(torch.isnan(n_sig).all()) and torch.equal(n_grad, grad)                                # sigma == NULL: not written
    assert bool((t_sig == SENTINEL).all()) and bool((t_grad == SENTINEL).all())
    c_sig, c_grad, _, _ = _raw(ops, t, pts, null_colour=True)
    assert torch.equal(c_sig, ref) and torch.equal(c_grad, grad)                                       # colour pointers not read


@pytest.mark.parametrize("trig", [0, 1, 3])
@pytest.mark.parametrize("b,P", SHAPES)
def test_gradient_against_fp64_autograd_of_the_oracle(trig, b, P, x3, monkeypatch):
    """per image max |own - ref64| / max |ref64| < 1e-4 and, at every point, cos(own, ref64) >= 1 - 1e-6 (no point of these
    inputs is degenerate: min |grad sigma| is 0.12 .. 0.87 against a maximum of about 16).  The fp32 oracle's own distance
    from fp64 is printed next to the kernel's."""
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    G, pts, style, ref64, ref32 = _case(5, b, P)
    Gd = seeded_generator(5, device=dev())
    with torch.no_grad():
        args = Gd.siren._siren_args(_styles(style.to(dev())))
    own = ops.siren_sigma_grad(pts.to(dev()), *args)[1]
    e_own, c_own = _errors(own, ref64)
    e_orc, c_orc = _errors(ref32, ref64)
    nrm = ref64.norm(dim=-1)
    print(f"grad sigma trig={trig} ({b}, {P}): max err / max |ref64|  kernel {e_own:.2e}  oracle(fp32) {e_orc:.2e} | "
          f"1 - min cos  kernel {1 - c_own:.2e}  oracle(fp32) {1 - c_orc:.2e} | |ref64| min {float(nrm.min()):.2f} max {float(nrm.max()):.2f}")
    assert torch.isfinite(own).all()
    assert e_own < BAR
    assert c_own >= 1 - 1e-6


def _scaled_inputs(scale_w, scale_ws, b, P):
    """test_gpu_kernels.py::test_siren_forward_x3_sigma_is_fp32_class's construction: W1 / Wc / Wf times scale_w with the FiLM gain
    layers compensated (the same function), and final_layer.weight times scale_ws (sigma - bias and its gradient scale with it)"""
    G, pts, style = _siren_inputs(11, b, P)
    with torch.no_grad():
        for lay in (G.siren.network[1], G.siren.color_layer_sine):
            lay.linear.weight.mul_(scale_w); lay.linear.bias.mul_(scale_w)
            lay.gain_fc.weight.div_(scale_w); lay.gain_fc.bias.copy_((lay.gain_fc.bias + 2.0) / scale_w - 2.0)
        G.siren.color_layer_linear[0].weight.mul_(scale_w)
        G.siren.final_layer.weight.mul_(scale_ws)
    return G, pts, style


_BASE = {}


@pytest.mark.parametrize("scale_w,scale_ws", [(37.0, 1.0), (3e-4, 1.0), (1.0, 1e-3), (1.0, 1e3)])
def test_gradient_does_not_depend_on_the_magnitude_of_the_weights(scale_w, scale_ws, x3, monkeypatch):
    """the fp16 planes' range (W1 * 2^k next to g1 * 2^-k: dp1 is rescaled by a power of two per image) and the revolutions
    of the hardware-sine staging (both transposed factors carry 1 / 2 pi): the error against fp64 stays under the same 1e-4 and
    within 4x of the unscaled weights' — a subnormal or overflowed plane costs orders of magnitude, not a factor"""
    ops = x3
    b, P = 2, 4096 + 64
    G0, pts, style, ref64, _ = _case(11, b, P)
    G, _, _ = _scaled_inputs(scale_w, scale_ws, b, P)
    ref = ref64 * scale_ws           # W1's scaling leaves the function as it is up to rounding; ws scales the gradient
    for trig in (0, 1, 3):
        monkeypatch.setattr(ops, "TRIG_MODE", trig)
        if trig not in _BASE:
            Gd = seeded_generator(11, device=dev())
            with torch.no_grad():
                _BASE[trig] = _errors(ops.siren_sigma_grad(pts.to(dev()), *Gd.siren._siren_args(_styles(style.to(dev()))))[1], ref64)[0]
        Gd = G.to(dev())
        with torch.no_grad():
            args = Gd.siren._siren_args(_styles(style.to(dev())))
        own = ops.siren_sigma_grad(pts.to(dev()), *args)[1]
        e, c = _errors(own, ref)
        print(f"grad sigma scale_w={scale_w} scale_ws={scale_ws} trig={trig}: max err / max |ref64| {e:.2e} (unscaled {_BASE[trig]:.2e}), "
              f"1 - min cos {1 - c:.2e}")
        assert torch.isfinite(own).all()
        assert _BASE[trig] < BAR and e < BAR
        assert e <= 4 * _BASE[trig]


@pytest.mark.parametrize("n", [(5, 3, 7), (17, 17, 17)])
def test_grid_form_equals_the_points_form_bit_for_bit(n, x3):
    """105 points (less than a chunk, non-cubic: a swapped axis shows) and 4913 (several chunks, ragged last), two images"""
    ops = x3
    B = 2
    G, _, style = _siren_inputs(6, B, 1)
    g = torch.Generator().manual_seed(61)
    gx, gy, gz = (((torch.rand(k, generator=g) - 0.5) * 0.3).to(dev()) for k in n)
    Gd = G.to(dev())
    with torch.no_grad():
        args = Gd.siren._siren_args(_styles(style.to(dev())))
    sig, grad = ops.siren_sigma_grad_grid(gx, gy, gz, *args)
    r_sig, r_grad = ops.siren_sigma_grad(_lattice_points(gx, gy, gz, B), *args)
    assert sig.shape == (B, *n) and grad.shape == (B, *n, 3) and sig.grad_fn is None and grad.grad_fn is None
    assert torch.isfinite(r_sig).all() and torch.isfinite(r_grad).all()
    assert not torch.equal(r_sig[0], r_sig[1]) and not torch.equal(r_grad[0], r_grad[1])
    assert torch.equal(sig.reshape(B, -1), r_sig) and torch.equal(grad.reshape(B, -1, 3), r_grad)
    assert torch.equal(sig, ops.siren_sigma_grid(gx, gy, gz, *args))


def _zs(seed, d, b=2):
    g = torch.Generator().manual_seed(seed)
    return {"z_nerf": torch.randn(b, 256, generator=g).to(d), "z_inr": torch.randn(b, 512, generator=g).to(d)}


def test_generator_density_gradient_public_api(x3):
    """density_grid(return_gradient=True): the default call's sigma bit for bit, the documented shapes, the lattice kernel's
    gradient; density_gradient at arbitrary points with psi < 1: the ops call on the truncated styles (the same 10 000 draws as
    generate_avg_frequencies); the INR mapping network never runs"""
    from cips3d_amd.evaluation import density_lattice
    ops = x3
    d = dev()
    G = seeded_generator(8, device=d)
    zs = _zs(81, d)
    N = 9
    g = torch.Generator().manual_seed(82)
    pts = ((torch.rand(2, 77, 3, generator=g) - 0.5) * 0.3).to(d)
    calls, inr = [], G._map_inr
    G._map_inr = lambda z: (calls.append(1), inr(z))[1]
    try:
        vol = G.density_grid(zs, N)
        vol_g, grad = G.density_grid(zs, N, return_gradient=True)
        torch.manual_seed(17)
        sig_t, grad_t = G.density_gradient(zs, pts, psi=0.5)
    finally:
        del G._map_inr
    assert not calls
    assert vol.shape == (2, N, N, N) and vol_g.shape == (2, N, N, N) and grad.shape == (2, N, N, N, 3)
    assert vol_g.dtype == grad.dtype == torch.float32 and vol_g.grad_fn is None and grad.grad_fn is None and not grad.requires_grad
    assert torch.isfinite(vol).all() and torch.equal(vol, vol_g)
    with torch.no_grad():
        styles = G._map_nerf(zs["z_nerf"])
        lat = _lattice_points(*(a.to(d) for a in density_lattice(N, 0.3, (0., 0., 0.))), 2)
        ref_s, ref_g = ops.siren_sigma_grad(lat, *G.siren._siren_args(styles))
        torch.manual_seed(17)
        avg = G.generate_avg_frequencies(device=d)
        trunc = G.get_truncated_freq_phase(styles, {k: avg[k] for k in styles}, 0.5)
        ref_st, ref_gt = ops.siren_sigma_grad(pts, *G.siren._siren_args(trunc))
        ref_s1 = ops.siren_sigma_grad(pts, *G.siren._siren_args(styles))[0]
    assert torch.equal(vol_g.reshape(2, -1), ref_s) and torch.equal(grad.reshape(2, -1, 3), ref_g)
    assert sig_t.shape == (2, 77) and grad_t.shape == (2, 77, 3) and grad_t.grad_fn is None
    assert torch.isfinite(ref_gt).all() and torch.equal(sig_t, ref_st) and torch.equal(grad_t, ref_gt)
    assert not torch.equal(ref_s1, ref_st)


def _geometry_kwargs(hier):
    return dict(img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=6, h_stddev=0.3, v_stddev=0.155,
                hierarchical_sample=hier, sample_dist="gaussian")


def test_v1_generator_and_other_shapes_and_the_exact_fp32_mode(x3, monkeypatch):
    """generator_v1 inherits the entry points (its NeRF mapping network has no nerf_rgb head, which sigma does not depend on);
    other widths return the autograd gradient of their own forward; SIREN_FWD_MODE "f32" raises instead of falling back"""
    from cips3d_amd.generator import NeRFNetwork
    from test_generator_v1_cpu import seeded_generator_v1
    ops = x3
    d = dev()
    g = torch.Generator().manual_seed(10)
    b, P = 2, 300
    pts = ((torch.rand(b, P, 3, generator=g) - 0.5) * 0.3).to(d)
    G1 = seeded_generator_v1(9, device=d)
    zs = _zs(91, d)
    sig, grad = G1.density_gradient(zs, pts)
    vol, vgrad = G1.density_grid(zs, 5, return_gradient=True)
    with torch.no_grad():
        styles = G1.siren._sigma_args(G1._map_nerf(zs["z_nerf"]))
        ref_s, ref_g = ops.siren_sigma_grad(pts, *G1.siren._siren_args(styles))
        ref = G1.siren(pts, G1.mapping_network(**zs))[..., 32]
    assert torch.isfinite(ref_g).all() and torch.equal(sig, ref_s) and torch.equal(grad, ref_g) and torch.equal(sig, ref)
    assert vol.shape == (2, 5, 5, 5) and vgrad.shape == (2, 5, 5, 5, 3) and torch.equal(vol, G1.density_grid(zs, 5))
    geo = G1.geometry(zs, **_geometry_kwargs(False))
    assert geo.depth.shape == (2, 1, 8, 8) and geo.normals.shape == (2, 3, 8, 8)
    assert all(bool(torch.isfinite(v).all()) for v in (geo.depth, geo.points, geo.sigma, geo.normals))

    torch.manual_seed(10)
    net = NeRFNetwork(hidden_dim=64, rgb_dim=32, style_dim=128).to(d)
    assert not net.fused
    sd = _styles(torch.randn(b, 128, generator=g).to(d))
    p = pts.clone().requires_grad_(True)
    ref_s = net(p, sd)[..., -1]
    ref_g, = torch.autograd.grad(ref_s.sum(), p)
    sig, grad = net.density_gradient(pts, sd)
    assert sig.grad_fn is None and grad.grad_fn is None and not grad.requires_grad
    assert torch.allclose(sig, ref_s.detach(), rtol=1e-5) and torch.allclose(grad, ref_g, rtol=1e-5)
    gx, gy, gz = (((torch.rand(k, generator=g) - 0.5) * 0.3).to(d) for k in (4, 3, 5))
    ls, lg = net.density_gradient_lattice(gx, gy, gz, sd)
    rs, rg = net.density_gradient(_lattice_points(gx, gy, gz, b), sd)
    assert ls.shape == (b, 4, 3, 5) and lg.shape == (b, 4, 3, 5, 3)
    assert torch.allclose(ls.reshape(b, -1), rs, rtol=1e-5) and torch.allclose(lg.reshape(b, -1, 3), rg, rtol=1e-5)

    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "f32")
    G, _, style = _siren_inputs(12, b, P)
    Gd = G.to(d)
    with pytest.raises(RuntimeError, match="fp32"):
        Gd.siren.density_gradient(pts, _styles(style.to(d)))
    with pytest.raises(RuntimeError, match="fp32"):
        Gd.siren.density_gradient_lattice(gx, gy, gz, _styles(style.to(d)))


@pytest.mark.parametrize("hier", [False, True])
def test_geometry(hier, x3):
    """r8, S = 6, b = 2 (last_back: the weights of a ray sum to one, so its depth is a mean of its sample depths):
    shapes, dtypes, no grad_fn; points == origin + dirs * depth rebuilt from ops.rays_fwd; sigma and normals == what
    ops.siren_sigma_grad gives at those points, negated and normalised; the flat path's depth against the oracle's
    rays -> siren -> integrate chain; ray_start <= depth <= ray_end with centred samples; exact zeros for a zero gradient.
    Random numbers — the rule geometry() documents: after the same seed it returns forward()'s pitch_yaw and leaves the
    generators in the state forward() (whole images, one shot, under no_grad) leaves them in."""
    ops = x3
    d = dev()
    b, img, S = 2, 8, 6
    n, E = img * img, (2 * S if hier else S)
    G = seeded_generator(13)
    g = torch.Generator().manual_seed(131)
    zs = {"z_nerf": torch.randn(b, 256, generator=g), "z_inr": torch.randn(b, 512, generator=g)}
    rand = dict(jitter=torch.rand(b, n, S, 1, generator=g), theta=torch.randn(b, 1, generator=g), phi=torch.randn(b, 1, generator=g),
                noise_c=torch.randn(b, n, S, 1, generator=g), u=torch.rand(b * n, S, generator=g),
                noise_f=torch.randn(b, n, E, 1, generator=g))
    if not hier:
        with torch.no_grad():
            sd = dict(G.named_parameters())
            r = orc.rays(b, img, 12, 0.88, 1.12, S, rand["jitter"], rand["theta"], rand["phi"], 0.3, 0.155)
            out = orc.siren(sd, r["points"].reshape(b, n * S, 3), orc.mapping_nerf(sd, zs["z_nerf"])).reshape(b, n, S, 33)
            ref_depth = orc.integrate(out, r["z"], rand["noise_f"], 0.0, last_back=True)[1].view(b, n)
    G = G.to(d)
    G.device = d
    zs = {k: v.to(d) for k, v in zs.items()}
    rand = {k: v.to(d) for k, v in rand.items()}
    kw = _geometry_kwargs(hier)
    calls, inr = [], G._map_inr
    G._map_inr = lambda z: (calls.append(1), inr(z))[1]
    try:
        geo = G.geometry(zs, **kw, last_back=True, rand_override=rand)
    finally:
        del G._map_inr
    assert not calls
    for name, c in (("depth", 1), ("points", 3), ("sigma", 1), ("normals", 3)):
        v = getattr(geo, name)
        assert v.shape == (b, c, img, img) and v.dtype == torch.float32 and v.grad_fn is None and not v.requires_grad, name
        assert torch.isfinite(v).all(), name
    assert geo.pitch_yaw.shape == (b, 2)

    def rows(v):                     # (b,c,H,W) -> (b,n,c)
        return v.permute(0, 2, 3, 1).reshape(b, n, -1)
    depth = rows(geo.depth)
    pitch_yaw, origin, c2w = ops.camera_pose(rand["theta"], rand["phi"], False, 0.3, math.pi * 0.5, 0.155, math.pi * 0.5)
    xg, yg, zg = ops.pixel_grids(img, img, S, 0.88, 1.12, d)
    zc = float((-torch.ones(1) / np.tan((2 * math.pi * 12 / 360) / 2)).item())
    dirs = ops.rays_fwd(xg, yg, zg, zc, c2w, rand["jitter"].reshape(b, n, S), b, img, img, S)[2]
    pts = origin.view(b, 1, 3) + dirs * depth
    assert torch.equal(geo.pitch_yaw, pitch_yaw)
    assert torch.equal(rows(geo.points), pts)
    with torch.no_grad():
        sig, grad = ops.siren_sigma_grad(pts, *G.siren._siren_args(G._map_nerf(zs["z_nerf"])))
    nrm = grad.norm(dim=-1, keepdim=True)
    assert bool((nrm > 0).all())
    assert torch.equal(rows(geo.sigma), sig.unsqueeze(-1)) and torch.equal(rows(geo.normals), -grad / nrm)
    assert float((rows(geo.normals).norm(dim=-1) - 1).abs().max()) < 1e-6
    # jittered samples: a sample leaves its linspace depth by at most half a step (perturb_points: (u - 0.5) * step, u in [0, 1)),
    # resampled ones lie between coarse ones, and with last_back the weights sum to one, so the depth is a mean of depths
    # inside [ray_start - step / 2, ray_end + step / 2]; the slack is the rounding of that E-term fp32 sum
    half, slack = 0.5 * (1.12 - 0.88) / (S - 1), (E + 1) * 2.0 ** -24
    assert float(depth.min()) >= (0.88 - half) * (1 - slack) and float(depth.max()) <= (1.12 + half) * (1 + slack)
    if not hier:
        e = max_rel(depth.squeeze(-1), ref_depth)
        print(f"geometry depth (flat, r8, S=6) against the oracle: max_rel {e:.2e}")
        assert e < 5e-5

    # centred samples (jitter 0.5: the sample depths are the linspace itself; resampled ones lie between them): the depth is a
    # mean of depths inside [ray_start, ray_end]; the slack is the rounding of that E-term fp32 sum, (E + 1) * 2^-24 relative
    geo_c = G.geometry(zs, **kw, last_back=True, rand_override={**rand, "jitter": torch.full_like(rand["jitter"], 0.5)})
    assert float(geo_c.depth.min()) >= 0.88 * (1 - slack) and float(geo_c.depth.max()) <= 1.12 * (1 + slack)

    # the same seed: forward()'s camera, and the generators left where forward() leaves them
    # (psi < 1: the 10 000 latents of the average styles are drawn first, both z_nerf and z_inr, as forward() draws them)
    for psi in (1, 0.5):
        torch.manual_seed(7)
        geo_s = G.geometry(zs, **kw, psi=psi)
        after_geo = (torch.rand(1, device=d), torch.rand(1))
        torch.manual_seed(7)
        with torch.no_grad():
            _, py = G(zs, **kw, psi=psi)
        after_fwd = (torch.rand(1, device=d), torch.rand(1))
        assert torch.equal(geo_s.pitch_yaw, py) and not torch.equal(geo_s.pitch_yaw, geo.pitch_yaw), psi
        assert torch.equal(after_geo[0], after_fwd[0]) and torch.equal(after_geo[1], after_fwd[1]), psi

    # a zero gradient (sigma head weights zero: sigma is its bias everywhere) gives exact zeros, not NaN
    with torch.no_grad():
        G.siren.final_layer.weight.zero_()
    geo_z = G.geometry(zs, **kw, rand_override=rand)
    assert bool((geo_z.normals == 0).all()) and bool((geo_z.sigma == G.siren.final_layer.bias).all())
