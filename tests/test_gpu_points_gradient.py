"""GPU: gradients w.r.t. the sample points and the camera — siren_bwd_points_x3_kernel (cips_siren_bwd_points_x3, _rays) against
fp64 autograd of the oracle's SIREN, its buffers, its rays form against its points form BIT FOR BIT, rays_bwd_cam_kernel
(cips_rays_bwd_cam) against the fp64 sum, the autograd Functions against the fp64 yardstick that
tests/test_points_gradient_yardstick_cpu.py restates and validates, and the generator's public calls on top of them."""
import ctypes as C
import math

import pytest
import torch

from conftest import max_rel, rel_err, seeded_generator
from oracle import cips3d_oracle as orc
from test_gpu_density_gradient import BAR, SENTINEL, SHAPES, _scaled_inputs, _styles
from test_gpu_density_gradient import _case as _sigma_case
from test_gpu_kernels import TOL, _siren_inputs, dev
from test_points_gradient_yardstick_cpu import apply_camera, camera_space64, render64, sd64

pytestmark = pytest.mark.gpu
FOV, RAY_START, RAY_END = 12, 0.88, 1.12
ZC = float((-torch.ones(1) / torch.tan(torch.tensor((2 * math.pi * FOV / 360) / 2))).item())


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _vjp(G, pts, style, up, dtype):
    """J^T up of the oracle's SIREN w.r.t. the points by autograd in `dtype`, on the CPU -> (b,P,3) fp64"""
    sd = {k: v.detach().to(dtype) for k, v in G.named_parameters()}
    p = pts.to(dtype).clone().requires_grad_(True)
    return torch.autograd.grad((orc.siren(sd, p, style.to(dtype)) * up.to(dtype)).sum(), p)[0].double()


_REF = {}


def _case(seed, b, P):
    """inputs and references of one shape, computed once and shared: G (CPU), pts, style, up (b,P,33), ref64, ref32"""
    key = (seed, b, P)
    if key not in _REF:
        G, pts, style = _siren_inputs(seed, b, P)
        up = torch.randn(b, P, 33, generator=torch.Generator().manual_seed(seed + 1000))
        _REF[key] = (G, pts, style, up, _vjp(G, pts, style, up, torch.float64), _vjp(G, pts, style, up, torch.float32))
    return _REF[key]


def _err(own, ref64):
    """the worst image's max |own - ref64| / max |ref64|"""
    own = own.detach().double().cpu()
    return max(float((own[i] - ref64[i]).abs().max() / ref64[i].abs().max()) for i in range(ref64.shape[0]))


def _args(G, style):
    Gd = G.to(dev())
    with torch.no_grad():
        return Gd.siren._siren_args(_styles(style.to(dev())))


def _own(ops, args, pts, up):
    t = ops._siren_prep(args)
    d = dev()
    b, P, _ = pts.shape
    return ops.siren_bwd_points(t, up[..., :32].contiguous().to(d), up[..., 32].contiguous().to(d), b, P, points=pts.to(d))


@pytest.mark.parametrize("trig", [0, 1, 3])
@pytest.mark.parametrize("b,P", SHAPES)
def test_kernel_against_fp64_autograd_of_the_oracle(trig, b, P, x3, monkeypatch):
    """upstream randn(b,P,33); per image max |own - ref64| / max |ref64| < 1e-4 (the standing bar for free-running SIREN
    gradients); the fp32 oracle's own distance is printed next to it.  Measured on MI355X: see DESIGN section 3."""
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    G, pts, style, up, ref64, ref32 = _case(5, b, P)
    own = _own(ops, _args(seeded_generator(5), style), pts, up)
    e_own, e_orc = _err(own, ref64), _err(ref32, ref64)
    print(f"points VJP trig={trig} ({b}, {P}): max err / max |ref64|  kernel {e_own:.2e}  oracle(fp32) {e_orc:.2e}")
    assert own.shape == (b, P, 3) and torch.isfinite(own).all()
    assert e_own < BAR


def _raw(ops, t, pts, dfeat, dsig):
    """cips_siren_bwd_points_x3 through ctypes into a NaN-filled buffer with 64 trailing sentinel floats -> dpoints, the tail"""
    from cips3d_amd import _lib
    B, P, _ = pts.shape
    out = torch.full((B * P * 3 + 64,), float("nan"), device=pts.device)
    out[B * P * 3:] = SENTINEL
    sw = ops._siren_struct(t)
    _lib.check(_lib.load().cips_siren_bwd_points_x3(C.byref(sw), ops._p(pts), ops._p(dfeat), ops._p(dsig), ops._p(out), B, P,
                                                    ops._stream()), "cips_siren_bwd_points_x3")
    torch.cuda.synchronize()
    return out[:B * P * 3].view(B, P, 3), out[B * P * 3:]


@pytest.mark.parametrize("trig", [0, 1, 3])
@pytest.mark.parametrize("b,P", SHAPES)
def test_buffers_are_written_exactly_and_zero_upstream_gives_exact_zeros(trig, b, P, x3, monkeypatch):
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    d = dev()
    G, pts, style, up, _, _ = _case(5, b, P)
    up = up.clone()
    dead = torch.zeros(b, P, dtype=torch.bool)
    dead[:, ::7] = True
    dead[:, -1] = True                      # the last point of the ragged tail
    dead[0, 32:96] = True                   # a whole wave-step of image 0
    up[dead] = 0.0
    args = _args(seeded_generator(5), style)
    t = ops._siren_prep(args)
    dfeat, dsig, p = up[..., :32].contiguous().to(d), up[..., 32].contiguous().to(d), pts.to(d)
    own, tail = _raw(ops, t, p, dfeat, dsig)
    assert torch.isfinite(own).all()                                    # every element written ...
    assert bool((tail == SENTINEL).all())                               # ... nothing behind
    assert bool((own[dead.to(d)] == 0).all()) and bool((own[~dead.to(d)].abs().sum(-1) > 0).all())
    assert torch.equal(own, ops.siren_bwd_points(t, dfeat, dsig, b, P, points=p))


@pytest.mark.parametrize("trig", [0, 1, 3])
def test_unit_sigma_upstream_agrees_with_the_sigma_gradient_kernel(trig, x3, monkeypatch):
    """dfeat = 0, dsigma = 1 is d sigma / d point: both kernels within the bar of the same fp64 gradient (two kernels, other
    operand planes: no bit equality)"""
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    b, P = SHAPES[1]
    G, pts, style, ref64, _ = _sigma_case(5, b, P)
    args = _args(seeded_generator(5), style)
    up = torch.zeros(b, P, 33)
    up[..., 32] = 1.0
    own = _own(ops, args, pts, up)
    other = ops.siren_sigma_grad(pts.to(dev()), *args)[1]
    e_own, e_other = _err(own, ref64), _err(other, ref64)
    print(f"d sigma / d point trig={trig}: points-VJP kernel {e_own:.2e}, sigma-gradient kernel {e_other:.2e} (against fp64)")
    assert e_own < BAR and e_other < BAR


_BASE = {}


@pytest.mark.parametrize("scale_w,scale_ws", [(37.0, 1.0), (3e-4, 1.0), (1.0, 1e-3), (1.0, 1e3)])
def test_vjp_does_not_depend_on_the_magnitude_of_the_weights(scale_w, scale_ws, x3, monkeypatch):
    """W1 / Wc / Wf x 37 and x 3e-4 with the FiLM gains compensated, ws x 1e-3 and x 1e3: the error against fp64 of the SCALED
    network stays under 1e-4 and within 4x of the unscaled weights' (tests/test_points_gradient_yardstick_cpu.py: the fp32 oracle
    itself stays inside this) — a subnormal or overflowed operand plane, or a lost factor of the hardware-sine staging, costs
    orders of magnitude"""
    ops = x3
    b, P = 2, 4096 + 64
    G0, pts, style, up, ref0, _ = _case(11, b, P)
    G, _, _ = _scaled_inputs(scale_w, scale_ws, b, P)
    ref = _vjp(G, pts, style, up, torch.float64)
    for trig in (0, 1, 3):
        monkeypatch.setattr(ops, "TRIG_MODE", trig)
        if trig not in _BASE:
            _BASE[trig] = _err(_own(ops, _args(seeded_generator(11), style), pts, up), ref0)
        own = _own(ops, _args(G, style), pts, up)
        e = _err(own, ref)
        print(f"points VJP scale_w={scale_w} scale_ws={scale_ws} trig={trig}: max err / max |ref64| {e:.2e} (unscaled {_BASE[trig]:.2e})")
        assert torch.isfinite(own).all()
        assert _BASE[trig] < BAR and e < BAR
        assert e <= 4 * _BASE[trig]


def _grids(img, S, d):
    return (torch.linspace(-1, 1, img, device=d), torch.linspace(1, -1, img, device=d), torch.linspace(RAY_START, RAY_END, S, device=d))


def _camera(b, g):
    """a cam2world (b,4,4) fp32 of the oracle's drawn camera"""
    return orc.rays(b, 2, FOV, RAY_START, RAY_END, 2, torch.rand(b, 4, 2, 1, generator=g), torch.randn(b, 1, generator=g),
                    torch.randn(b, 1, generator=g), 0.3, 0.155)["cam2world"].contiguous()


@pytest.mark.parametrize("img,S,b", [(8, 4, 2), (10, 5, 3)])
def test_rays_form_equals_the_points_form_and_the_camera_reduction(img, S, b, x3):
    """coarse form (grids + jitter) at ops.rays_fwd's points, zvals form at the resampler's origin + direction * depth points:
    torch.equal (100 rays: no multiple of the 32-ray granule).  cips_rays_bwd_cam against the fp64 sum of dpoint x [q, 1] over
    the same dpoints: per image and column of the 3 x 4 block max_rel < 1e-5 (an fp32 sum of at most 1 500 terms); row 3 zeros;
    two calls give the same bits."""
    ops = x3
    d = dev()
    n = img * img
    P = n * S
    g = torch.Generator().manual_seed(40 + img)
    G, _, style = _siren_inputs(7, b, 1)
    t = ops._siren_prep(_args(G, style))
    xg, yg, zg = _grids(img, S, d)
    c2w = _camera(b, g).to(d)
    jit = torch.rand(b, n, S, generator=g).to(d)
    dfeat, dsig = torch.randn(b, P, 32, generator=g).to(d), torch.randn(b, P, generator=g).to(d)
    pts, z, dirs = ops.rays_fwd(xg, yg, zg, ZC, c2w, jit, b, img, img, S)
    # fine depths and the points the resampler materialises for them (origin + direction * depth, its sum, its order)
    fine_z, fine_pts = ops.resample_fwd(torch.randn(b * n, S, generator=g).to(d), z.view(b * n, S), None, 0.0,
                                        torch.rand(b * n, S, generator=g).to(d), c2w[:, :3, 3].contiguous(), dirs.view(b * n, 3),
                                        b, n, S)
    fine_z, fine_pts = fine_z.view(b, n, S), fine_pts.view(b, P, 3)
    q64, _, d64 = camera_space64(b, img, S, jit.cpu().view(b, n, S, 1))
    for name, rp, points, q in (("coarse", ops._ray_params(xg, yg, zg, ZC, c2w, jit, img, img, S), pts.view(b, P, 3), q64),
                                ("zvals", ops._ray_params(xg, yg, zg, ZC, c2w, None, img, img, S, fine_z), fine_pts,
                                 d64.unsqueeze(2) * fine_z.cpu().double().view(b, n, S, 1))):
        dp_rays = ops.siren_bwd_points(t, dfeat, dsig, b, P, rays=rp)
        dp_pts = ops.siren_bwd_points(t, dfeat, dsig, b, P, points=points.contiguous())
        assert torch.isfinite(dp_rays).all() and float(dp_rays.abs().max()) > 0
        assert torch.equal(dp_rays, dp_pts), name
        dcam = ops.rays_bwd_cam(rp, dp_rays, b)
        dp64 = dp_rays.double().cpu()
        ref = torch.einsum("bpi,bpj->bij", dp64, torch.cat([q.reshape(b, P, 3), torch.ones(b, P, 1, dtype=torch.float64)], -1))
        own = dcam.double().cpu()
        e = max(float((own[i, :3, j] - ref[i, :, j]).abs().max() / ref[i, :, j].abs().max()) for i in range(b) for j in range(4))
        print(f"rays_bwd_cam {name} r{img} S={S} b={b}: worst column max_rel {e:.2e}")
        assert dcam.shape == (b, 4, 4) and bool((dcam[:, 3] == 0).all())
        assert e < 1e-5
        assert torch.equal(dcam, ops.rays_bwd_cam(rp, dp_rays, b))


def _march_case(img, S, b, d):
    g = torch.Generator().manual_seed(100 + img + S)
    n = img * img
    G = seeded_generator(11)
    D = dict(style=torch.randn(b, 128, generator=g), jitter=torch.rand(b, n, S, 1, generator=g),
             theta=torch.randn(b, 1, generator=g), phi=torch.randn(b, 1, generator=g), noise=torch.randn(b, n, S, 1, generator=g),
             up=torch.randn(b, n, 32, generator=g))
    D["c2w"] = orc.rays(b, img, FOV, RAY_START, RAY_END, S, D["jitter"], D["theta"], D["phi"], 0.3, 0.155)["cam2world"].contiguous()
    return G, D


def _poison(d):
    """a large NaN-filled block through the caching allocator and back: what torch.empty hands out next holds NaNs"""
    x = torch.full((48 << 20,), float("nan"), device=d)
    del x


@pytest.mark.parametrize("img,S,b,noise_std,clamp,flags", [(8, 4, 2, 0.0, "relu", 0), (16, 24, 2, 0.3, "relu", 0),
                                                           (10, 5, 3, 0.2, "softplus", 3), (24, 12, 1, 0.0, "relu", 1)])
def test_ray_march_camera_gradient_against_the_yardstick(img, S, b, noise_std, clamp, flags, x3):
    """the four cases of test_fused_march_forward_backward, loss (fea * up).sum() through net.march: cam2world.grad against the
    fp64 yardstick to rel_err < 1e-3 (TOL of test_gpu_kernels.py, the bar of the reduced parameter gradients on these cases);
    every SIREN parameter / style gradient of that backward torch.equal to a run without the camera gradient; relu: finite and
    the same bits across two runs although the allocator hands out NaN-filled blocks (a read of an unwritten dead row shows)"""
    ops = x3
    d = dev()
    n = img * img
    G, D = _march_case(img, S, b, d)
    sd = sd64(G)
    q, z, d_cam = camera_space64(b, img, S, D["jitter"])
    c64 = D["c2w"].double().requires_grad_(True)
    p, dirs, orig = apply_camera(q, d_cam, c64)
    fea = render64(sd, D["style"].double(), p, z, orig, dirs, D["noise"].double(), noise_std, clamp, bool(flags & 1), bool(flags & 2))[0]
    ref, = torch.autograd.grad((fea * D["up"].double()).sum(), c64)

    net = G.to(d).siren
    xg, yg, zg = _grids(img, S, d)
    geom = (b, img, img, S, ZC, float(noise_std), ops._CLAMP[clamp], flags, True)
    jd, nd, upd = D["jitter"].to(d).reshape(b, n, S).contiguous(), D["noise"].to(d).reshape(b, n, S).contiguous(), D["up"].to(d)

    def run(cam_grad):
        for prm in net.parameters():
            prm.grad = None
        std = D["style"].to(d).requires_grad_(True)
        c2w = D["c2w"].to(d).requires_grad_(cam_grad)
        f, _ = net.march({"nerf_w0": std, "nerf_w1": std, "nerf_rgb": std}, geom, xg, yg, zg, c2w, jd, nd)
        if clamp == "relu":
            _poison(d)
        (f * upd).sum().backward()
        torch.cuda.synchronize()
        return c2w.grad, [std.grad.clone()] + [prm.grad.clone() for prm in net.parameters()]

    g_cam, g_par = run(True)
    g_cam2, _ = run(True)
    none, g_par0 = run(False)
    e = rel_err(g_cam[:, :3], ref[:, :3])
    print(f"march camera gradient r{img} S={S} b={b} noise {noise_std} {clamp} flags {flags}: rel err {e:.2e}")
    assert none is None and g_cam.shape == (b, 4, 4) and torch.isfinite(g_cam).all() and bool((g_cam[:, 3] == 0).all())
    assert torch.equal(g_cam, g_cam2)
    assert all(torch.equal(a, c) for a, c in zip(g_par, g_par0))
    assert e < TOL


@pytest.mark.parametrize("clamp,noise_std", [("relu", 0.0), ("softplus", 0.2)])
def test_hierarchical_camera_gradient_against_the_yardstick(clamp, noise_std, x3):
    """evaluate_rays (coarse: grids + jitter; fine: zvals) + CompositeFunction, S = 4, r8, b = 2, the fine depths pinned to the
    yardstick's through ops.resample_debug: cam2world.grad (the sum of both passes') to rel_err < 1e-3, parameter gradients
    torch.equal with and without it"""
    ops = x3
    d = dev()
    img, S, b = 8, 4, 2
    n = img * img
    G, D = _march_case(img, S, b, d)
    g = torch.Generator().manual_seed(77)
    noise_c, u, noise_f = torch.randn(b, n, S, 1, generator=g), torch.rand(b * n, S, generator=g), torch.randn(b, n, 2 * S, 1, generator=g)
    sd = sd64(G)
    q, z, d_cam = camera_space64(b, img, S, D["jitter"])
    c64 = D["c2w"].double().requires_grad_(True)
    p, dirs, orig = apply_camera(q, d_cam, c64)
    fea, fz = render64(sd, D["style"].double(), p, z, orig, dirs, noise_f.double(), noise_std, clamp,
                       hier=(noise_c.double(), u.double(), None))
    ref, = torch.autograd.grad((fea * D["up"].double()).sum(), c64)

    net = G.to(d).siren
    xg, yg, zg = _grids(img, S, d)
    jd, upd = D["jitter"].to(d).reshape(b, n, S).contiguous(), D["up"].to(d)
    cm = ops._CLAMP[clamp]

    def run(cam_grad):
        for prm in net.parameters():
            prm.grad = None
        std = D["style"].to(d).requires_grad_(True)
        sdict = {"nerf_w0": std, "nerf_w1": std, "nerf_rgb": std}
        c2w = D["c2w"].to(d).requires_grad_(cam_grad)
        rays = (sdict, (b, img, img, S, ZC), xg, yg, zg, c2w)
        feat_c, sig_c, z_c = net.evaluate_rays(*rays, jitter=jd)
        with torch.no_grad(), ops.resample_debug(pin=[fz.float()]):
            rp = ops._ray_params(xg, yg, zg, ZC, c2w.detach(), None, img, img, S)
            drawn = ops.resample_fwd(sig_c.view(b * n, S), z_c.view(b * n, S), noise_c.to(d).reshape(b * n, S) if noise_std else None,
                                     noise_std, u.to(d), None, None, b, n, S, cm, rays=rp)[0]
            fine_z = ops.fine_z_debug(drawn)
        feat_f, sig_f, _ = net.evaluate_rays(*rays, zvals=fine_z.view(b, n * S))
        out = ops.CompositeFunction.apply(feat_c.view(b * n, S, 32), sig_c.view(b * n, S), z_c.view(b * n, S),
                                          feat_f.view(b * n, S, 32), sig_f.view(b * n, S), fine_z.view(b * n, S),
                                          noise_f.to(d).reshape(b * n, 2 * S) if noise_std else None, noise_std, cm, 0)
        if clamp == "relu":
            _poison(d)
        (out[0].view(b, n, 32) * upd).sum().backward()
        torch.cuda.synchronize()
        return c2w.grad, [std.grad.clone()] + [prm.grad.clone() for prm in net.parameters()]

    g_cam, g_par = run(True)
    g_cam2, _ = run(True)
    _, g_par0 = run(False)
    e = rel_err(g_cam[:, :3], ref[:, :3])
    print(f"hierarchical camera gradient {clamp} noise {noise_std}: rel err {e:.2e}")
    assert torch.isfinite(g_cam).all() and torch.equal(g_cam, g_cam2)
    assert all(torch.equal(a, c) for a, c in zip(g_par, g_par0))
    assert e < TOL


# ---- generator level: plumbing ----
IMG, S_, B_ = 8, 6, 2
KW = dict(img_size=IMG, fov=FOV, ray_start=RAY_START, ray_end=RAY_END, num_steps=S_, h_stddev=0.3, v_stddev=0.155,
          sample_dist="gaussian", clamp_mode="softplus")


def _gen_inputs(d, hier):
    g = torch.Generator().manual_seed(500)
    n, E = IMG * IMG, (2 * S_ if hier else S_)
    zs = {"z_nerf": torch.randn(B_, 256, generator=g).to(d), "z_inr": torch.randn(B_, 512, generator=g).to(d)}
    rand = dict(jitter=torch.rand(B_, n, S_, 1, generator=g), theta=torch.randn(B_, 1, generator=g), phi=torch.randn(B_, 1, generator=g),
                noise_c=torch.randn(B_, n, S_, 1, generator=g), u=torch.rand(B_ * n, S_, generator=g),
                noise_f=torch.randn(B_, n, E, 1, generator=g))
    G0 = torch.randn(B_, 3, IMG, IMG, generator=g).to(d)
    return zs, {k: v.to(d) for k, v in rand.items()}, G0


def _explicit(G, ops, d, zs, rand, G0, hier, pos, look, pins, fz):
    c, l = pos.clone().to(d).requires_grad_(True), look.clone().to(d).requires_grad_(True)
    G.zero_grad(set_to_none=True)
    first, rec = "gates" not in pins, []               # the first run records the head's gates, the later ones take them
    with ops.gate_debug(pin=None if first else pins["gates"], rec=rec if first else None), \
            ops.resample_debug(pin=[fz] if fz is not None else None):
        imgs, _ = G.forward_camera_pos_and_lookup(zs, h_mean=math.pi / 2, v_mean=math.pi / 2, hierarchical_sample=hier,
                                                  camera_pos=c, camera_lookup=l, rand_override=rand, **KW)
    if first:
        pins["gates"] = rec
    assert imgs.grad_fn is not None
    (imgs * G0).sum().backward()
    torch.cuda.synchronize()
    return imgs.detach(), c.grad, l.grad


POS = torch.tensor([[0.10, 0.15, 1.00], [-0.20, 0.05, 0.95]])
LOOK = torch.tensor([[-0.10, -0.20, -1.00], [0.25, -0.05, -0.90]])


@pytest.mark.parametrize("hier", [False, True])
def test_generator_explicit_camera_gradients(hier, x3, monkeypatch):
    """forward_camera_pos_and_lookup with camera_pos / camera_lookup requiring grad: finite, non-zero gradients that agree with
    the same call under MARCH_FUSED = False to rel_err < 1e-3 — that run takes the "points" form, whose torch-formed points and
    SirenFunction's dpoints are an independent route (the head's LeakyReLU gates and the fine depths are those of the first run)"""
    ops = x3
    d = dev()
    G = seeded_generator(21, device=d)
    G.device = d
    zs, rand, G0 = _gen_inputs(d, hier)
    fz = None
    if hier:
        rec = []
        with torch.no_grad(), ops.resample_debug(rec=rec):
            G.forward_camera_pos_and_lookup(zs, h_mean=math.pi / 2, v_mean=math.pi / 2, hierarchical_sample=True,
                                            camera_pos=POS.to(d), camera_lookup=LOOK.to(d), rand_override=rand, **KW)
        fz = rec[0]
    pins = {}
    imgs, gc, gl = _explicit(G, ops, d, zs, rand, G0, hier, POS, LOOK, pins, fz)
    monkeypatch.setattr(ops, "MARCH_FUSED", False)
    imgs_p, gc_p, gl_p = _explicit(G, ops, d, zs, rand, G0, hier, POS, LOOK, pins, fz)
    e = (max_rel(imgs, imgs_p), rel_err(gc, gc_p), rel_err(gl, gl_p))
    print(f"generator explicit camera hier={hier}: fused vs points form: imgs {e[0]:.2e} camera_pos.grad {e[1]:.2e} camera_lookup.grad {e[2]:.2e}")
    for v in (gc, gl, gc_p, gl_p):
        assert v.shape == (B_, 3) and torch.isfinite(v).all() and float(v.abs().max()) > 0
    assert e[0] < TOL and e[1] < TOL and e[2] < TOL


def test_generator_mean_angles_and_the_matching_explicit_camera(x3):
    """forward(h_mean=tensor, v_mean=tensor), 0-dim and (b,1), leaves both grads; the images equal the explicit camera's for the
    matching pose (position on the unit sphere at those angles, looking at the origin), and the chain rule through that pose
    gives the same angle gradients"""
    ops = x3
    d = dev()
    G = seeded_generator(21, device=d)
    G.device = d
    zs, rand, G0 = _gen_inputs(d, False)
    hm = torch.tensor(math.pi / 2 + 0.1, device=d, requires_grad=True)
    vm = torch.tensor([[math.pi / 2 - 0.05], [math.pi / 2 + 0.12]], device=d, requires_grad=True)
    rec = []
    with ops.gate_debug(rec=rec):
        imgs, _ = G(zs, hierarchical_sample=False, h_mean=hm, v_mean=vm, rand_override=rand, **KW)
    (imgs * G0).sum().backward()
    assert hm.grad is not None and vm.grad is not None and hm.grad.shape == () and vm.grad.shape == (B_, 1)
    assert torch.isfinite(hm.grad) and torch.isfinite(vm.grad).all() and float(hm.grad.abs()) > 0 and float(vm.grad.abs().min()) > 0
    # the matching explicit pose, built differentiably from fresh leaves
    hm2, vm2 = hm.detach().clone().requires_grad_(True), vm.detach().clone().requires_grad_(True)
    theta, phi = rand["theta"] * 0.3 + hm2, torch.clamp(rand["phi"] * 0.155 + vm2, 1e-5, math.pi - 1e-5)
    pos = torch.cat([torch.sin(phi) * torch.cos(theta), torch.cos(phi), torch.sin(phi) * torch.sin(theta)], -1)
    G.zero_grad(set_to_none=True)
    with ops.gate_debug(pin=rec):
        imgs_e, _ = G.forward_camera_pos_and_lookup(zs, h_mean=math.pi / 2, v_mean=math.pi / 2, hierarchical_sample=False,
                                                    camera_pos=pos, camera_lookup=-pos, rand_override=rand, **KW)
    (imgs_e * G0).sum().backward()
    e = (max_rel(imgs, imgs_e), rel_err(hm.grad, hm2.grad), rel_err(vm.grad, vm2.grad))
    print(f"generator h_mean / v_mean against the matching explicit camera: imgs {e[0]:.2e} h_mean.grad {e[1]:.2e} v_mean.grad {e[2]:.2e}")
    assert max(e) < TOL


def test_points_gradient_through_the_modules_and_what_is_refused(x3, monkeypatch):
    """G.siren(points.requires_grad_(), styles) and .evaluate leave points.grad (against fp64 autograd of the oracle); another
    width returns the autograd gradient of its own forward; the freeze variant leaves camera_pos.grad None; generator_v1 runs the
    explicit-camera case; double backward raises; SIREN_FWD_MODE "f32" raises instead of falling back"""
    from cips3d_amd.generator import NeRFNetwork
    from test_generator_v1_cpu import seeded_generator_v1
    ops = x3
    d = dev()
    b, P = 2, 300
    G, pts, style, up, ref64, _ = _case(12, b, P)
    Gd = seeded_generator(12, device=d)
    sdict = _styles(style.to(d))
    p = pts.to(d).requires_grad_(True)
    (Gd.siren(p, sdict) * up.to(d)).sum().backward()
    assert p.grad is not None and _err(p.grad, ref64) < BAR
    p2 = pts.to(d).requires_grad_(True)
    feat, sigma = Gd.siren.evaluate(p2, sdict)
    ((feat * up[..., :32].to(d)).sum() + (sigma * up[..., 32].to(d)).sum()).backward()
    assert torch.equal(p2.grad, p.grad)

    torch.manual_seed(10)
    net = NeRFNetwork(hidden_dim=64, rgb_dim=32, style_dim=128).to(d)
    assert not net.fused
    p3 = pts.to(d).requires_grad_(True)
    net.evaluate(p3, sdict)[1].sum().backward()
    assert p3.grad is not None and torch.isfinite(p3.grad).all() and float(p3.grad.abs().max()) > 0

    zs, rand, G0 = _gen_inputs(d, False)
    call = dict(h_mean=math.pi / 2, v_mean=math.pi / 2, hierarchical_sample=False, camera_lookup=LOOK.to(d), rand_override=rand, **KW)
    Gf = seeded_generator(21, freeze=True, device=d)
    Gf.device = d
    c = POS.clone().to(d).requires_grad_(True)
    imgs, _ = Gf.forward_camera_pos_and_lookup(zs, camera_pos=c, **call)
    (imgs * G0).sum().backward()
    assert c.grad is None

    G1 = seeded_generator_v1(9, device=d)
    G1.device = d
    c = POS.clone().to(d).requires_grad_(True)
    imgs, _ = G1.forward_camera_pos_and_lookup(zs, camera_pos=c, **call)
    (imgs * G0).sum().backward()
    assert c.grad is not None and torch.isfinite(c.grad).all() and float(c.grad.abs().max()) > 0

    p4 = pts.to(d).requires_grad_(True)
    # (a loss that is not linear in sigma: its upstream gradient depends on p4, so the first backward's result is part of a graph)
    g4, = torch.autograd.grad(Gd.siren.evaluate(p4, sdict)[1].square().sum(), p4, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g4.sum().backward()

    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "f32")
    p5 = pts.to(d).requires_grad_(True)
    out = Gd.siren.evaluate(p5, sdict)[1].sum()
    with pytest.raises(RuntimeError, match="fp32"):
        out.backward()
