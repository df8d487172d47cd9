"""CPU: the yardstick of the camera / sample-point gradients, and its validation.

The oracle's generator_forward builds its rays under no_grad and _points_forward forms the fine points under no_grad, as the
reference does, so it yields no gradient w.r.t. the camera.  The chain is restated here from the oracle's parts, in fp64:
  orc.rays (under an fp64 default dtype: differentiable in camera_pos / camera_lookup / theta_n / phi_n; or its camera-space
  samples, taken with the identity camera, under an fp64 cam2world leaf) -> orc.siren -> orc.fine_points for the DEPTHS only,
  the fine points re-formed as origins + dirs * fine_z outside no_grad -> sort, gather -> orc.integrate.
tests/test_gpu_points_gradient.py compares the kernels and the autograd Functions with it; this file validates it against
central differences, as tests/test_density_gradient_oracle_cpu.py validates its yardstick: step 1e-6 in every camera parameter
and in the coordinates of a few points, agreement better than 1e-7 of the gradient's largest entry (measured: 2e-10 .. 1.2e-8)."""
import contextlib

import pytest
import torch

from conftest import seeded_generator
from oracle import cips3d_oracle as orc

FOV, RAY_START, RAY_END, H_STD, V_STD = 12, 0.88, 1.12, 0.3, 0.155
STEP, AGREE = 1e-6, 1e-7


@contextlib.contextmanager
def fp64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def sd64(G):
    return {k: v.detach().double().cpu() for k, v in G.named_parameters()}


def rays64(b, img, S, jitter, theta_n=None, phi_n=None, camera_pos=None, camera_lookup=None, h_mean=None, v_mean=None):
    """orc.rays in fp64 (every tensor it creates is fp64 under the default dtype), differentiable in its camera arguments"""
    kw = {}
    if h_mean is not None:
        kw.update(h_mean=h_mean, v_mean=v_mean)
    with fp64_default():
        return orc.rays(b, img, FOV, RAY_START, RAY_END, S, jitter.double(), theta_n, phi_n, H_STD, V_STD,
                        camera_pos=camera_pos, camera_lookup=camera_lookup, **kw)


def camera_space64(b, img, S, jitter):
    """the camera-space samples q (b,n,S,3), their depths z (b,n,S,1) and directions (b,n,3): orc.rays with the identity camera
    (position 0, looking down -z: its cam2world is the unit matrix exactly)"""
    r = rays64(b, img, S, jitter, camera_pos=torch.zeros(b, 3, dtype=torch.float64),
               camera_lookup=torch.tensor([0., 0., -1.], dtype=torch.float64).expand(b, 3))
    assert torch.equal(r["cam2world"], torch.eye(4, dtype=torch.float64).expand(b, 4, 4))
    return r["points"], r["z"], r["dirs"]


def apply_camera(q, d_cam, c2w):
    """world points, directions and origins of camera-space samples under cam2world (b,4,4): p = R q + t"""
    b, n = d_cam.shape[:2]
    Rt = c2w[:, :3, :3].transpose(1, 2)
    t = c2w[:, :3, 3]
    return (q.reshape(b, -1, 3) @ Rt + t[:, None]).reshape(q.shape), d_cam @ Rt, t[:, None].expand(b, n, 3)


def render64(sd, style, points, z, origins, dirs, noise_f, noise_std, clamp="relu", last_back=False, white_back=False,
             hier=None):
    """points (b,n,S,3) -> pixel features (b,n,32) through orc.siren and orc.integrate, all in the dtype of its inputs.
    hier = (noise_c, u, fine_z or None): the hierarchical pass — depths from orc.fine_points (or the given ones), constants as in
    the reference; the fine points origins + dirs * fine_z with the graph of origins / dirs; merged by depth.
    -> fea, fine_z (None without hier)"""
    b, n, S, _ = points.shape
    coarse = orc.siren(sd, points.reshape(b, n * S, 3), style).reshape(b, n, S, 33)
    fz = None
    if hier is not None:
        noise_c, u, fz = hier
        if fz is None:
            with torch.no_grad():
                fz = orc.fine_points(coarse, z, noise_c, noise_std, u, origins, dirs, clamp)[1]
        fz = fz.detach().to(z.dtype).reshape(b, n, S, 1)
        fp = (origins.unsqueeze(2) + dirs.unsqueeze(2) * fz).reshape(b, n * S, 3)
        fine = orc.siren(sd, fp, style).reshape(b, n, S, 33)
        all_o, all_z = torch.cat([fine, coarse], -2), torch.cat([fz, z], -2)
        _, idx = torch.sort(all_z, dim=-2)
        z = torch.gather(all_z, -2, idx)
        coarse = torch.gather(all_o, -2, idx.expand(-1, -1, -1, 33))
    fea = orc.integrate(coarse, z, noise_f, noise_std, clamp_mode=clamp, last_back=last_back, white_back=white_back)[0]
    return fea, fz


def _draws(seed, b, img, S, hier):
    g = torch.Generator().manual_seed(seed)
    n, E = img * img, (2 * S if hier else S)
    d = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(style=d(b, 128), jitter=torch.rand(b, n, S, 1, generator=g, dtype=torch.float64), theta=d(b, 1), phi=d(b, 1),
                noise_c=d(b, n, S, 1), u=torch.rand(b * n, S, generator=g, dtype=torch.float64), noise_f=d(b, n, E, 1),
                up=d(b, n, 32), pos=torch.tensor([[0.1, 0.15, 1.0], [-0.2, 0.05, 0.95]], dtype=torch.float64)[:b],
                look=torch.tensor([[-0.1, -0.2, -1.0], [0.25, -0.05, -0.9]], dtype=torch.float64)[:b])


def _central(f, x, step=STEP):
    """central differences of the scalar f in every entry of x"""
    g = torch.zeros_like(x)
    flat, gf = x.detach().clone().reshape(-1), g.reshape(-1)
    for i in range(flat.numel()):
        hi, lo = flat.clone(), flat.clone()
        hi[i] += step
        lo[i] -= step
        gf[i] = (float(f(hi.reshape(x.shape))) - float(f(lo.reshape(x.shape)))) / (2 * step)
    return g


def _agreement(a, fd):
    return float((a - fd).abs().max() / fd.abs().max())


@pytest.mark.parametrize("hier,clamp,noise_std", [(False, "softplus", 0.2), (True, "softplus", 0.0), (False, "relu", 0.0)])
def test_yardstick_camera_gradients_against_central_differences(hier, clamp, noise_std):
    """explicit camera (position, look-at) and the drawn camera (raw angles: the same chain as h_mean / v_mean, which enter
    through theta = theta_n * stddev + mean), whole chain, fp64.  The fine depths are those of the unperturbed camera in every
    evaluation: constants, as in the reference.  (relu: no pre-activation of this case lies within the step of zero.)"""
    b, img, S = 2, 4, 4
    G = seeded_generator(3)
    sd, D = sd64(G), _draws(31, b, img, S, hier)
    fz = [None]

    def loss(pos=None, look=None, theta=None, phi=None):
        r = rays64(b, img, S, D["jitter"], theta, phi, pos, look)
        fea, z = render64(sd, D["style"], r["points"], r["z"], r["origins"], r["dirs"], D["noise_f"], noise_std, clamp,
                          hier=(D["noise_c"], D["u"], fz[0]) if hier else None)
        if hier and fz[0] is None:
            fz[0] = z
        return (fea * D["up"]).sum()

    pos, look = D["pos"].clone().requires_grad_(True), D["look"].clone().requires_grad_(True)
    g_pos, g_look = torch.autograd.grad(loss(pos=pos, look=look), (pos, look))
    e = (_agreement(g_pos, _central(lambda v: loss(pos=v, look=D["look"]), D["pos"])),
         _agreement(g_look, _central(lambda v: loss(pos=D["pos"], look=v), D["look"])))
    fz[0] = None
    th, ph = D["theta"].clone().requires_grad_(True), D["phi"].clone().requires_grad_(True)
    g_th, g_ph = torch.autograd.grad(loss(theta=th, phi=ph), (th, ph))
    e += (_agreement(g_th, _central(lambda v: loss(theta=v, phi=D["phi"]), D["theta"])),
          _agreement(g_ph, _central(lambda v: loss(theta=D["theta"], phi=v), D["phi"])))
    print(f"yardstick hier={hier} {clamp}: autograd vs central differences (step {STEP}): camera_pos {e[0]:.1e} camera_lookup {e[1]:.1e} "
          f"theta {e[2]:.1e} phi {e[3]:.1e}")
    assert float(g_pos.abs().max()) > 0 and float(g_look.abs().max()) > 0 and float(g_th.abs().min()) > 0
    assert max(e) < AGREE


def test_yardstick_cam2world_and_point_gradients_against_central_differences():
    """the matrix form (camera-space samples of the identity camera under an fp64 cam2world leaf: what the autograd Functions
    are compared with) — its 3 x 4 block against central differences, equal to the explicit-camera form's chain rule, and the
    VJP of orc.siren w.r.t. a few points"""
    b, img, S = 2, 4, 4
    G = seeded_generator(3)
    sd, D = sd64(G), _draws(32, b, img, S, False)
    q, z, d_cam = camera_space64(b, img, S, D["jitter"])
    c2w0 = rays64(b, img, S, D["jitter"], camera_pos=D["pos"], camera_lookup=D["look"])["cam2world"].detach()

    def loss(c2w):
        p, dirs, orig = apply_camera(q, d_cam, c2w)
        return (render64(sd, D["style"], p, z, orig, dirs, D["noise_f"], 0.2, "softplus")[0] * D["up"]).sum()

    c = c2w0.clone().requires_grad_(True)
    g, = torch.autograd.grad(loss(c), c)
    fd = _central(loss, c2w0)
    e_c = _agreement(g[:, :3], fd[:, :3])
    assert float(g[:, 3].abs().max()) == 0 and float(fd[:, 3].abs().max()) < 1e-9       # the points do not read row 3
    # the same loss through orc.rays' own camera: identical points, so d loss / d camera_pos is the translation column's gradient
    pos = D["pos"].clone().requires_grad_(True)
    r = rays64(b, img, S, D["jitter"], camera_pos=pos, camera_lookup=D["look"])
    g_pos, = torch.autograd.grad((render64(sd, D["style"], r["points"], r["z"], r["origins"], r["dirs"], D["noise_f"], 0.2,
                                           "softplus")[0] * D["up"]).sum(), pos)
    e_t = _agreement(g[:, :3, 3], g_pos)

    g_ = torch.Generator().manual_seed(33)
    pts = (torch.rand(b, 3, 3, generator=g_, dtype=torch.float64) - 0.5) * 0.3
    up = torch.randn(b, 3, 33, generator=g_, dtype=torch.float64)
    f = lambda p: (orc.siren(sd, p, D["style"]) * up).sum()
    p = pts.clone().requires_grad_(True)
    gp, = torch.autograd.grad(f(p), p)
    e_p = _agreement(gp, _central(f, pts))
    print(f"yardstick: cam2world vs central differences {e_c:.1e}, translation column vs camera_pos {e_t:.1e}, siren VJP w.r.t. "
          f"points vs central differences {e_p:.1e} (step {STEP})")
    assert max(e_c, e_p) < AGREE and e_t < 1e-12


def test_fp32_oracle_stays_inside_the_bar_for_the_scaled_weights():
    """the weight-magnitude cases of the GPU test (W1 / Wc / Wf x 37 and x 3e-4 with the gains compensated, ws x 1e-3 and x 1e3):
    the fp32 oracle's own VJP w.r.t. the points stays under 1e-4 of fp64 and within 4x of its unscaled error, so the rule the
    GPU test applies to the kernel is one fp32 arithmetic itself meets for these inputs"""
    from test_gpu_density_gradient import BAR, _scaled_inputs
    from test_gpu_kernels import _siren_inputs
    b, P = 2, 257
    up = torch.randn(b, P, 33, generator=torch.Generator().manual_seed(34), dtype=torch.float64)

    def err(G, pts, style, scale_ws=1.0):
        out = []
        for dt in (torch.float64, torch.float32):
            sd = {k: v.detach().to(dt) for k, v in G.named_parameters()}
            p = pts.to(dt).clone().requires_grad_(True)
            out.append(torch.autograd.grad((orc.siren(sd, p, style.to(dt)) * up.to(dt)).sum(), p)[0].double())
        return max(float((out[1][i] - out[0][i]).abs().max() / out[0][i].abs().max()) for i in range(b))

    base = err(*_siren_inputs(11, b, P))
    assert base < BAR
    for scale_w, scale_ws in [(37.0, 1.0), (3e-4, 1.0), (1.0, 1e-3), (1.0, 1e3)]:
        e = err(*_scaled_inputs(scale_w, scale_ws, b, P))
        print(f"fp32 oracle VJP scale_w={scale_w} scale_ws={scale_ws}: {e:.2e} (unscaled {base:.2e})")
        assert e < BAR and e <= 4 * base
