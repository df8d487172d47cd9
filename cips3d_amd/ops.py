"""Host-side operators over the C-ABI (include/cips3d_hip.h): thin launch wrappers plus the
torch.autograd.Functions that give the reference's Python API its backward.

PyTorch is used for device memory, streams and autograd bookkeeping only; every arithmetic
kernel on the hot path is a hand-written HIP kernel in libcips3d_hip.so.  There is no CPU
fallback: tensors must live on a ROCm device and the extension must be built.
"""
import contextlib
import ctypes as C
import math
import os
import weakref
from collections import namedtuple
from types import SimpleNamespace

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import (ConvDgradS2Desc, ConvWgradDesc, ConvX3Desc, GemmDesc, GemmX3Desc, GlinJob, GridParams, ModfcBwdJob,
                   ModfcPrepJob, RayParams, SirenGrads, SirenWeights, check)

LRELU_SLOPE = 0.2


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("cips3d_amd ops need tensors on the GPU (no CPU fallback)")
        if t.device.index != torch.cuda.current_device():
            # launches go to the CURRENT device's current stream (one process per GPU, torch.cuda.set_device(rank),
            # train.py:48): a tensor of another device would be read through the wrong context
            raise RuntimeError(f"tensor on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                               "call torch.cuda.set_device first")
        if t.dtype != torch.float32 and t.dtype not in (torch.int32, torch.int64, torch.bfloat16):
            raise RuntimeError(f"cips3d_amd ops are fp32 (got {t.dtype})")
        if not t.is_contiguous():
            raise RuntimeError("cips3d_amd ops need contiguous tensors")


def _c(t):
    return t.contiguous().float() if t is not None else None


# --------------------------------------------------------------------------------------
# H1 camera pose + rays
# --------------------------------------------------------------------------------------


def camera_pose(theta_raw, phi_raw, uniform, h_stddev, h_mean, v_stddev, v_mean):
    """raw draws (b, 1) x 2 -> pitch_yaw (b, 2), origin (b, 3), cam2world (b, 4, 4); see cips_camera_pose"""
    lib = _lib.load()
    dev = theta_raw.device
    B = theta_raw.shape[0]
    th, ph = _c(theta_raw), _c(phi_raw)
    py = torch.empty(B, 2, device=dev); origin = torch.empty(B, 3, device=dev); c2w = torch.empty(B, 4, 4, device=dev)
    check(lib.cips_camera_pose(_p(th), _p(ph), 1 if uniform else 0, float(h_stddev), float(h_mean), float(v_stddev),
                               float(v_mean), _p(py), _p(origin), _p(c2w), B, _stream()), "cips_camera_pose")
    return py, origin, c2w


_GRIDS = {}


def pixel_grids(W, H, S, ray_start, ray_end, device):
    """the three linspaces of the ray set-up (constants of the geometry), built once per geometry and device"""
    key = (W, H, S, float(ray_start), float(ray_end), str(device))
    g = _GRIDS.get(key)
    if g is None:
        g = (torch.linspace(-1, 1, W, device=device), torch.linspace(1, -1, H, device=device),
             torch.linspace(ray_start, ray_end, S, device=device))
        if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
            return g        # built inside a hipGraph capture: the tensors live in the graph's pool and hold data only
                            # during replays — never cached for eager callers
        if len(_GRIDS) > 64:
            _GRIDS.clear()
        _GRIDS[key] = g
    return g


# The `geom` of the Functions and functions that generate rays in-kernel, and the longer one of RayMarchFunction /
# RayMarchGeoFunction (a plain tuple in this order is taken too).  grad_mode: the caller's torch.is_grad_enabled(), inside a
# Function's forward it is always off; live_fwd: the caller joins the list stream (live_forward_join) whether or not a
# backward follows.
RayGeom = namedtuple("RayGeom", "B H W S zc")
MarchGeom = namedtuple("MarchGeom", RayGeom._fields + ("noise_std", "clamp_mode", "flags", "grad_mode", "live_fwd"), defaults=(False,))


def rays_fwd(xg, yg, zg, zc, cam2world, jitter, B, H, W, S):
    """-> points (B,n,S,3), z (B,n,S), dirs (B,n,3); see cips_rays_fwd."""
    lib = _lib.load()
    dev = cam2world.device
    n = H * W
    points = torch.empty(B, n, S, 3, device=dev)
    z = torch.empty(B, n, S, device=dev)
    dirs = torch.empty(B, n, 3, device=dev)
    xg, yg, zg, cam2world, jitter = _c(xg), _c(yg), _c(zg), _c(cam2world), _c(jitter)
    _chk(xg, yg, zg, cam2world, jitter)
    check(lib.cips_rays_fwd(_p(xg), _p(yg), _p(zg), float(zc), _p(cam2world), _p(jitter),
                            _p(points), _p(z), _p(dirs), B, H, W, S, _stream()), "cips_rays_fwd")
    return points, z, dirs


# --------------------------------------------------------------------------------------
# generic GEMM
# --------------------------------------------------------------------------------------
def gemm(A, Bm, Cm, M, N, K, lda, ldb, ldc, batch=1, strideA=0, strideB=0, strideC=0,
         a_kmajor=False, b_nmajor=False, alpha=1.0, bias=None, bias_m=None, act=0, slope=LRELU_SLOPE,
         act_gain=1.0, resid=None, C2=None, add=None, rgb_g=None, rgb_w=None, C_unmasked=None, mask=None):
    lib = _lib.load()
    d = GemmDesc()
    d.A, d.B, d.C = _p(A), _p(Bm), _p(Cm)
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc = lda, ldb, ldc
    d.strideA, d.strideB, d.strideC = strideA, strideB, strideC
    d.batch = batch
    d.a_kmajor = 1 if a_kmajor else 0
    d.b_nmajor = 1 if b_nmajor else 0
    d.alpha = alpha
    d.bias, d.bias_m = _p(bias), _p(bias_m)
    d.act, d.slope, d.act_gain = act, slope, act_gain
    d.resid, d.C2, d.add = _p(resid), _p(C2), _p(add)
    d.rgb_g, d.rgb_w = _p(rgb_g), _p(rgb_w)
    d.C_unmasked, d.mask = _p(C_unmasked), _p(mask)
    check(lib.cips_gemm_f32(C.byref(d), _stream()), "cips_gemm_f32")
    return Cm


def bmm_nn(x, w, out=None, **epi):
    """out[b] (M,N) = x[b] (M,K) @ w[b] (K,N); x (B,M,K), w (B,K,N) contiguous."""
    B, M, K = x.shape
    N = w.shape[-1]
    if out is None:
        out = torch.empty(B, M, N, device=x.device)
    gemm(x, w, out, M, N, K, K, N, N, batch=B, strideA=M * K, strideB=K * N, strideC=M * N, **epi)
    return out


def bmm_tn(a, b, out=None):
    """out[b] (Ma,N) = a[b]^T @ b[b]; a (B,K,Ma), b (B,K,N)."""
    B, K, Ma = a.shape
    N = b.shape[-1]
    if out is None:
        out = torch.empty(B, Ma, N, device=a.device)
    gemm(a, b, out, Ma, N, K, Ma, N, N, batch=B, strideA=K * Ma, strideB=K * N, strideC=Ma * N, a_kmajor=True)
    return out


# --------------------------------------------------------------------------------------
# H2 SIREN
# --------------------------------------------------------------------------------------
# the 16 SIREN tensors (FiLM vectors, then weights) in the one order the Functions take them, save them and return their
# gradients; "d" + name are the fields of SirenGrads
_SIREN_NAMES = ("g0", "p0", "g1", "p1", "gc", "pc", "w0", "b0", "w1", "b1", "ws", "bs", "wc", "bc", "wf", "bf")
BOX_SCALE = 2.0 / 0.24   # UniformBoxWarp(0.24), generator.py:249
TRIG_MODE = 1            # 1 hardware v_sin_f32/v_cos_f32 after Cody-Waite reduction (default; measured as accurate
                         # as the polynomial on MI355X: 1.2e-6 vs 1.3e-6), 0 minimax polynomial


def _siren_struct(t):
    s = SirenWeights()
    for n in _SIREN_NAMES:
        setattr(s, n, _p(t[n]))
    s.box_scale = BOX_SCALE
    s.trig_mode = TRIG_MODE
    return s


def _siren_prep(siren):
    """the 16 SIREN tensors in _SIREN_NAMES order -> {name: detached contiguous fp32 tensor}, checked"""
    if len(siren) != len(_SIREN_NAMES):
        raise TypeError(f"expected the {len(_SIREN_NAMES)} SIREN tensors {_SIREN_NAMES}, got {len(siren)}")
    t = {n: _c(v.detach()) for n, v in zip(_SIREN_NAMES, siren)}
    _chk(*t.values())
    return t


def _split_k(P, target=8):
    """Largest split count <= target such that P/split is a multiple of 32."""
    for s in range(target, 0, -1):
        if P % s == 0 and (P // s) % 32 == 0:
            return s
    return 1


# The exact-fp32 mode of the path (the only environment variables the package reads besides
# CIPS_INR_MODE and CIPS_D_CONV_MODE).  Forward "x3": split-operand matrix-core chain (default: fp16 planes, sigma to fp32
# class); "f32": exact fp32 MFMA.  Backward "x3": fused split-bf16 kernel; "staged": fp32 data pass + split-bf16 K-major GEMMs;
# "staged_f32" (round 6): fp32 data pass with fp32-staged activations + fp32-MFMA weight-gradient GEMMs (the all-fp32 leg).
SIREN_FWD_MODE = os.environ.get("CIPS_SIREN_FWD", "x3")
SIREN_BWD_MODE = os.environ.get("CIPS_SIREN_BWD", "x3")
# The fused ray-march's backward (RayMarchFunction, backward "x3") skips the samples whose upstream gradient is exactly zero:
# the compositing backward reports them, a list kernel turns the mask into per-image point lists, and the fused SIREN
# backward walks the lists.  "0": the dense calls.
SIREN_BWD_LIVE = os.environ.get("CIPS_SIREN_BWD_LIVE", "1") != "0"
# ... and deals the live samples evenly to the workgroups of that launch (cips_siren_bwd_x3_live_plan / *_live_even /
# cips_siren_bwd_x3_reduce_segments) instead of giving every image the same number of workgroups.  "0": the *_live calls.
SIREN_BWD_EVEN = os.environ.get("CIPS_SIREN_BWD_EVEN", "1") != "0"
# ... and takes the lists and the EVEN plan from the FORWARD pass: what makes a sample dead under the relu clamp is known once the
# march has written sigma, so a training forward builds both on a stream of their own, beside the INR head, and the backward goes
# from the compositing backward (cips_composite_bwd_listed) straight into the SIREN backward.  Honoured only with the two
# switches above on, backward "x3", no clamp pin and a clamp that has dead samples.  "0": the lists are made in the backward.
SIREN_LIVE_FWD = os.environ.get("CIPS_SIREN_LIVE_FWD", "1") != "0"
# True: with SIREN_LIVE_FWD the finalisation sums the EVEN launch's rows itself (cips_siren_bwd_x3_finalize_segments, same bits)
# instead of reading the per-image sums of cips_siren_bwd_x3_reduce_segments.  Off: at the headline shape the row walk measured
# 91 us against 51 + 18 us for the two launches (profiles/fwd_live_ab.txt).
SIREN_FIN_SEGMENTS = False


class SirenFunction(torch.autograd.Function):
    """feat (B,P,32), sigma (B,P) = siren(points; per-image FiLM vectors, weights: `siren` in _SIREN_NAMES order).

    Mirrors NeRFNetwork.forward_with_frequencies_phase_shifts (generator.py:260-317); gains g*
    are already 15*gain_fc(style)+30 and phases p* = bias_fc(style) (film_layer.py:88-93), both
    computed by tiny torch Linears on the host side so autograd carries them to the mapping net.
    The gradient w.r.t. the points is computed only when they require one (the GAN step's points come from no_grad ray
    math): one extra launch, cips_siren_bwd_points_x3, behind whichever backward form ran.  Once differentiable.
    """

    @staticmethod
    def forward(ctx, points, *siren):
        lib = _lib.load()
        t = _siren_prep(siren)
        points = _c(points.detach())
        _chk(points)
        B, P, _ = points.shape
        feat = torch.empty(B, P, 32, device=points.device)
        sigma = torch.empty(B, P, device=points.device)
        sw = _siren_struct(t)
        fwd = lib.cips_siren_fwd_x3 if SIREN_FWD_MODE == "x3" else lib.cips_siren_fwd
        check(fwd(C.byref(sw), _p(points), _p(feat), _p(sigma), B, P, _stream()), "cips_siren_fwd")
        ctx.save_for_backward(points, *t.values())
        return feat, sigma

    @staticmethod
    @once_differentiable
    def backward(ctx, dfeat, dsigma):
        points = ctx.saved_tensors[0]
        t = dict(zip(_SIREN_NAMES, ctx.saved_tensors[1:]))
        B, P, _ = points.shape
        if not ctx.needs_input_grad[0]:
            return (None,) + _siren_backward(t, dfeat, dsigma, B, P, points=points)
        _need_x3_points_grad()
        dfeat, dsigma = _upstream(dfeat, dsigma, B, P, points.device)
        grads = _siren_backward(t, dfeat, dsigma, B, P, points=points)
        return (siren_bwd_points(t, dfeat, dsigma, B, P, points=points),) + grads


def _siren_sigma_f32(t, points):
    """sigma of the exact-fp32 forward (SIREN_FWD_MODE "f32": there is no sigma-only form of that kernel)"""
    B, P, _ = points.shape
    feat = torch.empty(B, P, 32, device=points.device)
    sigma = torch.empty(B, P, device=points.device)
    sw = _siren_struct(t)
    check(_lib.load().cips_siren_fwd(C.byref(sw), _p(points), _p(feat), _p(sigma), B, P, _stream()), "cips_siren_fwd")
    return sigma


def lattice_points(gx, gy, gz, B):
    """the lattice (gx[i], gy[j], gz[k]) of three 1-D coordinate tensors as points (B, nx * ny * nz, 3), x slowest: what the
    lattice kernels never build, for the paths that have no such kernel.  An expanded view over the batch."""
    n = (gx.numel(), gy.numel(), gz.numel())
    pts = torch.stack([gx.view(-1, 1, 1).expand(n), gy.view(1, -1, 1).expand(n), gz.view(1, 1, -1).expand(n)], -1)
    return pts.reshape(1, -1, 3).expand(B, -1, 3)


def _sigma_prep(points, siren):
    """the inputs of the points forms of the sigma family, detached, contiguous and checked -> t, points, (B, P)"""
    t = _siren_prep(siren)
    points = _c(points.detach())
    _chk(points)
    return t, points, points.shape[:2]


def _sigma_grid_prep(who, gx, gy, gz, siren):
    """... of the lattice forms -> t, (gx, gy, gz), GridParams over them, (B, nx, ny, nz)"""
    t = _siren_prep(siren)
    gx, gy, gz = (_c(v.detach()) for v in (gx, gy, gz))
    _chk(gx, gy, gz)
    if gx.dim() != 1 or gy.dim() != 1 or gz.dim() != 1:
        raise ValueError(f"{who} takes three 1-D coordinate tensors")
    nx, ny, nz = gx.numel(), gy.numel(), gz.numel()
    return t, (gx, gy, gz), GridParams(_p(gx), _p(gy), _p(gz), nx, ny, nz), (t["g0"].shape[0], nx, ny, nz)


def siren_sigma(points, *siren):
    """sigma (B,P) of SirenFunction at points (B,P,3) without the colour branch (cips_siren_sigma_x3: 4 B per point written
    instead of 132, bit for bit the forward kernel's sigma).  A plain function: inputs are detached, no gradient flows.  With
    SIREN_FWD_MODE "f32" the exact-fp32 forward runs and its sigma is returned."""
    t, points, (B, P) = _sigma_prep(points, siren)
    if SIREN_FWD_MODE != "x3":
        return _siren_sigma_f32(t, points)
    sigma = torch.empty(B, P, device=points.device)
    sw = _siren_struct(t)
    check(_lib.load().cips_siren_sigma_x3(C.byref(sw), _p(points), _p(sigma), B, P, _stream()), "cips_siren_sigma_x3")
    return sigma


def siren_sigma_grid(gx, gy, gz, *siren):
    """sigma (B, nx, ny, nz) over the lattice (gx[i], gy[j], gz[k]) of three 1-D coordinate tensors (cips_siren_sigma_x3_grid:
    the kernel reads the coordinates and computes none, no (B,P,3) tensor exists).  Same value as siren_sigma on the
    materialised points, bit for bit.  With SIREN_FWD_MODE "f32" the points are materialised for the exact-fp32 forward."""
    t, (gx, gy, gz), gp, shape = _sigma_grid_prep("siren_sigma_grid", gx, gy, gz, siren)
    if SIREN_FWD_MODE != "x3":
        return _siren_sigma_f32(t, lattice_points(gx, gy, gz, shape[0]).contiguous()).view(shape)
    sigma = torch.empty(shape, device=gx.device)
    sw = _siren_struct(t)
    check(_lib.load().cips_siren_sigma_x3_grid(C.byref(sw), C.byref(gp), _p(sigma), shape[0], _stream()),
          "cips_siren_sigma_x3_grid")
    return sigma


def _need_x3_sigma_grad():
    if SIREN_FWD_MODE != "x3":
        raise RuntimeError(f"the density gradient runs on the split-operand SIREN chain only: there is no exact-fp32 kernel "
                           f"for it (CIPS_SIREN_FWD={SIREN_FWD_MODE!r})")


def siren_sigma_grad(points, *siren):
    """sigma (B,P) and its gradient w.r.t. the points, grad (B,P,3), at points (B,P,3) (cips_siren_sigma_grad_x3).  sigma is
    siren_sigma's bit for bit.  A plain function: inputs are detached, the outputs carry no grad_fn.  With SIREN_FWD_MODE
    other than "x3" it raises: the exact-fp32 forward has no gradient kernel."""
    t, points, (B, P) = _sigma_prep(points, siren)
    _need_x3_sigma_grad()
    sigma = torch.empty(B, P, device=points.device)
    grad = torch.empty(B, P, 3, device=points.device)
    sw = _siren_struct(t)
    check(_lib.load().cips_siren_sigma_grad_x3(C.byref(sw), _p(points), _p(sigma), _p(grad), B, P, _stream()),
          "cips_siren_sigma_grad_x3")
    return sigma, grad


def siren_sigma_grad_grid(gx, gy, gz, *siren):
    """siren_sigma_grad over the lattice (gx[i], gy[j], gz[k]) of three 1-D coordinate tensors -> sigma (B, nx, ny, nz),
    grad (B, nx, ny, nz, 3) (cips_siren_sigma_grad_x3_grid: no points tensor exists).  The points form's values bit for bit."""
    t, (gx, gy, gz), gp, shape = _sigma_grid_prep("siren_sigma_grad_grid", gx, gy, gz, siren)
    _need_x3_sigma_grad()
    sigma = torch.empty(shape, device=gx.device)
    grad = torch.empty(*shape, 3, device=gx.device)
    sw = _siren_struct(t)
    check(_lib.load().cips_siren_sigma_grad_x3_grid(C.byref(sw), C.byref(gp), _p(sigma), _p(grad), shape[0], _stream()),
          "cips_siren_sigma_grad_x3_grid")
    return sigma, grad


def _proj_prep(who, proj_w, proj_b):
    """the 32 -> 3 projection of the colour entry points, detached, contiguous and checked"""
    proj_w, proj_b = _c(proj_w.detach()), _c(proj_b.detach())
    _chk(proj_w, proj_b)
    if tuple(proj_w.shape) != (3, 32) or tuple(proj_b.shape) != (3,):
        raise ValueError(f"{who} takes proj_w (3, 32) and proj_b (3,), got {tuple(proj_w.shape)} and {tuple(proj_b.shape)}")
    return proj_w, proj_b


def _rgb_composed(t, points, proj_w, proj_b, tanh):
    """the colour entry points on the exact-fp32 forward (SIREN_FWD_MODE "f32": that kernel has no colour form): its features
    through an fp32 linear -> rgb (B, P, 3), sigma (B, P)"""
    B, P, _ = points.shape
    feat = torch.empty(B, P, 32, device=points.device)
    sigma = torch.empty(B, P, device=points.device)
    sw = _siren_struct(t)
    check(_lib.load().cips_siren_fwd(C.byref(sw), _p(points), _p(feat), _p(sigma), B, P, _stream()), "cips_siren_fwd")
    y = torch.nn.functional.linear(feat, proj_w, proj_b)
    return (torch.tanh(y) if tanh else y), sigma


@torch.no_grad()
def siren_rgb(points, proj_w, proj_b, *siren, tanh=True, sigma=False):
    """rgb (B,P,3) = [tanh](proj_w . feat + proj_b) of SirenFunction's features at points (B,P,3), projected inside the kernel
    (cips_siren_rgb_x3: 12 B per point written instead of 132, no (B,P,32) tensor and no second launch; the summation order:
    include/cips3d_hip.h); with sigma=True -> (rgb, sigma (B,P)), sigma the forward kernel's bit for bit.  proj_w (3,32),
    proj_b (3): the generator's auxiliary RGB layer, or any 32 -> 3 map.  A plain function: inputs are detached, no gradient
    flows.  With SIREN_FWD_MODE "f32" the exact-fp32 forward runs and its features go through an fp32 linear."""
    t, points, (B, P) = _sigma_prep(points, siren)
    proj_w, proj_b = _proj_prep("siren_rgb", proj_w, proj_b)
    if SIREN_FWD_MODE != "x3":
        rgb, sig = _rgb_composed(t, points, proj_w, proj_b, tanh)
        return (rgb, sig) if sigma else rgb
    rgb = torch.empty(B, P, 3, device=points.device)
    sig = torch.empty(B, P, device=points.device) if sigma else None
    sw = _siren_struct(t)
    check(_lib.load().cips_siren_rgb_x3(C.byref(sw), _p(points), _p(proj_w), _p(proj_b), int(bool(tanh)), _p(rgb), _p(sig), B, P,
                                        _stream()), "cips_siren_rgb_x3")
    return (rgb, sig) if sigma else rgb


@torch.no_grad()
def siren_rgb_grid(gx, gy, gz, proj_w, proj_b, *siren, tanh=True, sigma=False):
    """siren_rgb over the lattice (gx[i], gy[j], gz[k]) of three 1-D coordinate tensors -> rgb (B, nx, ny, nz, 3), with
    sigma=True (rgb, sigma (B, nx, ny, nz)) (cips_siren_rgb_x3_grid: the kernel reads the coordinates, no points tensor exists).
    The points form's values bit for bit.  With SIREN_FWD_MODE "f32" the points are materialised for the exact-fp32 forward."""
    t, (gx, gy, gz), gp, shape = _sigma_grid_prep("siren_rgb_grid", gx, gy, gz, siren)
    proj_w, proj_b = _proj_prep("siren_rgb_grid", proj_w, proj_b)
    if SIREN_FWD_MODE != "x3":
        rgb, sig = _rgb_composed(t, lattice_points(gx, gy, gz, shape[0]).contiguous(), proj_w, proj_b, tanh)
        return (rgb.view(*shape, 3), sig.view(shape)) if sigma else rgb.view(*shape, 3)
    rgb = torch.empty(*shape, 3, device=gx.device)
    sig = torch.empty(shape, device=gx.device) if sigma else None
    sw = _siren_struct(t)
    check(_lib.load().cips_siren_rgb_x3_grid(C.byref(sw), C.byref(gp), _p(proj_w), _p(proj_b), int(bool(tanh)), _p(rgb), _p(sig),
                                             shape[0], _stream()), "cips_siren_rgb_x3_grid")
    return (rgb, sig) if sigma else rgb


def siren_surface(level, refine, geom, xg, yg, zg, cam2world, *siren, trace=False):
    """The iso-surface sigma = level as the camera rays of (geom = (B, H, W, S, zc), pixel grids, cam2world) see it
    (cips_siren_surface_x3: one launch, about S + refine + 1 sigma evaluations per ray at most, no (B, n, S, 3) points and no
    volume) -> depth (B, n) fp32, hit (B, n) uint8 (0 no crossing, 1 crossing, 2 the ray starts inside), sigma (B, n) the
    density at the point of `depth`, points (B, n, 3) = origin + direction * depth; with trace=True also the debug trace
    (B, n, S + refine, 2) of every (t, sigma) a ray's wave evaluated (NaN where it evaluated nothing).  The search rule:
    include/cips3d_hip.h.  A plain function: inputs are detached, no gradient flows.  The rays are the unjittered ones.  With
    SIREN_FWD_MODE other than "x3" it raises (siren_surface_composed is that mode's path)."""
    t = _siren_prep(siren)
    xg, yg, zg, cam2world, _, _ = _ray_prep(xg, yg, zg, cam2world, None, None)
    if SIREN_FWD_MODE != "x3":
        raise RuntimeError(f"the surface ray-cast kernel runs on the split-operand SIREN chain only (CIPS_SIREN_FWD="
                           f"{SIREN_FWD_MODE!r}): use siren_surface_composed")
    B, H, W, S, zc = RayGeom(*geom)
    if not 0 <= int(refine) <= 32:
        raise ValueError("siren_surface: refine must be in 0..32")
    n, dev = H * W, cam2world.device
    depth = torch.empty(B, n, device=dev)
    hit = torch.empty(B, n, dtype=torch.uint8, device=dev)
    sigma = torch.empty(B, n, device=dev)
    points = torch.empty(B, n, 3, device=dev)
    tr = torch.empty(B, n, S + int(refine), 2, device=dev) if trace else None
    sw = _siren_struct(t)
    rp = _ray_params(xg, yg, zg, zc, cam2world, None, H, W, S)
    check(_lib.load().cips_siren_surface_x3(C.byref(sw), C.byref(rp), float(level), int(refine), _p(depth), _p(hit), _p(sigma),
                                            _p(points), _p(tr), B, _stream()), "cips_siren_surface_x3")
    return (depth, hit, sigma, points, tr) if trace else (depth, hit, sigma, points)


def siren_surface_composed(level, refine, geom, xg, yg, zg, cam2world, *siren, sigma_fn=None):
    """siren_surface's search from existing pieces -> depth, hit, sigma, points: the world directions of cips_rays_fwd, one
    sigma launch over all (ray, sample) points of the coarse walk (a (B, n, S, 3) tensor, no early exit), the first crossing by
    tensor operations, then one sigma launch per bisection step and one for the final point.  sigma_fn(points (B, P, 3)) ->
    (B, P) is siren_sigma on `siren` unless given (NeRFNetwork.surface_rays hands in the tensor-operation SIREN of other
    widths).  The path of SIREN_FWD_MODE "f32" and the baseline of scripts/bench_surface.py; the same rule as the kernel, not
    its roundings (the points are origin + direction * t in torch's arithmetic)."""
    B, H, W, S, zc = RayGeom(*geom)
    xg, yg, zg, cam2world, _, _ = _ray_prep(xg, yg, zg, cam2world, None, None)
    if sigma_fn is None:
        def sigma_fn(p):
            return siren_sigma(p, *siren)
    n = H * W
    dirs = rays_fwd(xg, yg, zg, zc, cam2world, None, B, H, W, S)[2]                    # (B, n, 3) world directions
    origin = cam2world[:, None, :3, 3]

    def point(t):                                                                      # t (B, n, k) -> (B, n, k, 3)
        return origin.unsqueeze(2) + dirs.unsqueeze(2) * t.unsqueeze(-1)

    def sig_at(t):                                                                     # t (B, n) -> sigma (B, n)
        return sigma_fn(point(t.unsqueeze(-1)).reshape(B, n, 3))
    sig = sigma_fn(point(zg.view(1, 1, S).expand(B, n, S)).reshape(B, n * S, 3)).view(B, n, S)
    inside = sig[..., 0] >= level
    cross = (sig[..., :-1] < level) & (level <= sig[..., 1:])                          # crossing into step i + 1
    # the walk stops at the first crossing; a crossing needs sigma[i] < level, so nothing crosses before an inside start is seen
    first = cross.to(torch.uint8).argmax(-1)
    hit = torch.where(inside, 2, torch.where(cross.any(-1), 1, 0)).to(torch.uint8)
    one = hit == 1
    lo, hi = zg[first].expand(B, n), zg[first + 1].expand(B, n)
    slo, shi = sig.gather(-1, first.unsqueeze(-1)).squeeze(-1), sig.gather(-1, (first + 1).unsqueeze(-1)).squeeze(-1)
    for _ in range(int(refine)):
        mid = 0.5 * (lo + hi)
        sm = sig_at(mid)
        up = sm >= level
        lo, hi = torch.where(up, lo, mid), torch.where(up, mid, hi)
        slo, shi = torch.where(up, slo, sm), torch.where(up, sm, shi)
    depth = torch.where(one, lo + (level - slo) / (shi - slo) * (hi - lo), torch.where(inside, zg[0], zg[S - 1]).expand(B, n))
    points = point(depth.unsqueeze(-1)).reshape(B, n, 3).contiguous()
    return depth, hit, sigma_fn(points), points


def mesh_from_volume(sigma, gx, gy, gz, level, out=None):
    """Triangle meshes of the level set sigma = level: sigma (B, nx, ny, nz) on the lattice (gx[i], gy[j], gz[k]) of three
    strictly increasing 1-D coordinate tensors -> a list of B pairs (vertices (V_b, 3) fp32, faces (T_b, 3) int32), all on the
    GPU (cips_mesh_count / cips_mesh_emit: marching tetrahedra on the Kuhn decomposition, DESIGN.md section 3 "Meshes").  A
    point is inside iff sigma > level; the triangles' normals (P1 - P0) x (P2 - P0) point towards lower density; faces index
    their own image's vertices.  The pairs are views of two packed tensors; an image without a crossing gets (0, 3) tensors.
    Two calls on the same input give the same bits.

    ONE host synchronisation per call: the read of the per-image totals between the count and the emit launches, which sizes
    the outputs (the check that the coordinates increase rides on the same read).  For that reason the function cannot be
    captured in a hipGraph and raises under capture.  Inputs must be on the GPU, fp32 and contiguous; no gradient flows.
    out: optional (vertices, faces) buffers to fill instead of new tensors, (>= sum V, 3) fp32 and (>= sum T, 3) int32,
    contiguous; rows behind the totals are left untouched."""
    sigma, gx, gy, gz = (t.detach() for t in (sigma, gx, gy, gz))
    _chk(sigma, gx, gy, gz)
    if any(t.dtype != torch.float32 for t in (sigma, gx, gy, gz)):
        raise RuntimeError("mesh_from_volume takes fp32 tensors")
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("mesh_from_volume reads the mesh sizes on the host between its launches: it cannot be captured in a hipGraph")
    if sigma.dim() != 4 or gx.dim() != 1 or gy.dim() != 1 or gz.dim() != 1:
        raise ValueError("mesh_from_volume takes sigma (B, nx, ny, nz) and three 1-D coordinate tensors")
    B, nx, ny, nz = sigma.shape
    if (gx.numel(), gy.numel(), gz.numel()) != (nx, ny, nz):
        raise ValueError(f"coordinate tensors of {gx.numel()}, {gy.numel()}, {gz.numel()} points for a volume {nx} x {ny} x {nz}")
    lib = _lib.load()
    gp = GridParams(_p(gx), _p(gy), _p(gz), nx, ny, nz)
    nbytes = lib.cips_mesh_scratch_bytes(C.byref(gp), B)
    if nbytes < 0:
        raise ValueError(f"mesh_from_volume: a lattice of {nx} x {ny} x {nz} points (B = {B}) is out of range: at least 2 points "
                         "per axis, at most INT_MAX / 7 points and INT_MAX / 12 cells per image")
    dev = sigma.device
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    totals = torch.empty(B, 2, dtype=torch.int64, device=dev)
    level = float(level)
    check(lib.cips_mesh_count(C.byref(gp), _p(sigma), level, B, _p(scratch), nbytes, _p(totals), _stream()), "cips_mesh_count")
    increasing = torch.stack([(g[1:] > g[:-1]).all() for g in (gx, gy, gz)]).all()
    *host, ok = torch.cat([totals.view(-1), increasing.to(torch.int64).view(1)]).tolist()       # the one synchronisation
    if not ok:
        raise ValueError("mesh_from_volume: the coordinate tensors must be strictly increasing")
    V, T = host[0::2], host[1::2]
    if out is None:
        vertices = torch.empty(sum(V), 3, device=dev)
        faces = torch.empty(sum(T), 3, dtype=torch.int32, device=dev)
    else:
        vertices, faces = out
        _chk(vertices, faces)
        if vertices.dtype != torch.float32 or faces.dtype != torch.int32 or vertices.dim() != 2 or faces.dim() != 2 \
                or vertices.shape[1] != 3 or faces.shape[1] != 3 or vertices.shape[0] < sum(V) or faces.shape[0] < sum(T):
            raise ValueError(f"mesh_from_volume: out must be (>= {sum(V)}, 3) fp32 and (>= {sum(T)}, 3) int32")
    if sum(V) > 0 and sum(T) > 0:
        check(lib.cips_mesh_emit(C.byref(gp), _p(sigma), level, B, _p(scratch), nbytes, _p(totals), _p(vertices), _p(faces),
                                 _stream()), "cips_mesh_emit")
    meshes, v0, t0 = [], 0, 0
    for nv, nt in zip(V, T):
        meshes.append((vertices[v0:v0 + nv], faces[t0:t0 + nt]))
        v0 += nv
        t0 += nt
    return meshes


def _need_x3_points_grad():
    if SIREN_FWD_MODE != "x3":
        raise RuntimeError(f"the gradient w.r.t. the sample points / the camera runs on the split-operand SIREN chain only: "
                           f"there is no exact-fp32 kernel for it (CIPS_SIREN_FWD={SIREN_FWD_MODE!r})")


def _upstream(dfeat, dsigma, B, P, dev):
    """the upstream gradients of a SIREN Function as contiguous fp32 tensors (None: zeros)"""
    dfeat = _c(dfeat) if dfeat is not None else torch.zeros(B, P, 32, device=dev)
    dsigma = _c(dsigma) if dsigma is not None else torch.zeros(B, P, device=dev)
    return dfeat, dsigma


def siren_bwd_points(t, dfeat, dsigma, B, P, points=None, rays=None):
    """dpoints (B,P,3): the SIREN's vector-Jacobian product w.r.t. the sample points for the upstream gradients dfeat (B,P,32),
    dsigma (B,P) — the points given (B,P,3) or regenerated in-kernel from `rays` (cips_siren_bwd_points_x3 / _rays).  Dense:
    every row of dfeat / dsigma is read."""
    _need_x3_points_grad()
    _chk(dfeat, dsigma, points)
    dpoints = torch.empty(B, P, 3, device=dfeat.device)
    sw = _siren_struct(t)
    if points is not None:
        check(_lib.load().cips_siren_bwd_points_x3(C.byref(sw), _p(points), _p(dfeat), _p(dsigma), _p(dpoints), B, P, _stream()),
              "cips_siren_bwd_points_x3")
    else:
        check(_lib.load().cips_siren_bwd_points_x3_rays(C.byref(sw), C.byref(rays), _p(dfeat), _p(dsigma), _p(dpoints), B,
                                                        _stream()), "cips_siren_bwd_points_x3_rays")
    return dpoints


def rays_bwd_cam(rays, dpoints, B):
    """per-point gradients (B, H*W*S, 3) of the points `rays` generates -> the gradient of cam2world (B,4,4), row 3 zeros
    (cips_rays_bwd_cam: one launch, fixed summation order)"""
    _chk(dpoints)
    dcam = torch.empty(B, 4, 4, device=dpoints.device)
    check(_lib.load().cips_rays_bwd_cam(C.byref(rays), _p(dpoints), _p(dcam), B, _stream()), "cips_rays_bwd_cam")
    return dcam


def _siren_backward(t, dfeat, dsigma, B, P, points=None, rays=None, live=None):
    """SIREN backward for upstream gradients dfeat (B,P,32), dsigma (B,P) (None: zeros) -> the gradients of the 16 tensors
    in _SIREN_NAMES order.  The sample points are either given (B,P,3) or regenerated in-kernel from `rays` (a RayParams
    struct).  SIREN_BWD_MODE picks the form for given points; `rays` always takes the fused form, whatever the mode says
    (the staged data passes read a points tensor).  `live` (fused form only): (idx (B,P) int32, count (B) int32), the
    points to process per image (cips_siren_bwd_x3_live); the rows of dfeat / dsigma at other points are never read.  A
    `live` of four, (idx, count, seg, img), brings the EVEN plan of those counts along (live_plan_forward)."""
    dev = t["w0"].device
    dfeat = _c(dfeat) if dfeat is not None else torch.zeros(B, P, 32, device=dev)
    dsigma = _c(dsigma) if dsigma is not None else torch.zeros(B, P, device=dev)
    if SIREN_BWD_MODE == "x3" or points is None:
        return _siren_backward_fused(t, dfeat, dsigma, B, P, points, rays, live)
    assert live is None
    return _siren_backward_staged(t, dfeat, dsigma, B, P, points, f32=SIREN_BWD_MODE == "staged_f32")


def live_points(mask):
    """(idx (B,P) int32, count (B) int32) of a (B,P) uint8 mask: idx[b, :count[b]] = the ascending indices of its non-zero
    bytes (cips_live_points; the rest of idx is uninitialised).  No host synchronisation."""
    lib = _lib.load()
    B, P = mask.shape
    idx = torch.empty(B, P, dtype=torch.int32, device=mask.device)
    count = torch.empty(B, dtype=torch.int32, device=mask.device)
    check(lib.cips_live_points(_p(mask), B, P, _p(idx), _p(count), _stream()), "cips_live_points")
    return idx, count


def _live_plan(count, B, P):
    """(seg (B * chunks, 4) int32, img (B, 2) int32): the EVEN partition of lists with these counts (cips_siren_bwd_x3_live_plan)"""
    lib = _lib.load()
    seg = torch.empty(B * lib.cips_siren_bwd_x3_chunks(B, P), 4, dtype=torch.int32, device=count.device)
    img = torch.empty(B, 2, dtype=torch.int32, device=count.device)
    check(lib.cips_siren_bwd_x3_live_plan(_p(count), B, P, _p(seg), _p(img), _stream()), "cips_siren_bwd_x3_live_plan")
    return seg, img


# The stream the forward-time lists and plan run on, one per device: neither the caller's nor the generator's INR-mapping side
# stream, which is joined in front of the head.  live_forward_join makes the caller's stream wait for it.
_LIVE_STREAMS = {}
_LIVE_PENDING = set()


def live_forward_ok(clamp_mode, pin):
    """the forward-time lists apply (see SIREN_LIVE_FWD)"""
    return (SIREN_LIVE_FWD and SIREN_BWD_LIVE and SIREN_BWD_EVEN and SIREN_BWD_MODE == "x3" and pin is None
            and bool(_lib.load().cips_composite_has_dead_samples(clamp_mode)))


def live_plan_forward(sigma, noise, noise_std, B, n, S, clamp_mode, flags):
    """(idx, count, seg, img) of the flat path's samples the compositing backward can give a non-zero gradient
    (cips_live_points_clamp) and their EVEN plan, launched on the device's list stream behind the caller's.  Nothing waits for
    them here: the consumer (RayMarchFunction.backward) does, and live_forward_join() joins the stream for callers that may
    never run it."""
    lib = _lib.load()
    dev = sigma.device
    P = n * S
    idx = torch.empty(B, P, dtype=torch.int32, device=dev)
    count = torch.empty(B, dtype=torch.int32, device=dev)
    side = _LIVE_STREAMS.get(dev.index)
    if side is None:
        side = _LIVE_STREAMS[dev.index] = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        check(lib.cips_live_points_clamp(_p(sigma), _p(noise), float(noise_std), B, n, S, clamp_mode, flags, _p(idx), _p(count),
                                         _stream()), "cips_live_points_clamp")
        seg, img = _live_plan(count, B, P)
    for v in (sigma, noise, idx, count):
        if v is not None:
            v.record_stream(side)
    for v in (seg, img):
        v.record_stream(torch.cuda.current_stream(dev))
    _LIVE_PENDING.add(dev.index)
    return idx, count, seg, img


def live_forward_join(device=None):
    """the caller's stream waits for the forward-time lists of `device` (None: of every device); a no-op when none is pending.
    The generator calls it behind the INR head's forward and on every exit of its forward, so that a captured forward
    without a backward ends with no unjoined stream."""
    for i in [torch.device(device).index] if device is not None else list(_LIVE_PENDING):
        if i in _LIVE_PENDING:
            _LIVE_PENDING.discard(i)
            torch.cuda.current_stream(i).wait_stream(_LIVE_STREAMS[i])


def _siren_backward_fused(t, dfeat, dsigma, B, P, points, rays, live=None):
    """one kernel: recompute + data gradients + weight-gradient contractions on split bf16, nothing staged in HBM"""
    lib = _lib.load()
    dev = dfeat.device
    sw = _siren_struct(t)
    chunks = lib.cips_siren_bwd_x3_chunks(B, P)
    gw = lib.cips_siren_bwd_x3_gpart()
    sw_ = lib.cips_siren_bwd_x3_sred()
    sred = torch.empty(B * chunks, sw_, device=dev)
    gpart = torch.empty(B * chunks, gw, device=dev)
    planned = live is not None and len(live) == 4
    even = planned or (live is not None and SIREN_BWD_EVEN)
    img = None
    if planned:
        idx, count, seg, img = live
    elif even:
        # plan -> kernel -> segmented reduction: the partition follows the counts on the device, nothing is read back
        idx, count = live
        seg, img = _live_plan(count, B, P)
    if even:
        if points is not None:
            check(lib.cips_siren_bwd_x3_live_even(C.byref(sw), _p(points), _p(dfeat), _p(dsigma), _p(idx), _p(count), _p(seg),
                                                  _p(sred), _p(gpart), B, P, _stream()), "cips_siren_bwd_x3_live_even")
        else:
            check(lib.cips_siren_bwd_x3_rays_live_even(C.byref(sw), C.byref(rays), _p(dfeat), _p(dsigma), _p(idx), _p(count),
                                                       _p(seg), _p(sred), _p(gpart), B, _stream()),
                  "cips_siren_bwd_x3_rays_live_even")
    elif live is not None:
        idx, count = live
        if points is not None:
            check(lib.cips_siren_bwd_x3_live(C.byref(sw), _p(points), _p(dfeat), _p(dsigma), _p(idx), _p(count), _p(sred),
                                             _p(gpart), B, P, _stream()), "cips_siren_bwd_x3_live")
        else:
            check(lib.cips_siren_bwd_x3_rays_live(C.byref(sw), C.byref(rays), _p(dfeat), _p(dsigma), _p(idx), _p(count),
                                                  _p(sred), _p(gpart), B, _stream()), "cips_siren_bwd_x3_rays_live")
    elif points is not None:
        check(lib.cips_siren_bwd_x3(C.byref(sw), _p(points), _p(dfeat), _p(dsigma), _p(sred), _p(gpart), B, P,
                                    _stream()), "cips_siren_bwd_x3")
    else:
        check(lib.cips_siren_bwd_x3_rays(C.byref(sw), C.byref(rays), _p(dfeat), _p(dsigma), _p(sred), _p(gpart), B,
                                         _stream()), "cips_siren_bwd_x3_rays")
    # the 16 gradient tensors from the partials in one launch (was ~40 tiny torch reductions)
    outs = tuple(torch.empty_like(t[n]) for n in _SIREN_NAMES)
    sg = SirenGrads()
    for n, v in zip(_SIREN_NAMES, outs):
        setattr(sg, "d" + n, _p(v))
    # the partials are summed per image first (88 MB at C2: bandwidth-bound); the finalisation then walks B rows instead of
    # B * chunks
    if planned and SIREN_FIN_SEGMENTS:
        # ... or the finalisation walks an image's rows itself: no launch and no per-image sums in between
        check(lib.cips_siren_bwd_x3_finalize_segments(C.byref(sw), _p(sred), _p(gpart), _p(img), B, C.byref(sg), _stream()),
              "cips_siren_bwd_x3_finalize_segments")
        return outs
    if even:
        # an image's rows are img[b] = (first, n) here, n from 1 to all of them: one launch sums both arrays
        SRr = torch.empty(B, sw_, device=dev)
        Gpr = torch.empty(B, gw, device=dev)
        check(lib.cips_siren_bwd_x3_reduce_segments(_p(sred), _p(gpart), _p(img), B, _p(SRr), _p(Gpr), _stream()),
              "cips_siren_bwd_x3_reduce_segments")
    else:
        # every image has `chunks` rows: two streaming torch reductions, one launch each
        SRr = sred.view(B, chunks, sw_).sum(1) if chunks > 1 else sred
        Gpr = gpart.view(B, chunks, gw).sum(1) if chunks > 1 else gpart
    check(lib.cips_siren_bwd_x3_finalize(C.byref(sw), _p(SRr), _p(Gpr), B, 1, C.byref(sg), _stream()),
          "cips_siren_bwd_x3_finalize")
    return outs


def _siren_backward_staged(t, dfeat, dsigma, B, P, points, f32):
    """data pass that stages the activations and their gradients in HBM, then the weight-gradient contractions over the
    points as split-K GEMMs.  f32 False ("staged"): rows staged as split-bf16 Planes, contractions on the bf16x3 K-major
    GEMM; f32 True ("staged_f32", the all-fp32 leg): fp32 rows, contractions on the exact-fp32 MFMA GEMM (K-major A)."""
    lib = _lib.load()
    dev = dfeat.device
    sw = _siren_struct(t)
    BP = B * P
    empty = torch.empty if f32 else Planes.empty
    h1, h2, da2 = (empty(BP, 128, device=dev) for _ in range(3))
    hc, dac = (empty(BP, 64, device=dev) for _ in range(2))
    rows = lib.cips_siren_bwd_rows(B, P)
    red = torch.empty(rows, 868, device=dev)
    if f32:
        check(lib.cips_siren_bwd_data_f32(C.byref(sw), _p(points), _p(dfeat), _p(dsigma), _p(h1), _p(h2), _p(hc), _p(da2),
                                          _p(dac), _p(red), B, P, _stream()), "cips_siren_bwd_data_f32")
    else:
        check(lib.cips_siren_bwd_data(C.byref(sw), _p(points), _p(dfeat), _p(dsigma), _p(h1.hi), _p(h1.lo),
                                      _p(h2.hi), _p(h2.lo), _p(hc.hi), _p(hc.lo), _p(da2.hi), _p(da2.lo),
                                      _p(dac.hi), _p(dac.lo), _p(red), B, P, _stream()), "cips_siren_bwd_data")
    R = red.view(B, rows // B, 868).sum(1)          # (B, 868) deterministic reduction of partial rows

    def contract(A, Bm, M, N, batch, rows=BP):
        """(batch, M, N) = A^T @ Bm per chunk of rows / batch rows (split-K): A (rows, M), Bm (rows, N) row-major, i.e. K-major;
        Planes on the bf16x3 K-major GEMM, fp32 tensors on the fp32 GEMM"""
        Kc = rows // batch
        G = torch.empty(batch, M, N, device=dev)
        if isinstance(A, Planes):
            gemm_x3_km(A, Bm, M, N, Kc, M, N, batch, Kc * M, Kc * N, G)
        else:
            gemm(A, Bm, G, M, N, Kc, M, N, N, batch=batch, strideA=Kc * M, strideB=Kc * N, strideC=M * N, a_kmajor=True)
        return G

    sp = _split_k(P, 16)                             # per image: K = P
    if not f32 and (P // sp) % 32:
        # the bf16x3 K-major GEMM takes K in whole 32-row granules: a P off the granule contracts the staged planes on the fp32
        # GEMM (any K), as the dwf line below does at every P
        da2, h1, dac, h2 = da2.float(), h1.float(), dac.float(), h2.float()
    G1 = contract(da2, h1, 128, 128, B * sp).view(B, sp, 128, 128).sum(1)
    Gc = contract(dac, h2, 64, 128, B * sp).view(B, sp, 64, 128).sum(1)
    # the 32x64 colour-linear gradient (no per-image scale) stays on the fp32 GEMM in both modes.  B * P off the 32-row granule:
    # _split_k finds no split there, and all rows in ONE fp32 accumulation chain cost accuracy with its length (2 x 1029 points:
    # 4.4 x the error of a blocked fp32 sum) — the whole granules are split as ever, the last rows (< 32) make one more term.
    # (A count of granules without a divisor <= 1024, a prime one for instance, still leaves _split_k at 1 and one long chain.)
    dfr, hcf, main = dfeat.view(BP, 32), hc if f32 else hc.float(), BP - BP % 32
    dwf = contract(dfr, hcf, 32, 64, _split_k(main, 1024), main).sum(0) if main else 0
    if main < BP:
        dwf = dwf + contract(dfr[main:], hcf[main:], 32, 64, 1, BP - main)[0]
    # ---- assemble parameter / FiLM gradients (tiny tensors) ----
    g0, g1, gc = t["g0"], t["g1"], t["gc"]
    w0, b0, w1, b1, wc, bc = t["w0"], t["b0"], t["w1"], t["b1"], t["wc"], t["bc"]
    d = {}
    d["p0"] = dp0 = R[:, 0:128]
    S0 = R[:, 128:512].view(B, 3, 128).transpose(1, 2) * BOX_SCALE   # (B,128,3): sum_p da1 * x0_c
    d["g0"] = (S0 * w0.unsqueeze(0)).sum(-1) + b0.unsqueeze(0) * dp0
    d["w0"] = (g0.unsqueeze(-1) * S0).sum(0)
    d["b0"] = (g0 * dp0).sum(0)
    d["p1"] = dp1 = R[:, 512:640]
    d["g1"] = (G1 * w1.unsqueeze(0)).sum(-1) + b1.unsqueeze(0) * dp1
    d["w1"] = (g1.unsqueeze(-1) * G1).sum(0)
    d["b1"] = (g1 * dp1).sum(0)
    d["pc"] = dpc = R[:, 640:704]
    d["gc"] = (Gc * wc.unsqueeze(0)).sum(-1) + bc.unsqueeze(0) * dpc
    d["wc"] = (gc.unsqueeze(-1) * Gc).sum(0)
    d["bc"] = (gc * dpc).sum(0)
    d["ws"] = R[:, 704:832].sum(0, keepdim=True)
    d["bf"] = R[:, 832:864].sum(0)
    d["bs"] = R[:, 864].sum().view(1)
    d["wf"] = dwf
    return tuple(d[n] for n in _SIREN_NAMES)


# --------------------------------------------------------------------------------------
# H3 resample / composite
# --------------------------------------------------------------------------------------
def resample_fwd(sigma, z, noise, noise_std, u, origins, dirs, B, n, S, clamp_mode=0, debug=False, cdf_in=None, rays=None):
    """sigma/z/noise/u (B*n,S) -> fine_z (B*n,S), fine_pts (B*n,S,3) [+ weights, cdf, inds].
    rays (RayParams): ray directions / origins recomputed in-kernel, no fine_pts (the fine pass regenerates its points
    from fine_z): origins / dirs may be None, fine_pts is returned as None."""
    lib = _lib.load()
    dev = sigma.device
    sigma, z, noise, u, origins, dirs = _c(sigma), _c(z), _c(noise), _c(u), _c(origins), _c(dirs)
    _chk(sigma, z, noise, u, origins, dirs)
    R = B * n
    fine_z = torch.empty(R, S, device=dev)
    fine_pts = torch.empty(R, S, 3, device=dev) if rays is None else None
    w = cdf = inds = None
    if debug:
        w = torch.empty(R, S, device=dev)
        cdf = torch.empty(R, S - 1, device=dev)
        inds = torch.empty(R, S, device=dev, dtype=torch.int64)
    check(lib.cips_resample_fwd(_p(sigma), _p(z), _p(noise), float(noise_std), _p(u), _p(origins), _p(dirs),
                                _p(fine_z), _p(fine_pts), _p(w), _p(cdf), _p(inds), B, n, S, clamp_mode,
                                _p(_c(cdf_in)) if cdf_in is not None else None,
                                C.byref(rays) if rays is not None else None, _stream()), "cips_resample_fwd")
    if debug:
        return fine_z, fine_pts, w, cdf, inds
    return fine_z, fine_pts


_CLAMP = {"relu": 0, "softplus": 1}


def _geo_upstream(dfea, ddepth, dopacity, like, dev):
    """the upstream gradients of a differentiable-geometry backward as contiguous fp32 tensors: a missing dfea becomes zeros
    shaped `like`, a missing ddepth / dopacity stays None (the kernels take NULL for zeros)"""
    dfea = _c(dfea) if dfea is not None else torch.zeros(like, device=dev)
    ddepth, dopacity = _c(ddepth), _c(dopacity)
    _chk(dfea, ddepth, dopacity)
    return dfea, ddepth, dopacity


def _composite_bwd_call(name, args, ddepth, dopacity):
    """the compositing backward `name` on `args` (everything but the stream) — or, with an upstream gradient of the ray's
    depth or opacity, its `_geo` form, which takes the two behind them"""
    lib = _lib.load()
    if ddepth is None and dopacity is None:
        check(getattr(lib, name)(*args, _stream()), name)
    else:
        check(getattr(lib, name + "_geo")(*args, _p(ddepth), _p(dopacity), _stream()), name + "_geo")


def _composite_forward(ctx, geo, feat_c, sig_c, z_c, feat_f, sig_f, z_f, noise, noise_std, clamp_mode, flags):
    """the forward of CompositeFunction (geo False) and CompositeGeoFunction (True: also the opacity output)
    -> fea, depth, opacity or None, weights, order, zs"""
    lib = _lib.load()
    feat_c, sig_c, z_c = _c(feat_c.detach()), _c(sig_c.detach()), _c(z_c.detach())
    hier = feat_f is not None
    if hier:
        feat_f, sig_f, z_f = _c(feat_f.detach()), _c(sig_f.detach()), _c(z_f.detach())
    noise = _c(noise) if (noise is not None and noise_std != 0.0) else None
    _chk(feat_c, sig_c, z_c, feat_f, sig_f, z_f, noise)
    R, S, _ = feat_c.shape
    E = 2 * S if hier else S
    dev = feat_c.device
    fea = torch.empty(R, 32, device=dev)
    depth = torch.empty(R, device=dev)
    opacity = torch.empty(R, device=dev) if geo else None
    weights = torch.empty(R, E, device=dev)
    order = torch.empty(R, E, device=dev, dtype=torch.int32)
    zs = torch.empty(R, E, device=dev)
    pin, rec = _clamp_debug_forward(R, E, clamp_mode, dev)
    args = (_p(feat_c), _p(sig_c), _p(z_c), _p(feat_f), _p(sig_f), _p(z_f), _p(noise), float(noise_std), _p(fea), _p(depth),
            _p(weights), _p(order), _p(zs), R, S, clamp_mode, flags, _p(pin), _p(rec))
    if geo:
        check(lib.cips_composite_fwd_geo(*args, _p(opacity), _stream()), "cips_composite_fwd_geo")
    else:
        check(lib.cips_composite_fwd(*args, _stream()), "cips_composite_fwd")
    if rec is not None:
        clamp_debug.rec.append(rec.reshape(R, E))
    ctx.clamp_mask = pin                      # pinned branches: the backward takes the same ones (else: its own sign test)
    ctx.save_for_backward(feat_c, sig_c, z_c, feat_f, sig_f, z_f, noise, order)
    ctx.meta = (float(noise_std), clamp_mode, flags, hier)
    return fea, depth, opacity, weights, order, zs


def _composite_backward(ctx, dfea, ddepth=None, dopacity=None):
    """-> dfeat_c, dsig_c, dfeat_f, dsig_f of one compositing forward (cips_composite_bwd, or cips_composite_bwd_geo when the
    depth or the opacity has an upstream gradient too)"""
    feat_c, sig_c, z_c, feat_f, sig_f, z_f, noise, order = ctx.saved_tensors
    noise_std, clamp_mode, flags, hier = ctx.meta
    R, S, _ = feat_c.shape
    dfeat_c = torch.empty_like(feat_c)
    dsig_c = torch.empty_like(sig_c)
    dfeat_f = torch.empty_like(feat_f) if hier else None
    dsig_f = torch.empty_like(sig_f) if hier else None
    _composite_bwd_call("cips_composite_bwd",
                        (_p(feat_c), _p(sig_c), _p(z_c), _p(feat_f), _p(sig_f), _p(z_f), _p(noise), noise_std, _p(order),
                         _p(dfea), _p(dfeat_c), _p(dsig_c), _p(dfeat_f), _p(dsig_f), R, S, clamp_mode, flags,
                         _p(ctx.clamp_mask)), ddepth, dopacity)
    _tail_gate_publish(dfea.device)
    return dfeat_c, dsig_c, dfeat_f, dsig_f


class CompositeFunction(torch.autograd.Function):
    """Merge (optional) + alpha-composite; see cips_composite_fwd / _bwd.
    Inputs are flattened over rays: feat (R,S,32), sig (R,S), z (R,S); fine set may be None."""

    @staticmethod
    def forward(ctx, feat_c, sig_c, z_c, feat_f, sig_f, z_f, noise, noise_std, clamp_mode, flags):
        fea, depth, _, weights, order, zs = _composite_forward(ctx, False, feat_c, sig_c, z_c, feat_f, sig_f, z_f, noise,
                                                               noise_std, clamp_mode, flags)
        ctx.mark_non_differentiable(depth, weights, order, zs)
        return fea, depth, weights, order, zs

    @staticmethod
    def backward(ctx, dfea, *unused):
        dfeat_c, dsig_c, dfeat_f, dsig_f = _composite_backward(ctx, _c(dfea))
        return dfeat_c, dsig_c, None, dfeat_f, dsig_f, None, None, None, None, None


class CompositeGeoFunction(torch.autograd.Function):
    """CompositeFunction with the geometry differentiable: -> fea (R,32), depth (R), opacity (R), weights, order, zs, the first
    three with gradients.  depth = sum_k w_k z_k (+ (1 - sum w) z_last under last_back), opacity = sum_k w_k before the last_back
    top-up (the reference's weights_sum, pigan_utils.py:261); both are linear in the weights like the features, and their
    upstream gradients enter the same reverse scan (cips_composite_bwd_geo).  The depths z stay constants, as in the
    reference; `weights` is not a differentiable output.  An upstream of the features alone takes CompositeFunction's call.
    Once differentiable."""

    @staticmethod
    def forward(ctx, feat_c, sig_c, z_c, feat_f, sig_f, z_f, noise, noise_std, clamp_mode, flags):
        fea, depth, opacity, weights, order, zs = _composite_forward(ctx, True, feat_c, sig_c, z_c, feat_f, sig_f, z_f, noise,
                                                                     noise_std, clamp_mode, flags)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(weights, order, zs)
        return fea, depth, opacity, weights, order, zs

    @staticmethod
    @once_differentiable
    def backward(ctx, dfea, ddepth, dopacity, *unused):
        if dfea is None and ddepth is None and dopacity is None:
            return (None,) * 10
        feat_c = ctx.saved_tensors[0]
        dfea, ddepth, dopacity = _geo_upstream(dfea, ddepth, dopacity, (feat_c.shape[0], 32), feat_c.device)
        dfeat_c, dsig_c, dfeat_f, dsig_f = _composite_backward(ctx, dfea, ddepth, dopacity)
        return dfeat_c, dsig_c, None, dfeat_f, dsig_f, None, None, None, None, None


# --------------------------------------------------------------------------------------
# Grouped small Linear layers (style -> per-image vectors), one launch for all of them
# --------------------------------------------------------------------------------------


class GroupedLinearFunction(torch.autograd.Function):
    """ys = [x @ W_j^T + b_j for j] for Linear layers that share their input x (B, in): the SinStyleMod.modulation
    layers of the CIPS head (mod_conv_fc.py:433-436, 474) or the gain_fc / bias_fc of the FiLM layers
    (film_layer.py:59-63, 88-93).  forward(x, W_0, b_0, W_1, b_1, ...) -> tuple of (B, out_j)."""

    @staticmethod
    def forward(ctx, x, *wb):
        lib = _lib.load()
        x = _c(x.detach())
        ws = [_c(w.detach()) for w in wb[0::2]]
        bs = [_c(b.detach()) if b is not None else None for b in wb[1::2]]
        _chk(x, *ws, *[b for b in bs if b is not None])
        B, in_dim = x.shape
        n = len(ws)
        if n > lib.cips_grouped_linear_max_jobs() or in_dim % 4 or in_dim > 512:
            raise RuntimeError("grouped linear: at most 32 jobs, in_dim a multiple of 4 and <= 512")
        jobs = (GlinJob * n)()
        ys = []
        for j, (w, b) in zip(jobs, zip(ws, bs)):
            y = torch.empty(B, w.shape[0], device=x.device)
            j.x, j.w, j.bias, j.y = _p(x), _p(w), _p(b), _p(y)
            j.in_dim, j.out_dim = in_dim, w.shape[0]
            ys.append(y)
        check(lib.cips_grouped_linear_fwd(jobs, n, B, _stream()), "cips_grouped_linear_fwd")
        ctx.save_for_backward(x, *ws)
        ctx.has_bias = [b is not None for b in bs]
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        lib = _lib.load()
        x, *ws = ctx.saved_tensors
        B, in_dim = x.shape
        n = len(ws)
        jobs = (GlinJob * n)()
        dws, dbs, keep = [], [], []
        for j, w, dy, hb in zip(jobs, ws, dys, ctx.has_bias):
            dy = _c(dy) if dy is not None else torch.zeros(B, w.shape[0], device=x.device)
            keep.append(dy)
            dw = torch.empty_like(w)
            db = torch.empty(w.shape[0], device=x.device) if hb else None
            j.x, j.w, j.dy, j.dw, j.db = _p(x), _p(w), _p(dy), _p(dw), _p(db)
            j.in_dim, j.out_dim = in_dim, w.shape[0]
            dws.append(dw); dbs.append(db)
        dx = scratch = None
        nscr = 0
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            nscr = lib.cips_grouped_linear_scratch(jobs, n, B)
            scratch = torch.empty(nscr, device=x.device)
        check(lib.cips_grouped_linear_bwd(jobs, n, B, _p(dx), _p(scratch), nscr, _stream()), "cips_grouped_linear_bwd")
        out = [dx]
        for dw, db in zip(dws, dbs):
            out += [dw, db]
        return tuple(out)


def grouped_linear(pairs):
    """pairs: list of (x (B,in), nn.Linear) -> list of Linear(x).  Layers whose inputs are the SAME tensor go into one
    grouped launch (the reference's style dicts alias one tensor per mapping network, multi_head_mapping.py:147-153);
    anything else (truncated / mixed styles) falls back to one launch per distinct input."""
    out = [None] * len(pairs)
    groups = {}
    for idx, (x, lin) in enumerate(pairs):
        groups.setdefault(id(x), []).append(idx)
    mx = 32
    for idxs in groups.values():
        x = pairs[idxs[0]][0]
        if x.dim() != 2 or x.shape[1] % 4 or x.shape[1] > 512 or x.shape[0] > 256 or not x.is_cuda:
            for i in idxs:
                out[i] = pairs[i][1](pairs[i][0])
            continue
        for c0 in range(0, len(idxs), mx):
            chunk = idxs[c0:c0 + mx]
            args = []
            for i in chunk:
                lin = pairs[i][1]
                args += [lin.weight, lin.bias]
            ys = GroupedLinearFunction.apply(x, *args)
            for i, y in zip(chunk, ys):
                out[i] = y
    return out


# --------------------------------------------------------------------------------------
# Row-wise normalisation + activation of the mapping MLPs
# --------------------------------------------------------------------------------------
class RowNormFunction(torch.autograd.Function):
    """y = act(norm(x)) per batch row (cips_rownorm_fwd / _bwd): mode bit 0 LayerNorm(gamma, beta; eps 1e-5), bit 1
    LeakyReLU(0.2) after it, bit 2 PixelNorm (multi_head_mapping.py:13-19, :62-84)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mode):
        lib = _lib.load()
        x = _c(x.detach())
        gamma = _c(gamma.detach()) if gamma is not None else None
        beta = _c(beta.detach()) if beta is not None else None
        _chk(x, gamma, beta)
        rows, cols = x.shape
        y = torch.empty_like(x)
        stats = torch.empty(rows, 2, device=x.device)
        check(lib.cips_rownorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), _p(stats), rows, cols, mode, LRELU_SLOPE, _stream()),
              "cips_rownorm_fwd")
        ctx.save_for_backward(x, y, gamma, stats)
        ctx.mode = mode
        return y

    @staticmethod
    def backward(ctx, dy):
        lib = _lib.load()
        x, y, gamma, stats = ctx.saved_tensors
        rows, cols = x.shape
        dy = _c(dy)
        dx = torch.empty_like(x)
        ln = bool(ctx.mode & 1)
        dyhat = torch.empty_like(x) if ln else None
        dgamma = torch.empty(cols, device=x.device) if ln else None
        dbeta = torch.empty(cols, device=x.device) if ln else None
        check(lib.cips_rownorm_bwd(_p(x), _p(y), _p(gamma), _p(stats), _p(dy), _p(dx), _p(dyhat), _p(dgamma), _p(dbeta), rows,
                                   cols, ctx.mode, LRELU_SLOPE, _stream()), "cips_rownorm_bwd")
        return dx, dgamma, dbeta, None


# --------------------------------------------------------------------------------------
# Fused ray-march (non-hierarchical sampling): rays + SIREN + composite in one kernel
# --------------------------------------------------------------------------------------
MARCH_FUSED = True      # False: flat sampling as rays / SIREN / composite launches (what the hierarchical path uses); the
                        # parity test of the fused kernel against that path flips it


def march_available():
    """the fused march runs on the split-bf16 register chain (forward) and regenerates points in the fused backward"""
    return MARCH_FUSED and SIREN_FWD_MODE == "x3" and SIREN_BWD_MODE == "x3"


def _ray_params(xg, yg, zg, zc, cam2world, jitter, H, W, S, zvals=None):
    r = RayParams()
    r.xg, r.yg, r.zg, r.cam2world, r.jitter, r.zvals = _p(xg), _p(yg), _p(zg), _p(cam2world), _p(jitter), _p(zvals)
    r.zc, r.H, r.W, r.S = float(zc), H, W, S
    return r


def _ray_prep(xg, yg, zg, cam2world, jitter, per_sample):
    """the ray inputs of SirenRaysFunction / RayMarchFunction as detached contiguous fp32 tensors, checked: pixel grids,
    cam2world, the optional jitter draw and the Function's optional per-sample tensor (`zvals` / `noise`)"""
    r = [_c(v.detach()) if v is not None else None for v in (xg, yg, zg, cam2world, jitter, per_sample)]
    _chk(*r)
    return r


class SirenRaysFunction(torch.autograd.Function):
    """feat (B,P,32), sigma (B,P), z (B,P) = siren(points generated in-kernel) — SirenFunction without the (B,P,3)
    points tensor, for the two passes of the hierarchical path: the coarse pass generates its stratified samples from
    (grids, cam2world, jitter) (comm_utils.py:365-438, 584-679), the fine pass from the resampled depths
    `zvals`: origin + direction * z (generator_nerf_inr.py:590-592).  Backward: cips_siren_bwd_x3_rays; when cam2world requires a
    gradient also the per-point gradients (cips_siren_bwd_points_x3_rays) and their reduction to the matrix (cips_rays_bwd_cam).
    Grids, jitter and zvals get none.  Once differentiable."""

    @staticmethod
    def forward(ctx, geom, xg, yg, zg, cam2world, jitter, zvals, *siren):
        lib = _lib.load()
        B, H, W, S, zc = geom = RayGeom(*geom)
        t = _siren_prep(siren)
        xg, yg, zg, cam2world, jitter, zvals = _ray_prep(xg, yg, zg, cam2world, jitter, zvals)
        dev = cam2world.device
        P = H * W * S
        feat = torch.empty(B, P, 32, device=dev)
        sigma = torch.empty(B, P, device=dev)
        z = torch.empty(B, P, device=dev) if zvals is None else zvals
        sw = _siren_struct(t)
        rp = _ray_params(xg, yg, zg, zc, cam2world, jitter, H, W, S, zvals)
        check(lib.cips_siren_fwd_x3_rays(C.byref(sw), C.byref(rp), _p(feat), _p(sigma), _p(z) if zvals is None else None, B,
                                         _stream()), "cips_siren_fwd_x3_rays")
        ctx.save_for_backward(xg, yg, zg, cam2world, jitter, zvals, *t.values())
        ctx.geom = geom
        ctx.mark_non_differentiable(z)
        return feat, sigma, z

    @staticmethod
    @once_differentiable
    def backward(ctx, dfeat, dsigma, _dz):
        xg, yg, zg, cam2world, jitter, zvals = ctx.saved_tensors[:6]
        t = dict(zip(_SIREN_NAMES, ctx.saved_tensors[6:]))
        B, H, W, S, zc = ctx.geom
        rp = _ray_params(xg, yg, zg, zc, cam2world, jitter, H, W, S, zvals)
        if not ctx.needs_input_grad[4]:
            return (None,) * 7 + _siren_backward(t, dfeat, dsigma, B, H * W * S, rays=rp)
        _need_x3_points_grad()
        dfeat, dsigma = _upstream(dfeat, dsigma, B, H * W * S, cam2world.device)
        grads = _siren_backward(t, dfeat, dsigma, B, H * W * S, rays=rp)
        dcam = rays_bwd_cam(rp, siren_bwd_points(t, dfeat, dsigma, B, H * W * S, rays=rp), B)
        return (None,) * 4 + (dcam,) + (None,) * 2 + grads


class RayMarchFunction(torch.autograd.Function):
    """pixels_fea (B,n,32), depth (B,n) = composite(SIREN(points(rays, jitter))) for hierarchical_sample=False: the
    chain get_initial_rays_trig / perturb_points / transform_sampled_points (comm_utils.py:365-438, 584-679) ->
    NeRFNetwork (generator.py:260-317) -> fancy_integration (pigan_utils.py:212-273) as ONE kernel that walks the
    samples along each ray (cips_march_fwd_x3).  Under no_grad nothing per-sample reaches HBM (4 S + 132 B per ray);
    a training forward also writes feat / sigma / z for the backward, which is cips_composite_bwd followed by the fused
    SIREN backward with the points regenerated in-kernel (cips_siren_bwd_x3_rays) — with SIREN_BWD_LIVE their *_live forms
    and cips_live_points between them: the SIREN backward then runs over the samples with a non-zero upstream gradient.
    With SIREN_LIVE_FWD, for a caller that says so in geom and joins the list stream behind its next stage, the training
    forward makes those lists and their EVEN plan itself, on another stream (live_plan_forward), and the backward is
    cips_composite_bwd_listed followed by the SIREN backward.
    When cam2world requires a gradient the backward also runs the dense per-point kernel (cips_siren_bwd_points_x3_rays) and its
    reduction (cips_rays_bwd_cam); the live forms of the compositing backward leave the rows of dead samples unwritten, so the
    buffers are then allocated zero-filled — a dead sample's gradient is exactly zero.  Once differentiable."""

    @staticmethod
    def forward(ctx, geom, xg, yg, zg, cam2world, jitter, noise, *siren):
        fea, depth, _ = _march_forward(ctx, False, geom, xg, yg, zg, cam2world, jitter, noise, *siren)
        ctx.mark_non_differentiable(depth)
        return fea, depth

    @staticmethod
    @once_differentiable
    def backward(ctx, dfea, _ddepth):
        return _march_backward(ctx, _c(dfea))


class RayMarchGeoFunction(torch.autograd.Function):
    """RayMarchFunction with the geometry differentiable: -> pixels_fea (B,n,32), depth (B,n), opacity (B,n), all three with
    gradients (cips_march_fwd_x3_geo; depth and opacity as CompositeGeoFunction defines them).  The backward takes every route
    RayMarchFunction's takes — dense, masked, the forward-time lists, and the camera's — with the `_geo` form of the route's
    compositing backward when the depth or the opacity has an upstream gradient (only dsigma changes; the liveness rules hold
    whatever the upstream is: a relu-clamped sample has alpha = 0 and d alpha / dx = 0), and exactly RayMarchFunction's calls
    when only the features have one.  Once differentiable; no host synchronisation."""

    @staticmethod
    def forward(ctx, geom, xg, yg, zg, cam2world, jitter, noise, *siren):
        ctx.set_materialize_grads(False)
        return _march_forward(ctx, True, geom, xg, yg, zg, cam2world, jitter, noise, *siren)

    @staticmethod
    @once_differentiable
    def backward(ctx, dfea, ddepth, dopacity):
        if dfea is None and ddepth is None and dopacity is None:
            return (None,) * (7 + len(_SIREN_NAMES))
        feat = ctx.saved_tensors[6]
        g = ctx.geom
        return _march_backward(ctx, *_geo_upstream(dfea, ddepth, dopacity, (g.B, g.H * g.W, 32), feat.device))


def _march_forward(ctx, geo, geom, xg, yg, zg, cam2world, jitter, noise, *siren):
    """the forward of RayMarchFunction (geo False) and RayMarchGeoFunction (True: also the opacity output)
    -> fea, depth, opacity or None"""
    lib = _lib.load()
    B, H, W, S, zc, noise_std, clamp_mode, flags, grad_mode, live_fwd = geom = MarchGeom(*geom)
    t = _siren_prep(siren)
    xg, yg, zg, cam2world, jitter, noise = _ray_prep(xg, yg, zg, cam2world, jitter, noise if noise_std != 0.0 else None)
    dev = cam2world.device
    n = H * W
    # per-sample outputs only when a backward can follow: the caller's grad mode counts (inside forward() it is
    # always off, and under torch.no_grad() needs_input_grad still reports the parameters' requires_grad)
    train = grad_mode and any(ctx.needs_input_grad)
    fea = torch.empty(B, n, 32, device=dev)
    depth = torch.empty(B, n, device=dev)
    opacity = torch.empty(B, n, device=dev) if geo else None
    feat = torch.empty(B, n * S, 32, device=dev) if train else None
    sigma = torch.empty(B, n * S, device=dev) if train else None
    z = torch.empty(B, n * S, device=dev) if train else None
    sw = _siren_struct(t)
    rp = _ray_params(xg, yg, zg, zc, cam2world, jitter, H, W, S)
    pin, rec = _clamp_debug_forward(B * n, S, clamp_mode, dev)
    args = (C.byref(sw), C.byref(rp), _p(noise), float(noise_std), clamp_mode, flags, _p(fea), _p(depth), None, _p(feat),
            _p(sigma), _p(z), B, _p(pin), _p(rec))
    if geo:
        check(lib.cips_march_fwd_x3_geo(*args, _p(opacity), _stream()), "cips_march_fwd_x3_geo")
    else:
        check(lib.cips_march_fwd_x3(*args, _stream()), "cips_march_fwd_x3")
    if rec is not None:
        clamp_debug.rec.append(rec.reshape(B * n, S))
    ctx.clamp_mask = pin
    ctx.live_fwd = train and bool(live_fwd) and live_forward_ok(clamp_mode, pin)
    if train:
        lists = live_plan_forward(sigma, noise, noise_std, B, n, S, clamp_mode, flags) if ctx.live_fwd else ()
        ctx.save_for_backward(xg, yg, zg, cam2world, jitter, noise, feat, sigma, z, *t.values(), *lists)
    ctx.geom = geom
    return fea, depth, opacity


def _march_backward(ctx, dfea, ddepth=None, dopacity=None):
    """the backward of one march forward for the upstream gradient dfea (B,n,32) and, optionally, those of depth / opacity (B,n)
    -> the gradients of the Functions' inputs (geom, xg, yg, zg, cam2world, jitter, noise, *siren)"""
    xg, yg, zg, cam2world, jitter, noise, feat, sigma, z = ctx.saved_tensors[:9]
    t = dict(zip(_SIREN_NAMES, ctx.saved_tensors[9:9 + len(_SIREN_NAMES)]))
    B, H, W, S, zc, noise_std, clamp_mode, flags, _, _ = ctx.geom
    n = H * W
    R = B * n
    want_cam = ctx.needs_input_grad[4]
    if want_cam:
        _need_x3_points_grad()
    # the camera gradient's kernel reads every row, the live forms below write only the live ones
    dfeat = torch.zeros_like(feat) if want_cam else torch.empty_like(feat)
    dsig = torch.zeros_like(sigma) if want_cam else torch.empty_like(sigma)
    use_live = SIREN_BWD_LIVE and SIREN_BWD_MODE == "x3"
    live = None
    if ctx.live_fwd:
        live = ctx.saved_tensors[9 + len(_SIREN_NAMES):]
        # the lists' stream, whether or not a live_forward_join has made some stream wait for it already
        _LIVE_PENDING.discard(dfea.device.index)
        torch.cuda.current_stream(dfea.device).wait_stream(_LIVE_STREAMS[dfea.device.index])
        _composite_bwd_call("cips_composite_bwd_listed",
                            (_p(feat), _p(sigma), _p(z), _p(noise), float(noise_std), _p(dfea), _p(dfeat), _p(dsig), R, S,
                             clamp_mode, flags), ddepth, dopacity)
    elif use_live:
        mask = torch.empty(B, n * S, dtype=torch.uint8, device=dfea.device)
        _composite_bwd_call("cips_composite_bwd_live",
                            (_p(feat), _p(sigma), _p(z), None, None, None, _p(noise), float(noise_std), None, _p(dfea),
                             _p(dfeat), _p(dsig), None, None, _p(mask), None, R, S, clamp_mode, flags, _p(ctx.clamp_mask)),
                            ddepth, dopacity)
    else:
        _composite_bwd_call("cips_composite_bwd",
                            (_p(feat), _p(sigma), _p(z), None, None, None, _p(noise), float(noise_std), None, _p(dfea),
                             _p(dfeat), _p(dsig), None, None, R, S, clamp_mode, flags, _p(ctx.clamp_mask)), ddepth, dopacity)
    _tail_gate_publish(dfea.device)
    rp = _ray_params(xg, yg, zg, zc, cam2world, jitter, H, W, S)
    if live is None and use_live:
        live = live_points(mask)
    grads = _siren_backward(t, dfeat, dsig, B, n * S, rays=rp, live=live)
    if not want_cam:
        return (None,) * 7 + grads
    dcam = rays_bwd_cam(rp, siren_bwd_points(t, dfeat, dsig, B, n * S, rays=rp), B)
    return (None,) * 4 + (dcam,) + (None,) * 2 + grads


# --------------------------------------------------------------------------------------
# H4 CIPS INR head (all blocks of CIPSNet.forward in one autograd node)
# --------------------------------------------------------------------------------------
def modfc_prep(W, s, eps=1e-8):
    lib = _lib.load()
    in_dim, out_dim = W.shape
    B = s.shape[0]
    dev = W.device
    wb = torch.empty(B, in_dim, out_dim, device=dev)
    wbt = torch.empty(B, out_dim, in_dim, device=dev)
    demod = torch.empty(B, out_dim, device=dev)
    check(lib.cips_modfc_prep(_p(W), _p(s), _p(wb), _p(wbt), _p(demod), B, in_dim, out_dim, eps, _stream()),
          "cips_modfc_prep")
    return wb, wbt, demod


def modfc_prep_bwd(W, s, demod, gwb):
    lib = _lib.load()
    in_dim, out_dim = W.shape
    B = s.shape[0]
    dev = W.device
    cbuf = torch.empty(B, out_dim, device=dev)
    dW = torch.empty(in_dim, out_dim, device=dev)
    ds = torch.empty(B, in_dim, device=dev)
    check(lib.cips_modfc_prep_bwd(_p(W), _p(s), _p(demod), _p(gwb), _p(cbuf), _p(dW), _p(ds), B, in_dim, out_dim,
                                  _stream()), "cips_modfc_prep_bwd")
    return dW, ds


def torgb_fwd(x2d, w, b, rgb2d, accumulate):
    lib = _lib.load()
    M, K = x2d.shape
    check(lib.cips_torgb_fwd(_p(x2d), _p(w), _p(b), _p(rgb2d), M, K, 1 if accumulate else 0, _stream()),
          "cips_torgb_fwd")


def torgb_bwd_w(x2d, drgb2d):
    lib = _lib.load()
    M, K = x2d.shape
    chunks = lib.cips_torgb_bwd_partials(M)
    part = torch.empty(chunks, 4, K, device=x2d.device)
    dw = torch.empty(3, K, device=x2d.device)
    db = torch.empty(3, device=x2d.device)
    check(lib.cips_torgb_bwd_w(_p(x2d), _p(drgb2d), _p(part), _p(dw), _p(db), M, K, _stream()), "cips_torgb_bwd_w")
    return dw, db


def torgb_bwd_x_x3(drgb2d, w, gate_bits, out_unmasked, P):
    """P (Planes (.., K)) = (drgb2d (M,3) @ w (3,K)) * (gate bit ? 1 : slope); out_unmasked: optional fp32 copy before gating"""
    lib = _lib.load()
    M, K = drgb2d.shape[0], w.shape[1]
    check(lib.cips_torgb_bwd_x_x3(_p(drgb2d), _p(_c(w)), _p(gate_bits), LRELU_SLOPE, _p(out_unmasked), _p(P.hi), _p(P.lo), M, K,
                                  _stream()), "cips_torgb_bwd_x_x3")


def torgb_bwd_x(drgb2d, w, add, mask, out_unmasked, out):
    lib = _lib.load()
    M = drgb2d.shape[0]
    K = w.shape[1]
    check(lib.cips_torgb_bwd_x(_p(drgb2d), _p(w), _p(add), _p(mask), LRELU_SLOPE, _p(out_unmasked), _p(out), M, K,
                               _stream()), "cips_torgb_bwd_x")


# ---- instrumentation of the path's discontinuities (parity tests; never set in production) -----------------------
class DebugHook:
    """A pin / record hook: `pin` is an iterator the instrumented op draws its decisions from in call order instead of taking
    them itself (None: not pinned), `rec` a list that receives the decisions it took (None: not recorded).
    `with hook(pin=[...] or None, rec=list or None): ...` sets both and restores the outer values on exit, so uses nest.
    leftover: the message of the assertion that every pin was drawn when the block ends without an exception (None: not
    asserted)."""

    def __init__(self, leftover=None):
        self.pin, self.rec, self.leftover = None, None, leftover

    @property
    def active(self):
        return self.pin is not None or self.rec is not None

    @contextlib.contextmanager
    def __call__(self, pin=None, rec=None):
        old = (self.pin, self.rec)
        self.pin, self.rec = (iter(pin) if pin is not None else None), rec
        try:
            yield self
            if self.leftover is not None and self.pin is not None:
                assert next(self.pin, None) is None, self.leftover
        finally:
            self.pin, self.rec = old


# A LeakyReLU gate (pre-activation > 0) is the one discontinuity of the head: two fp32 evaluations of the same layer
# may disagree on it for pre-activations within rounding of zero, and each disagreement moves the gradients by a
# finite amount.  Gradient parity is therefore stated for a GIVEN set of gates:
#   pin: uint8 bit planes (B, n, C/8) (bit c&7 of byte c>>3 = gate of column c), one per modulated-FC layer in call
#        order; the forward epilogues then apply `gate ? 1 : slope` from the plane instead of deciding by the sign
#        they computed, and the backward uses the same plane.
#   rec: receives the bit plane every layer actually used, in call order.
gate_debug = DebugHook(leftover="pinned gate planes left over")
# The other discontinuity of the path: importance resampling places the fine samples by a searchsorted over the coarse
# weights' cdf (pigan_utils.py:164-273); a cdf value within rounding of the uniform draw puts a sample in the
# neighbouring bin.  rec collects the depths every hierarchical forward resampled (b*n, S); pin (such tensors)
# replaces them — parity tests compare gradients for the SAME sample placement.
resample_debug = DebugHook()
# The third discontinuity: relu(sigma + nerf_noise * eps) in fancy_integration (pigan_utils.py:246-252).  The reference trains
# its first 5 000 steps with nerf_noise 1 -> 0 (train.py:325-327); a pre-activation within rounding of 0 takes either
# branch, and the two gradients of the sigma head (sums of d sigma with heavy cancellation) move by a finite amount per
# flipped sample.  pin: uint8 tensors (R, E) (R rays, E sorted positions; 0 = clamped, else the linear branch), one per
# composite / fused-march forward in call order — forward AND backward then take the branch from it.  rec: receives the
# branches each forward actually took.
clamp_debug = DebugHook()


def _clamp_debug_forward(R, E, clamp_mode, dev):
    """-> (pin, rec) for one composite forward of R rays x E positions: both None outside clamp_debug / for softplus"""
    if not clamp_debug.active or clamp_mode != 0:
        return None, None
    pin = None
    if clamp_debug.pin is not None:
        pin = next(clamp_debug.pin).to(device=dev, dtype=torch.uint8).reshape(-1).contiguous()
        if pin.numel() != R * E:
            raise ValueError(f"clamp_debug: pinned mask of {pin.numel()} entries for {R} rays x {E} positions")
    return pin, (torch.empty(R * E, dtype=torch.uint8, device=dev) if clamp_debug.rec is not None else None)


def fine_z_debug(fine_z):
    """-> the depths one hierarchical forward is to use: `fine_z` itself (recorded under resample_debug(rec=...)), or the next
    pinned tensor in its shape — a different object, so a caller that materialised points from `fine_z` can tell"""
    if resample_debug.rec is not None:
        resample_debug.rec.append(fine_z.detach().clone())
    if resample_debug.pin is None:
        return fine_z
    return next(resample_debug.pin).to(fine_z.device).reshape(fine_z.shape).contiguous()


def _next_pin(B, n, C, dev):
    if gate_debug.pin is None:
        return None
    p = next(gate_debug.pin)
    assert p.dtype == torch.uint8 and tuple(p.shape) == (B, n, C // 8), (tuple(p.shape), (B, n, C // 8))
    return p.to(dev).contiguous()


def _bits_to_pm1(p):
    """uint8 bit plane (..., C/8) -> fp32 (..., C) of +1 / -1 (the fp32 GEMM's `mask` operand reads the sign)"""
    sh = torch.arange(8, device=p.device)
    g = ((p.unsqueeze(-1).to(torch.int32) >> sh) & 1).reshape(*p.shape[:-1], p.shape[-1] * 8)
    return (g * 2 - 1).float()


def _sign_to_bits(a):
    """fp32 (..., C) -> uint8 bit plane (..., C/8) of a > 0"""
    w = (1 << torch.arange(8, device=a.device)).to(torch.int32)
    return ((a > 0).reshape(*a.shape[:-1], a.shape[-1] // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def _head_params(nblocks, params):
    """the head's parameter layout: (W1, s1, W2, s2) per block, then (T, tau) of the ToRGB tap of every block k >= 3 — what
    follows them are the handles of gradient ports -> blocks (list of 4-tuples), rgbp (flat list), detached and contiguous"""
    blocks = [tuple(_c(p.detach()) for p in params[4 * k:4 * k + 4]) for k in range(nblocks)]
    rgbp = [_c(p.detach()) for p in params[4 * nblocks:4 * nblocks + 2 * max(nblocks - 3, 0)]]
    return blocks, rgbp


def _head_grads(dx0, grads_blocks, grads_rgb):
    """the head's gradients in autograd order: (nblocks, grad_mode, ports, x0), then the layout of _head_params"""
    return (None, None, None, dx0) + tuple(g for gb in grads_blocks for g in gb) + tuple(grads_rgb)


class InrHeadFunction(torch.autograd.Function):
    """rgb_pre (B,n,3) = CIPSNet body (generator.py:1107-1153, before the final tanh).

    args: x0 (B,n,in0); then per block k (nblocks of them): W1 (in,out), s1 (B,in), W2 (out,out),
    s2 (B,out); then per block with a ToRGB (k >= 3): T (3,out), tau (3).
    s* = SinStyleMod.modulation(style) (mod_conv_fc.py:474) computed on the host side.
    Blocks k >= 4 use the skip connection (generator.py:1128, 971-973).
    grad_mode, ports: as InrHeadX3Function; this form keeps what a backward needs either way and has no gradient ports."""

    @staticmethod
    def forward(ctx, nblocks, grad_mode, ports, x0, *params):
        if ports is not None:
            raise RuntimeError("the exact-fp32 INR head has no gradient ports")
        x0 = _c(x0.detach())
        B, n, _ = x0.shape
        dev = x0.device
        blocks, rgbp = _head_params(nblocks, params)
        _chk(x0, *[t for blk in blocks for t in blk], *rgbp)
        saved = []
        x = x0
        rgb = torch.empty(B, n, 3, device=dev)
        first_rgb = True
        for k, (W1, s1, W2, s2) in enumerate(blocks):
            skip = k >= 4
            cout = W1.shape[1]
            wb1, wbt1, d1 = modfc_prep(W1, s1)
            pin1 = _next_pin(B, n, cout, dev)
            # pinned (tests): gate from the supplied plane (`mask` operand: C = acc * (mask > 0 ? 1 : slope))
            m1 = _bits_to_pm1(pin1) if pin1 is not None else None
            a1 = bmm_nn(x, wb1, mask=m1) if pin1 is not None else bmm_nn(x, wb1, act=1)
            wb2, wbt2, d2 = modfc_prep(W2, s2)
            pin2 = _next_pin(B, n, cout, dev)
            m2 = _bits_to_pm1(pin2) if pin2 is not None else None
            e2 = dict(mask=m2) if pin2 is not None else dict(act=1)
            if skip and a1.shape[-1] == x.shape[-1]:
                out = torch.empty_like(a1)
                a2 = bmm_nn(a1, wb2, resid=x, C2=out, **e2)
            else:
                a2 = bmm_nn(a1, wb2, **e2)
                out = a2
            if gate_debug.rec is not None:
                gate_debug.rec.append(pin1 if pin1 is not None else _sign_to_bits(a1))
                gate_debug.rec.append(pin2 if pin2 is not None else _sign_to_bits(a2))
            if k >= 3:
                T, tau = rgbp[2 * (k - 3)], rgbp[2 * (k - 3) + 1]
                torgb_fwd(out.view(B * n, -1), T, tau, rgb.view(B * n, 3), accumulate=not first_rgb)
                first_rgb = False
            # the backward's gate operands: the sign of the stored activations, or the pinned planes
            saved.append((x, a1 if m1 is None else m1, a2 if m2 is None else m2, out, wbt1, d1, wbt2, d2, a1))
            x = out
        if first_rgb:
            rgb.zero_()
        ctx.nblocks = nblocks
        ctx.blocks = blocks
        ctx.rgbp = rgbp
        ctx.saved = saved
        return rgb

    @staticmethod
    def backward(ctx, drgb):
        nblocks, blocks, rgbp, saved = ctx.nblocks, ctx.blocks, ctx.rgbp, ctx.saved
        drgb = _c(drgb)
        B, n, _ = drgb.shape
        dev = drgb.device
        drgb2 = drgb.view(B * n, 3)
        grads_blocks = [None] * nblocks
        grads_rgb = [None] * len(rgbp)
        width = saved[-1][3].shape[-1]
        g2 = torch.empty(B, n, width, device=dev)
        Dout = None     # unmasked grad wrt out_k (kept while block k has a skip)
        dx0 = None
        for k in range(nblocks - 1, -1, -1):
            xin, m1, a2, out, wbt1, d1, wbt2, d2, a1 = saved[k]      # m1, a2: gate operands (sign); a1: activation
            W1, s1, W2, s2 = blocks[k]
            skip = (k >= 4) and (a1.shape[-1] == xin.shape[-1])
            if k == nblocks - 1:
                if k >= 3:
                    T = rgbp[2 * (k - 3)]
                    Dout = torch.empty(B, n, width, device=dev) if skip else None
                    torgb_bwd_x(drgb2, T, None, a2, Dout, g2)
                else:  # degenerate configuration (fewer than 4 blocks): no gradient reaches the head
                    g2.zero_()
                    Dout = torch.zeros(B, n, width, device=dev) if skip else None
            if k >= 3:
                dT, dtau = torgb_bwd_w(out.view(B * n, -1), drgb2)
                grads_rgb[2 * (k - 3)], grads_rgb[2 * (k - 3) + 1] = dT, dtau
            # ---- mod2: y2 = a1 @ wb2 ----
            gwb2 = bmm_tn(a1, g2)                                  # (B, out, out) = a1^T @ g2
            dW2, ds2 = modfc_prep_bwd(W2, s2, d2, gwb2)
            g1 = bmm_nn(g2, wbt2, mask=m1)                         # dL/dy1 = (g2 @ wb2^T) * lrelu'(a1)
            # ---- mod1: y1 = xin @ wb1 ----
            gwb1 = bmm_tn(xin, g1)
            dW1, ds1 = modfc_prep_bwd(W1, s1, d1, gwb1)
            grads_blocks[k] = (dW1, ds1, dW2, ds2)
            if k == 0:
                dx0 = bmm_nn(g1, wbt1)
            else:
                # grad wrt out_{k-1} = dx1_k [+ Dout_k via skip] [+ drgb @ T_{k-1}], then the gate of a2_{k-1}
                a2_prev = saved[k - 1][2]
                prev_skip = (k - 1 >= 4) and (saved[k - 1][1].shape[-1] == saved[k - 1][0].shape[-1])
                newD = torch.empty(B, n, width, device=dev) if prev_skip else None
                epi = dict(mask=a2_prev, C_unmasked=newD)
                if skip:
                    epi["add"] = Dout
                if k - 1 >= 3:
                    epi["rgb_g"] = drgb2
                    epi["rgb_w"] = rgbp[2 * (k - 1 - 3)]
                g2 = bmm_nn(g1, wbt1, out=torch.empty(B, n, width, device=dev), **epi)
                Dout = newD
        return _head_grads(dx0, grads_blocks, grads_rgb)


# --------------------------------------------------------------------------------------
# H4 on the bf16 matrix cores: 3-pass split GEMM ("bf16x3"), see csrc/gemm_bf16x3.hip
# --------------------------------------------------------------------------------------
# "bf16x3" (default, ~1e-5 rel. per layer), "f32" (exact fp32 MFMA) or "bf16" (single pass on the hi planes: the AMP-class
# arithmetic — operands rounded to bf16, fp32 accumulate; ~1e-3 of the image range, ~1 % of the gradients — on one third of
# the matrix work; every GEMM of the head, forward and backward, through the cips_gemm_bf16* entry points).  Read when a head
# evaluation starts: a captured graph keeps the mode it was captured in.
INR_MODE = os.environ.get("CIPS_INR_MODE", "bf16x3")


def _x3_entry(single, suffix=""):
    """the split-plane GEMM entry point `suffix` of the 3-pass family or, with `single`, of the single-pass one"""
    name = ("cips_gemm_bf16" if single else "cips_gemm_bf16x3") + suffix
    return name, getattr(_lib.load(), name)
BF = torch.bfloat16
# The head's weight-gradient tail (style / modulated-weight gradients of all layers, ToRGB weight gradients: ~0.75 ms of streaming
# kernels at C2) depends on nothing that follows the head in the backward pass.  "side": it hangs off the head through two
# gradient ports whose autograd nodes live on the generator's side stream, so it runs next to the compositing / SIREN backward
# instead of in front of it (CIPSNet.forward; profiles/r6_cores_tail_probe.txt).  "main": everything inside InrHeadX3Function.
INR_TAIL = os.environ.get("CIPS_INR_TAIL", "side")


class Planes:
    """An fp32 matrix carried as two bf16 planes (x = hi + lo)."""
    __slots__ = ("hi", "lo")

    def __init__(self, hi, lo):
        self.hi, self.lo = hi, lo

    @staticmethod
    def empty(*shape, device):
        return Planes(torch.empty(*shape, device=device, dtype=BF), torch.empty(*shape, device=device, dtype=BF))

    def float(self):
        return self.hi.float() + self.lo.float()


X3_KERNEL = 0        # descriptor field `kernel` of every split-bf16 GEMM issued from here: 0 = the library's automatic choice
                     # (production); 1 / 2 / 3 force a kernel (cips3d_hip.h) — set by the kernel parity tests and microbenchmarks


def _x3_operands(d, A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, C):
    """the fields every split-bf16 GEMM descriptor sets: operand planes, shape, strides, the fp32 output C (M, N) and the
    constants -> d"""
    d.A_hi, d.A_lo, d.B_hi, d.B_lo = _p(A.hi), _p(A.lo), _p(Bm.hi), _p(Bm.lo)
    d.M, d.N, d.K, d.lda, d.ldb = M, N, K, lda, ldb
    d.strideA, d.strideB, d.batch = strideA, strideB, batch
    d.C, d.ldc, d.strideC = _p(C), N, M * N
    d.slope = LRELU_SLOPE
    d.kernel = X3_KERNEL
    return d


def _x3_desc(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, C=None, P=None, T=None, ldt=0, strideT=0,
             mask_out=None, add=None, rgb_g=None, rgb_w=None, C_unmasked=None, mask=None, act=0, res=None, gate_bits=0,
             torgb=None, addp=None, b_kmajor=0):
    d = _x3_operands(GemmX3Desc(), A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, C)
    d.b_kmajor = b_kmajor          # 1: Bm is stored (batch, K, ldb), row-major over the contraction index (cips3d_hip.h)
    d.P_hi, d.P_lo = (_p(P.hi), _p(P.lo)) if P is not None else (None, None)
    d.ldp, d.strideP = N, M * N
    d.T_hi, d.T_lo = (_p(T.hi), _p(T.lo)) if T is not None else (None, None)
    d.ldt, d.strideT = ldt, strideT
    d.mask_out, d.add, d.rgb_g, d.rgb_w = _p(mask_out), _p(add), _p(rgb_g), _p(rgb_w)
    d.C_unmasked, d.mask = _p(C_unmasked), _p(mask)
    d.act = act
    d.res_hi, d.res_lo = (_p(res.hi), _p(res.lo)) if res is not None else (None, None)
    d.gate_bits = gate_bits        # bit 0: `mask` is a uint8 bit plane (M, N/8); bit 1: `mask_out` is written as one
    if torgb is not None:          # (T (3, N), partials (N/128, batch*M, 4)): ToRGB forward folded into the epilogue
        d.torgb_w, d.torgb_part = _p(torgb[0]), _p(torgb[1])
    if addp is not None:           # (Planes of a gated tensor, bit plane of that gate): the addend, un-gated on the fly
        d.addp_hi, d.addp_lo, d.addp_gate, d.addp_gain = _p(addp[0].hi), _p(addp[0].lo), _p(addp[1]), 1.0 / LRELU_SLOPE
    return d


_ADDP_OK = {}


def _addp_shape_ok(n, cin, cout, nb, dev, single=False):
    """does the library take the planes addend at this shape?  (a property of the shape, of the kernel selector and of the
    kernel family: asked once per shape with stand-in pointers — the query reads only shapes, flags and pointer alignment)"""
    key = (n, cin, cout, nb, dev.index, X3_KERNEL, single)
    ok = _ADDP_OK.get(key)
    if ok is None:
        gq = Planes.empty(1, 8, 8, device=dev)
        ok = _ADDP_OK[key] = gemm_x3_takes_addp(gq, gq, n, cin, cout, cout, cout, nb, n * cout, cin * cout, P=gq,
                                                addp=(gq, gq.hi), mask=gq.hi, gate_bits=1, single=single)
    return ok


def gemm_x3_takes_addp(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, single=False, **epi):
    """True when the library runs this descriptor with the planes addend (256x256-tile kernel, interior shapes)"""
    d = _x3_desc(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, **epi)
    return bool(_x3_entry(single, "_takes_addp")[1](C.byref(d)))


# The head's dX GEMMs (dL/dx = g . Wb^T) read the forward's weight planes wbt (B, out, in) as a k-major B operand
# (descriptor field b_kmajor) wherever the library's 256x256-tile kernel takes that form, and the prep then writes no wb
# (B, in, out) planes for the layer: half the bytes of the HBM-bound prep.  False: both orientations, wb as the B operand —
# the former path, kept as the other side of the parity test (tests/test_gpu_head_bkmajor.py: rgb and every gradient equal).
HEAD_DX_BKMAJOR = True
_BKMAJOR_OK = {}


def gemm_x3_takes_bkmajor(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, **epi):
    """True when the library runs this descriptor with B read k-major (Bm (batch, K, ldb); 3-pass entry, 256x256-tile kernel)"""
    d = _x3_desc(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, b_kmajor=1, **epi)
    return bool(_lib.load().cips_gemm_bf16x3_takes_bkmajor(C.byref(d)))


def _dx_bkmajor_ok(n, cin, cout, nb, dev, single, form):
    """does the dX GEMM of a (cin, cout) layer over n pixels of nb images take the layer's wbt planes (nb, cout, cin) as its
    k-major B operand?  form: its epilogue — "gate" (gate bit plane in, planes out), "addp" (+ the planes addend), "c"
    (plain fp32 output), None (a form the k-major kernel has not: the fp32 addend or copy, bf16 gate planes).  Asked like
    _addp_shape_ok: once per shape, with stand-in pointers; the single-pass family has no k-major form."""
    if not HEAD_DX_BKMAJOR or single or form is None:
        return False
    key = (n, cin, cout, nb, dev.index, X3_KERNEL, form)
    ok = _BKMAJOR_OK.get(key)
    if ok is None:
        gq = Planes.empty(1, 8, 8, device=dev)
        epi = {"gate": dict(P=gq, mask=gq.hi, gate_bits=1), "addp": dict(P=gq, mask=gq.hi, gate_bits=1, addp=(gq, gq.hi)),
               "c": dict(C=gq.hi)}[form]
        ok = _BKMAJOR_OK[key] = gemm_x3_takes_bkmajor(gq, gq, n, cin, cout, cout, cin, nb, n * cout, cout * cin, **epi)
    return ok


def gemm_x3(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, single=False, **epi):
    """C[b][m][n] = epi(sum_k A[b][m][k] * B[b][n][k]); A, B, P, T, res: Planes; row-major aux use ld = N.
    b_kmajor=1: B is stored (batch, K, ldb) instead (refused unless gemm_x3_takes_bkmajor says yes).
    single: sum_k A_hi * B_hi only (cips_gemm_bf16; here and in the functions below)"""
    name, fn = _x3_entry(single)
    d = _x3_desc(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, **epi)
    check(fn(C.byref(d), _stream()), name)


def gemm_x3_torgb(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, P, rgb_w, rgb_b, rgb2d, accumulate, single=False, **epi):
    """gemm_x3 with planes output P followed by ToRGB forward on it (rgb2d (batch*M, 3) (+)= P . rgb_w^T + rgb_b):
    folded into the GEMM epilogue when the library's 256x256-tile kernel takes the shape (partials per 128-column
    block + one finishing launch), else the ToRGB kernel on the written planes."""
    lib = _lib.load()
    name, fn = _x3_entry(single)
    part = torch.empty(max(N // 128, 1), batch * M, 4, device=P.hi.device)
    d = _x3_desc(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, P=P, torgb=(rgb_w, part), **epi)
    if N % 128 == 0 and rgb_w.is_contiguous() and _x3_entry(single, "_fuses_torgb")[1](C.byref(d)):
        check(fn(C.byref(d), _stream()), name)
        check(lib.cips_torgb_finish(_p(part), N // 128, _p(rgb_b), _p(rgb2d), batch * M, 1 if accumulate else 0, _stream()),
              "cips_torgb_finish")
        return
    d.torgb_w, d.torgb_part = None, None
    check(fn(C.byref(d), _stream()), name)
    torgb_fwd_x3(P, rgb_w, rgb_b, rgb2d, accumulate)


def gemm_x3_km(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, Cm, single=False):
    """C[b][m][n] = sum_k A[b][k][m] * B[b][k][n]; A, B: Planes stored [K][ld] (k-major), C fp32 (M,N)."""
    name, fn = _x3_entry(single, "_km")
    d = _x3_operands(GemmX3Desc(), A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, Cm)
    check(fn(C.byref(d), _stream()), name)


def gemm_x3_km_grouped(problems, M, N, K, lda, ldb, batch, strideA, strideB, single=False):
    """problems: list of (A Planes, B Planes, C fp32) of one shape -> one launch when the library supports the shape
    (256x256 tiles), else one K-major GEMM per problem."""
    name, fn = _x3_entry(single, "_km_grouped")
    descs = (GemmX3Desc * len(problems))()
    for d, (A, Bm, Cm) in zip(descs, problems):
        _x3_operands(d, A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, Cm)
    rc = fn(descs, len(problems), _stream())
    if rc == 801:      # hipErrorNotSupported
        for (A, Bm, Cm) in problems:
            gemm_x3_km(A, Bm, M, N, K, lda, ldb, batch, strideA, strideB, Cm, single=single)
        return
    check(rc, name)


def split_planes(x, want_p=True, want_t=True):
    """x (B, rows, cols) fp32 -> Planes row-major (B,rows,cols) and transposed (B,cols,rows)."""
    lib = _lib.load()
    B, rows, cols = x.shape
    dev = x.device
    P = Planes.empty(B, rows, cols, device=dev) if want_p else None
    T = Planes.empty(B, cols, rows, device=dev) if want_t else None
    check(lib.cips_split_planes(_p(x), _p(P.hi) if P else None, _p(P.lo) if P else None,
                                _p(T.hi) if T else None, _p(T.lo) if T else None, rows, cols, cols, cols, rows, B,
                                rows * cols, rows * cols, rows * cols, _stream()), "cips_split_planes")
    return P, T


def conv1x1_smallk(x, w):
    """x (B, C<=4, H, W), w (O, C) -> y (B, O, H, W): the RGB input convs as a streaming kernel"""
    lib = _lib.load()
    B, C, H, W = x.shape
    O = w.shape[0]
    y = torch.empty(B, O, H, W, device=x.device)
    check(lib.cips_conv1x1_smallk(_p(x), _p(w), _p(y), B, C, O, H * W, _stream()), "cips_conv1x1_smallk")
    return y


def conv1x1_smallk_bwd_data(dy, w, C):
    """dy (B, O, H, W), w (O, C<=4) -> dx (B, C, H, W)"""
    lib = _lib.load()
    B, O, H, W = dy.shape
    dx = torch.empty(B, C, H, W, device=dy.device)
    check(lib.cips_conv1x1_smallk_bwd_data(_p(dy), _p(w), _p(dx), B, C, O, H * W, _stream()), "cips_conv1x1_smallk_bwd_data")
    return dx


def conv1x1_smallk_bwd_weight(dy, x):
    """dy (B, O, H, W), x (B, C<=4, H, W) -> dw (O, C) = sum over images and pixels of dy x^T: the weight gradient of the
    RGB input convs (autograd of F.conv2d in EqualConv2d.forward, exp/cips3d/models/discriminator.py:40-48, for the 1x1
    layers of :457-459)"""
    lib = _lib.load()
    B, O, H, W = dy.shape
    C = x.shape[1]
    S = lib.cips_conv1x1_smallk_bwd_weight_splits(O, H * W)
    part = torch.empty(S, O, C, device=dy.device)
    check(lib.cips_conv1x1_smallk_bwd_weight(_p(dy), _p(x), _p(part), B, C, O, H * W, _stream()), "cips_conv1x1_smallk_bwd_weight")
    return part.sum(0) if S > 1 else part[0]


def split_planes_nhwc(x):
    """x (B, C, H, W) fp32 NCHW -> NHWC split planes (B*H*W + 1, C): the transposing form of cips_split_planes; the
    extra last row is zero (the implicit-GEMM convolution reads it wherever a tap falls into the padding)."""
    lib = _lib.load()
    B, C, H, W = x.shape
    n = H * W
    hi = torch.empty(B * n + 1, C, device=x.device, dtype=BF)
    lo = torch.empty(B * n + 1, C, device=x.device, dtype=BF)
    if C % 8 == 0 and x.dtype == torch.float32 and x.is_contiguous():
        check(lib.cips_split_planes_nhwc(_p(x), _p(hi), _p(lo), B, C, n, _stream()), "cips_split_planes_nhwc")
        return Planes(hi, lo)
    hi[B * n:].zero_(); lo[B * n:].zero_()
    check(lib.cips_split_planes(_p(x), None, None, _p(hi), _p(lo), C, n, n, n, C, B, C * n, C * n, C * n, _stream()),
          "cips_split_planes")
    return Planes(hi, lo)


def conv2d_x3(wP, xP, B, Cin, H, W, O, kh, kw, stride, pad, ksplit=None, bias=None, act=False, slope=0.2, act_scale=1.0,
              single=False):
    """Implicit-GEMM convolution: wP Planes (O, kh*kw*Cin) with contraction index (tap, channel), xP NHWC Planes from
    split_planes_nhwc -> y (B, O, Ho, Wo) fp32.
    single: sum over the contraction of w_hi * x_hi only (cips_conv2d_bf16; here and in the two functions below): the lo
    planes are not read, and a shape the single-pass kernel does not take raises (hipError 801) — the caller decides
    (discriminator._single_pass)."""
    lib = _lib.load()
    name = "cips_conv2d_bf16" if single else "cips_conv2d_x3"
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    y = torch.empty(B, O, Ho, Wo, device=xP.hi.device)
    d = ConvX3Desc()
    d.w_hi, d.w_lo, d.x_hi, d.x_lo, d.y = _p(wP.hi), _p(wP.lo), _p(xP.hi), _p(xP.lo), _p(y)
    d.B, d.C, d.H, d.W, d.O, d.kh, d.kw, d.stride, d.pad = B, Cin, H, W, O, kh, kw, stride, pad
    ks = getattr(lib, name + "_ksplit")(B, O, Ho * Wo, kh * kw * Cin) if ksplit is None else ksplit
    part = None
    if ks > 1:                                   # few output tiles: split the contraction over the idle CUs
        part = torch.empty(ks, B, O, Ho, Wo, device=xP.hi.device)
        d.ksplit, d.part = ks, _p(part)
    else:
        d.ksplit, d.part = 1, None
    d.bias = _p(bias) if bias is not None else None            # EqualConv2d + FusedLeakyReLU in the epilogue
    d.act, d.slope, d.act_scale = (1 if act else 0), float(slope), float(act_scale)
    check(getattr(lib, name)(C.byref(d), _stream()), name)
    return y


def dgrad_s2_banks(w):
    """w (O, C, kh, kw) fp32 -> (Planes of the four parity filter banks back to back, element offsets [4]) for
    conv2d_x3_dgrad_s2: bank (a, b) = [C][(ty, tx, o)] with w[o][c][a + 2(Ta-1-ty)][b + 2(Tb-1-tx)] (include/cips3d_hip.h)."""
    O, C, kh, kw = w.shape
    parts, offs, tot = [], [], 0
    for a in range(2):
        for b in range(2):
            offs.append(tot)
            sub = w[:, :, a::2, b::2]
            if sub.numel() == 0:
                continue
            bank = sub.flip(2, 3).permute(1, 2, 3, 0).reshape(-1)          # (C, Ta, Tb, O)
            parts.append(bank)
            tot += bank.numel()
    flat = torch.cat(parts).contiguous()
    P, _ = split_planes(flat.view(1, tot // 32, 32), want_p=True, want_t=False)
    return P, offs


def dgrad_s2_layout(H, W):
    """-> (element offsets [4] of the parity blocks per (B*C) planes, plane sizes Np[4]) for an (H, W) input"""
    nps = []
    for a in range(2):
        for b in range(2):
            hs, ws = (H - a + 1) // 2, (W - b + 1) // 2
            nps.append((hs * ws + 7) // 8 * 8)
    return nps


def conv2d_x3_dgrad_s2(banks, w_off, dyP, B, Cin, H, W, O, kh, kw, single=False):
    """Data gradient of a stride-2 unpadded convolution as four parity sub-convolutions in one launch (cips_conv2d_x3_dgrad_s2).
    banks / w_off: dgrad_s2_banks(w); dyP: NHWC Planes of dy (B, O, Ho, Wo).  -> (dxp fp32 flat, out_off [4]): the gradient w.r.t.
    the (B, Cin, H, W) input in parity-block layout, consumed by upfirdn2d_parity (or parity_to_nchw in tests)."""
    lib = _lib.load()
    nps = dgrad_s2_layout(H, W)
    # the four blocks are read TOGETHER by upfirdn2d_parity (one output needs all four parities); with B*C a power of two
    # their natural offsets are congruent modulo 64 KiB and the four streams queue on the same memory channels — skew them
    out_off, tot = [], 0
    for i, n_ in enumerate(nps):
        tot += i * 1184                     # floats: 4 736 B, 16-byte granular
        out_off.append(tot)
        tot += B * Cin * n_
    dxp = torch.empty(tot, device=dyP.hi.device)
    d = ConvDgradS2Desc()
    d.w_hi, d.w_lo, d.dy_hi, d.dy_lo, d.dxp = _p(banks.hi), _p(banks.lo), _p(dyP.hi), _p(dyP.lo), _p(dxp)
    d.B, d.C, d.H, d.W, d.O, d.kh, d.kw = B, Cin, H, W, O, kh, kw
    for i in range(4):
        d.w_off[i] = w_off[i]
        d.out_off[i] = out_off[i]
    name = "cips_conv2d_bf16_dgrad_s2" if single else "cips_conv2d_x3_dgrad_s2"
    check(getattr(lib, name)(C.byref(d), _stream()), name)
    return dxp, out_off


def parity_to_nchw(dxp, out_off, B, C, H, W):
    """the parity-block layout of conv2d_x3_dgrad_s2 as an ordinary (B, C, H, W) tensor (tests / fallbacks: torch indexing)"""
    out = torch.empty(B, C, H, W, device=dxp.device)
    nps = dgrad_s2_layout(H, W)
    for a in range(2):
        for b in range(2):
            hs, ws = (H - a + 1) // 2, (W - b + 1) // 2
            i = 2 * a + b
            blk = dxp[out_off[i]:out_off[i] + B * C * nps[i]].view(B, C, nps[i])[:, :, :hs * ws].reshape(B, C, hs, ws)
            out[:, :, a::2, b::2] = blk
    return out


def upfirdn2d_parity(dxp, out_off, kernel, major, in_h, in_w, pad_x0, pad_x1, pad_y0, pad_y1):
    """cips_upfirdn2d (4 x 4 kernel, up = down = 1) on planes stored as conv2d_x3_dgrad_s2's parity blocks -> (major, out_h, out_w)"""
    lib = _lib.load()
    k = _native_in(kernel, "kernel")
    if tuple(k.shape) != (4, 4):
        raise RuntimeError("upfirdn2d_parity: 4 x 4 kernels only")
    out_h, out_w = in_h + pad_y0 + pad_y1 - 3, in_w + pad_x0 + pad_x1 - 3
    out = torch.empty(major, out_h, out_w, device=dxp.device)
    offs = (C.c_longlong * 4)(*out_off)
    check(lib.cips_upfirdn2d_parity(_p(dxp), C.byref(offs), _p(k), _p(out), major, in_h, in_w, pad_x0, pad_x1, pad_y0, pad_y1,
                                    _stream()), "cips_upfirdn2d_parity")
    return out


def conv2d_x3_wgrad_declines(B, N):
    """conv2d_x3_wgrad's contraction runs over the B * N output pixels of the batch in 32-row k-tiles"""
    return (B * N) % 32 != 0


def conv2d_bf16_wgrad_declines(B, N):
    """the single-pass weight gradient (conv2d_x3_wgrad(single=True)) walks 64-row k-tiles, two at least"""
    return (B * N) % 64 != 0 or B * N < 128


def conv2d_x3_wgrad(dyP, xP, B, Cin, H, W, O, kh, kw, stride, pad, scale=1.0, nch=None, single=False):
    """Weight gradient of conv2d_x3: dyP, xP NHWC Planes from split_planes_nhwc -> dW (O, Cin, kh, kw) fp32, or None when
    the pixel count does not split into 32-row k-tiles (conv2d_x3_wgrad_declines; single: into 64-row k-tiles,
    conv2d_bf16_wgrad_declines).  The pixel range is cut into chunks so
    that a 512x512 filter bank still fills the chip (4 tiles per tap and chunk); cips_conv_wgrad_finish adds the partial
    sums, applies `scale` and lays the result out as (O, Cin, kh, kw)."""
    lib = _lib.load()
    Ho, Wo = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    K = B * Ho * Wo
    if (conv2d_bf16_wgrad_declines if single else conv2d_x3_wgrad_declines)(B, Ho * Wo):
        return None
    # chunks of the pixel range: the persistent grid runs ceil(tiles*nch / 256) rounds of ~K/nch rows each (+ an
    # epilogue worth ~512 rows); 36 tiles x 7 chunks = 252 of 256 CUs in one round (powers of two: 144, or 288 in two)
    tiles = ((O + 255) // 256) * ((Cin + 255) // 256) * kh * kw
    kt_rows, kt_cost = (64, 21) if single else (32, 32)       # a 64-row single-pass k-tile: 32 MFMAs against a 32-row k-tile's 48
    T = K // kt_rows
    best = None
    forced = nch
    nch = 1
    for cand in range(1, 33):                   # any count: the kernel cuts the range at k-tile granularity
        if cand > 1 and T // cand < 8:
            break
        cost = -(-tiles * cand // 256) * (-(-T // cand) * kt_cost + 512)
        if best is None or cost < best:
            nch, best = cand, cost
    if forced is not None:
        nch = forced
    part = torch.empty(nch, kh * kw, O, Cin, device=xP.hi.device)
    d = ConvWgradDesc()
    d.dy_hi, d.dy_lo, d.x_hi, d.x_lo, d.part = _p(dyP.hi), _p(dyP.lo), _p(xP.hi), _p(xP.lo), _p(part)
    d.B, d.C, d.H, d.W, d.O, d.kh, d.kw, d.stride, d.pad, d.nchunks = B, Cin, H, W, O, kh, kw, stride, pad, nch
    name = "cips_conv2d_bf16_wgrad" if single else "cips_conv2d_x3_wgrad"
    check(getattr(lib, name)(C.byref(d), _stream()), name)
    dw = torch.empty(O, Cin, kh, kw, device=xP.hi.device)
    check(lib.cips_conv_wgrad_finish(_p(part), _p(dw), nch, kh * kw, O, Cin, float(scale), _stream()), "cips_conv_wgrad_finish")
    return dw


def _modfc_prep_x3_out(W, B, want_wb=True):
    """what one layer's split-plane prep writes: wb Planes (B,in,out) — None when not wanted —, wbt Planes (B,out,in),
    demod (B,out)"""
    in_dim, out_dim = W.shape
    return (Planes.empty(B, in_dim, out_dim, device=W.device) if want_wb else None,
            Planes.empty(B, out_dim, in_dim, device=W.device), torch.empty(B, out_dim, device=W.device))


def modfc_prep_x3(W, s, eps=1e-8, want_wb=True):
    """one layer through the single-job entry: the scalar kernels whatever the shape"""
    lib = _lib.load()
    in_dim, out_dim = W.shape
    B = s.shape[0]
    wb, wbt, demod = _modfc_prep_x3_out(W, B, want_wb)
    check(lib.cips_modfc_prep_x3(_p(W), _p(s), _p(wb.hi) if wb else None, _p(wb.lo) if wb else None, _p(wbt.hi), _p(wbt.lo),
                                 _p(demod), B, in_dim, out_dim, eps, _stream()), "cips_modfc_prep_x3")
    return wb, wbt, demod


def modfc_prep_x3_batch(layers, eps=1e-8, want_wb=None):
    """layers: list of (W (in,out), s (B,in)) -> list of (wb Planes (B,in,out), wbt Planes (B,out,in), demod (B,out)),
    all layers in two launches.  want_wb: one flag per layer, False = no wb planes for it (None in its place)."""
    lib = _lib.load()
    mx = lib.cips_modfc_max_jobs()
    out = []
    for c0 in range(0, len(layers), mx):
        chunk = layers[c0:c0 + mx]
        jobs = (ModfcPrepJob * len(chunk))()
        B = chunk[0][1].shape[0]
        for i, (j, (W, s)) in enumerate(zip(jobs, chunk)):
            wb, wbt, demod = _modfc_prep_x3_out(W, B, want_wb is None or want_wb[c0 + i])
            j.weight, j.s, j.demod = _p(W), _p(s), _p(demod)
            j.wb_hi, j.wb_lo = (_p(wb.hi), _p(wb.lo)) if wb is not None else (None, None)
            j.wbt_hi, j.wbt_lo = _p(wbt.hi), _p(wbt.lo)
            j.in_dim, j.out_dim = W.shape
            out.append((wb, wbt, demod))
        check(lib.cips_modfc_prep_x3_batch(jobs, len(chunk), B, eps, _stream()), "cips_modfc_prep_x3_batch")
    return out


def _modfc_form(entry, job_type, shapes, B):
    jobs = (job_type * max(len(shapes), 1))()
    for j, (in_dim, out_dim) in zip(jobs, shapes):
        j.in_dim, j.out_dim = in_dim, out_dim
    code = getattr(_lib.load(), entry)(jobs, len(shapes), B)
    if code < 0:
        raise ValueError(f"{entry[:-5]} refuses these jobs (hipError {-code})")
    return code


def modfc_prep_x3_batch_form(shapes, B):
    """which kernels one call of cips_modfc_prep_x3_batch runs for layers of these (in_dim, out_dim) shapes (at most
    cips_modfc_max_jobs() of them: one chunk of modfc_prep_x3_batch), host only: bit 0 (CIPS_MODFC_PREP_COLSUM16) 16-byte
    column sums, bit 1 (CIPS_MODFC_PREP_TILES64) 64 x 64 plane tiles; ValueError for jobs the entry point refuses"""
    return _modfc_form("cips_modfc_prep_x3_batch_form", ModfcPrepJob, shapes, B)


def modfc_prep_bwd_batch_form(shapes, B):
    """the same for cips_modfc_prep_bwd_batch: 0 the scalar three-pass kernels, 2 / 4 the fused dW / ds pass of 2 / 4
    chunks of 256 columns (CIPS_MODFC_BWD_*)"""
    return _modfc_form("cips_modfc_prep_bwd_batch_form", ModfcBwdJob, shapes, B)


def modfc_prep_bwd_batch(layers, cores=False):
    """layers: list of (W, s, demod, gwb) -> list of (dW, ds), all layers in three launches.  cores=True: the co-resident
    form (no LDS, <= 40 VGPRs: runs beside the fused SIREN backward when issued on a side stream; B <= 64, out % 4 == 0)."""
    lib = _lib.load()
    mx = lib.cips_modfc_max_jobs()
    out = []
    cores = bool(cores) and layers[0][1].shape[0] <= 64 and all(W.shape[1] % 4 == 0 for W, _, _, _ in layers)
    parts = lib.cips_cores_colsum_parts() if cores else 1
    for c0 in range(0, len(layers), mx):
        chunk = layers[c0:c0 + mx]
        jobs = (ModfcBwdJob * len(chunk))()
        B = chunk[0][1].shape[0]
        keep = []
        for j, (W, s, demod, gwb) in zip(jobs, chunk):
            in_dim, out_dim = W.shape
            dev = W.device
            cbuf = torch.empty(parts, B, out_dim, device=dev)
            dW = torch.empty(in_dim, out_dim, device=dev)
            ds = torch.empty(B, in_dim, device=dev)
            j.weight, j.s, j.demod, j.gwb = _p(W), _p(s), _p(demod), _p(gwb)
            j.cbuf, j.dweight, j.ds = _p(cbuf), _p(dW), _p(ds)
            j.in_dim, j.out_dim = in_dim, out_dim
            keep.append(cbuf)
            out.append((dW, ds))
        if cores:
            check(lib.cips_modfc_prep_bwd_batch_cores(jobs, len(chunk), B, _stream()), "cips_modfc_prep_bwd_batch_cores")
        else:
            check(lib.cips_modfc_prep_bwd_batch(jobs, len(chunk), B, _stream()), "cips_modfc_prep_bwd_batch")
    return out


def torgb_fwd_x3(xp, w, b, rgb2d, accumulate):
    lib = _lib.load()
    K = xp.hi.shape[-1]
    M = xp.hi.numel() // K
    check(lib.cips_torgb_fwd_x3(_p(xp.hi), _p(xp.lo), _p(w), _p(b), _p(rgb2d), M, K, 1 if accumulate else 0,
                                _stream()), "cips_torgb_fwd_x3")


def torgb_bwd_w_x3(xp, drgb2d):
    lib = _lib.load()
    K = xp.hi.shape[-1]
    M = xp.hi.numel() // K
    chunks = lib.cips_torgb_bwd_partials(M)
    part = torch.empty(chunks, 4, K, device=drgb2d.device)
    dw = torch.empty(3, K, device=drgb2d.device)
    db = torch.empty(3, device=drgb2d.device)
    check(lib.cips_torgb_bwd_w_x3(_p(xp.hi), _p(xp.lo), _p(drgb2d), _p(part), _p(dw), _p(db), M, K, _stream()),
          "cips_torgb_bwd_w_x3")
    return dw, db


def torgb_bwd_w_x3_batch(xps, drgb2d, cores=False):
    """the ToRGB weight / bias gradients of several taps (Planes of one shape) against one drgb: list of (dw (3, K), db (3,)).
    Two launches for all of them when K = 512 (<= 8 taps), else one pair per tap.  cores=True: the co-resident form of the
    batched launch (see modfc_prep_bwd_batch)."""
    lib = _lib.load()
    K = xps[0].hi.shape[-1]
    M = xps[0].hi.numel() // K
    n = len(xps)
    if K != 512 or n > 8 or n < 2:
        return [torgb_bwd_w_x3(xp, drgb2d) for xp in xps]
    chunks = lib.cips_torgb_bwd_partials(M)
    dev = drgb2d.device
    part = torch.empty(n, chunks, 4, K, device=dev)
    dw = torch.empty(n, 3, K, device=dev)
    db = torch.empty(n, 3, device=dev)
    hi = (C.c_void_p * n)(*[_p(xp.hi) for xp in xps])
    lo = (C.c_void_p * n)(*[_p(xp.lo) for xp in xps])
    fn = lib.cips_torgb_bwd_w_x3_batch_cores if cores else lib.cips_torgb_bwd_w_x3_batch
    check(fn(hi, lo, n, _p(drgb2d), _p(part), _p(dw), _p(db), M, K, _stream()), "cips_torgb_bwd_w_x3_batch")
    return [(dw[i], db[i]) for i in range(n)]


# ToRGB forward folded into the epilogue of the block's second GEMM wherever the 256x256-tile kernel takes the shape
# (else the separate ToRGB kernel).  Backward: the skip gradient is re-read from the previous layer's GATED planes (un-gated
# on the fly with that gate's bit plane) instead of from a separate fp32 copy the previous GEMM would have to write, and the
# ToRGB tap's gradient into the last block's output is one streaming kernel — both where the shapes allow (bit-plane gates,
# interior tiles); the fp32 copy / the K = 32 zero-padded GEMM remain as the ragged-shape forms.


class _HeadLayer:
    """One SinBlock of the split-bf16 head: what the forward plans and writes, and what the backward reads.  gate1 / gate2:
    the LeakyReLU gates of a1 and of the block output as the backward's `mask` operand takes them — bit planes (`bits`;
    written by the forward's epilogues unless pinned), else the bf16 sign form: a1's own hi plane, and the output's hi
    plane or, behind a skip connection, a copy of a2's sign the forward writes."""
    __slots__ = ("cin", "cout", "skip", "bits", "pinned1", "pinned2", "xP", "a1P", "gate1", "oP", "gate2", "wb1", "d1", "wb2",
                 "d2", "wbt1", "wbt2")      # per modulated layer one of wb / wbt is kept, the other None (_head_dx_kmajor)


def _head_addp(layers, bits, n, nb, dev, single):
    """the backward recovers the skip gradient from the previous layer's gated planes (no fp32 copy): every layer has
    bit-plane gates and the 256x256-tile kernel takes the planes addend at the skip layers' shapes"""
    fam = {"single": True} if single else {}       # the default mode asks exactly as before
    return all(bits) and all(_addp_shape_ok(n, L.cin, L.cout, nb, dev, **fam) for L in layers[1:] if L.skip)


def _head_dx_kmajor(layers, n, nb, dev, single, train):
    """per block (dX through W1, dX through W2): True where the backward's dX GEMM reads the forward's wbt planes k-major, so
    that the prep writes no wb planes for the layer.  Decided from the epilogue the backward will launch (the rules of
    InrHeadX3Function.backward, below) and the library's query.  Without `train` nothing is kept and no backward follows:
    the plan is the one of the training step at the same shapes."""
    bits = [L.bits if train else L.cout % 32 == 0 for L in layers]
    addp = _head_addp(layers, bits, n, nb, dev, single)
    plan = []
    for k, L in enumerate(layers):
        if k == 0:
            form1 = "c"
        elif not bits[k - 1]:
            form1 = None
        elif L.skip:
            form1 = "addp" if addp else None
        elif k - 1 >= 3:
            form1 = None                                # the rgb term without an addend: no 256x256-tile form at all
        else:
            form1 = "gate" if addp or not layers[k - 1].skip else None
        plan.append((_dx_bkmajor_ok(n, L.cin, L.cout, nb, dev, single, form1),
                     _dx_bkmajor_ok(n, L.cout, L.cout, nb, dev, single, "gate" if bits[k] else None)))
    return plan


def _pixel_split(n, ksp, more):
    """pixel-split factor of a per-image weight gradient over n pixels: `ksp`, doubled while `more(ksp)` holds and the
    halves stay whole 32-row k-tiles of at least 512 rows"""
    while more(ksp) and n % (2 * ksp * 32) == 0 and n // (2 * ksp) >= 512:
        ksp *= 2
    return ksp


def _split_parts(out, ksp):
    """what a weight-gradient GEMM split in `ksp` pixel parts writes: `out` (nb, M, N) itself, or (nb*ksp, M, N) partials"""
    return out if ksp == 1 else torch.empty(out.shape[0] * ksp, *out.shape[1:], device=out.device)


def _sum_split(part, out):
    """out (nb, M, N) = the sum of the pixel-split partials `part` (nb*ksp, M, N); nothing to do when part is out"""
    if part is not out:
        torch.sum(part.view(out.shape[0], -1, *out.shape[1:]), dim=1, out=out)


def _wgrad_km(A, G, out, n, ksp, defer=False, single=False):
    """out[b] (M, N) = A[b]^T G[b] over the n pixels of image b (A (nb, n, M), G (nb, n, N) row-major Planes) on the K-major
    GEMM, the pixel range split in `ksp` parts — a pure view, (nb, n, C) -> (nb*ksp, n/ksp, C).  The partial products are
    summed into `out` here, or with `defer` by the caller's _sum_split of what this returns."""
    nb, M, N = out.shape
    part = _split_parts(out, ksp)
    nk = n // ksp
    gemm_x3_km(A, G, M, N, nk, M, N, nb * ksp, nk * M, nk * N, part, single=single)
    if defer:
        return part
    _sum_split(part, out)
    return out


def _head_wgrad(L, gP, g1P, gwb1, gwb2, n, single=False):
    """the per-image weight gradients of one block: dWb2 = a1^T g, dWb1 = x^T g1.  Each contracts over the n pixels of one
    image; with few images per GPU a 512x512 output is too few tiles for the chip, so the pixel range is split in parts and
    the partial products are summed."""
    nb, cin, cout = gwb1.shape
    ksp = _pixel_split(n, 1, lambda s: nb * s < 32)
    if cin == cout:
        part2, part1 = _split_parts(gwb2, ksp), _split_parts(gwb1, ksp)
        nk = n // ksp
        gemm_x3_km_grouped([(L.a1P, gP, part2), (L.xP, g1P, part1)], cout, cout, nk, cout, cout, nb * ksp, nk * cout, nk * cout,
                           single=single)
    else:
        # the block's square problem alone is half a chip of 256 x 256 tiles: two pixel halves fill it
        tiles = (cout + 255) // 256
        ksp2 = _pixel_split(n, ksp, lambda s: nb * s * tiles * tiles < 192)
        part2 = _wgrad_km(L.a1P, gP, gwb2, n, ksp2, defer=ksp2 == ksp, single=single)
        # a narrow first layer (cin = 32: one row tile, 2 column tiles per image = 64 workgroups) streams the whole gradient
        # plane through a quarter of the chip: split its pixel range further
        ksp1 = _pixel_split(n, ksp, lambda s: cin <= 128 and nb * s * tiles < 192)
        part1 = _wgrad_km(L.xP, g1P, gwb1, n, ksp1, defer=ksp1 == ksp, single=single)
    # partials of the common split `ksp` are summed here, dWb2 first (those of a split of its own right after their GEMM)
    _sum_split(part2, gwb2)
    _sum_split(part1, gwb1)


class InrHeadX3Function(torch.autograd.Function):
    """Same contract as InrHeadFunction, on the split-plane GEMMs: 3 passes (INR_MODE "bf16x3") or, in INR_MODE "bf16", the
    single pass on the hi planes for every GEMM of the forward and of the backward (the mode of the forward holds for its
    backward).  Every activation / gradient lives in HBM as row-major bf16
    hi/lo planes written by the producing GEMM's epilogue: the A operand of the next forward GEMM and of the dX GEMM, read
    k-major by the weight-gradient GEMMs.

    ports: None, or the TailPorts of inr_head_open_ports — the parameters then come detached and are followed by the ports'
    handles, which the backward answers with dL/dWb of every layer and drgb (the weight-gradient tail runs in the ports'
    backward nodes)."""

    @staticmethod
    def forward(ctx, nblocks, grad_mode, ports, x0, *params):
        x0 = _c(x0.detach())
        B, n, in0 = x0.shape
        if n % 32 or in0 % 32:
            raise RuntimeError("bf16x3 INR path needs pixels per image and feature width to be multiples of 32")
        dev = x0.device
        sp = ctx.single = INR_MODE == "bf16"
        blocks, rgbp = _head_params(nblocks, params)
        _chk(x0, *[t for blk in blocks for t in blk], *rgbp)
        train = grad_mode and any(ctx.needs_input_grad)       # no-grad / inference: nothing kept
        x0P, _ = split_planes(x0, want_t=False)
        rgb = torch.empty(B, n, 3, device=dev)
        dbg = gate_debug.active                                     # gate instrumentation (tests): bit planes always
        layers = []
        for k, (W1, s1, W2, s2) in enumerate(blocks):
            L = _HeadLayer()
            L.cin, L.cout = W1.shape
            L.skip = (k >= 4) and (L.cin == L.cout)
            # LeakyReLU gates as bit planes (1 bit per activation, written by the forward GEMMs' epilogues) instead of bf16
            # planes: 2.5 GB less HBM traffic per C2 step (layer widths that are not multiples of 32 keep the bf16 form)
            L.bits = (train or dbg) and L.cout % 32 == 0
            layers.append(L)
        # modulate / demodulate / split every layer's weights up front, in one batch: the planes wbt (B, out, in) of the
        # forward GEMMs, and wb (B, in, out) only for the layers whose dX GEMM does not read wbt k-major
        kmajor = _head_dx_kmajor(layers, n, B, dev, sp, train)
        prepped = modfc_prep_x3_batch([(W, s_) for (W1, s1, W2, s2) in blocks for (W, s_) in ((W1, s1), (W2, s2))],
                                      want_wb=[not f for pair in kmajor for f in pair])
        # every buffer is allocated here, before the first GEMM
        xP = x0P
        for k, L in enumerate(layers):
            cin, cout, bits = L.cin, L.cout, L.bits
            pin1 = _next_pin(B, n, cout, dev)
            pin2 = _next_pin(B, n, cout, dev)
            if (pin1 is not None or gate_debug.rec is not None) and not bits:
                raise RuntimeError("gate instrumentation needs layer widths that are multiples of 32")
            L.pinned1, L.pinned2 = pin1 is not None, pin2 is not None
            L.xP = xP
            L.a1P = Planes.empty(B, n, cout, device=dev)
            L.gate1 = pin1 if pin1 is not None else (torch.empty(B, n, cout // 8, device=dev, dtype=torch.uint8) if bits else L.a1P.hi)
            L.oP = Planes.empty(B, n, cout, device=dev)
            if pin2 is not None:
                L.gate2 = pin2
            elif bits:
                L.gate2 = torch.empty(B, n, cout // 8, device=dev, dtype=torch.uint8)
            elif L.skip:
                L.gate2 = torch.empty(B, n, cout, device=dev, dtype=BF) if train else None
            else:
                L.gate2 = L.oP.hi
            # the dX operand of each modulated layer: wb, or (wb None) the forward's own wbt planes
            L.wb1, wbt1, L.d1 = prepped[2 * k]
            L.wb2, wbt2, L.d2 = prepped[2 * k + 1]
            L.wbt1, L.wbt2 = (wbt1 if L.wb1 is None else None), (wbt2 if L.wb2 is None else None)
            xP = L.oP
        first_rgb = True
        for k, L in enumerate(layers):
            cin, cout = L.cin, L.cout
            wbt1, wbt2 = prepped[2 * k][1], prepped[2 * k + 1][1]
            res = L.xP if L.skip else None
            if L.pinned1:
                # pinned: `gate ? 1 : slope` from the supplied plane in place of the LeakyReLU on the computed sign
                gemm_x3(L.xP, wbt1, n, cout, cin, cin, cin, B, n * cin, cout * cin, P=L.a1P, mask=L.gate1, gate_bits=1, single=sp)
            else:
                gemm_x3(L.xP, wbt1, n, cout, cin, cin, cin, B, n * cin, cout * cin, P=L.a1P, act=1,
                        mask_out=L.gate1 if L.bits else None, gate_bits=2 if L.bits else 0, single=sp)
            mod2 = (L.a1P, wbt2, n, cout, cout, cout, cout, B, n * cout, cout * cout)
            if L.pinned2:
                gemm_x3(*mod2, P=L.oP, res=res, mask=L.gate2, gate_bits=1, single=sp)
            elif L.bits and k >= 3:
                gemm_x3_torgb(*mod2, L.oP, rgbp[2 * (k - 3)], rgbp[2 * (k - 3) + 1], rgb.view(B * n, 3), not first_rgb,
                              act=1, res=res, mask_out=L.gate2, gate_bits=2, single=sp)
                first_rgb = False
                continue
            elif L.bits:
                gemm_x3(*mod2, P=L.oP, act=1, res=res, mask_out=L.gate2, gate_bits=2, single=sp)
            elif L.skip:
                gemm_x3(*mod2, P=L.oP, act=1, res=res, mask_out=L.gate2, single=sp)
            else:
                gemm_x3(*mod2, P=L.oP, act=1, single=sp)
            if k >= 3:
                torgb_fwd_x3(L.oP, rgbp[2 * (k - 3)], rgbp[2 * (k - 3) + 1], rgb.view(B * n, 3), accumulate=not first_rgb)
                first_rgb = False
        if gate_debug.rec is not None:
            for L in layers:
                gate_debug.rec.append(L.gate1)
                gate_debug.rec.append(L.gate2)
        if nblocks <= 3:
            rgb.zero_()
        # kept for backward: every layer's input / a1 / output planes, both gates and the prepped weights
        ctx.layers, ctx.blocks, ctx.rgbp = (layers if train else []), blocks, rgbp
        ctx.dims = (B, n)
        ctx.ports = ports if train else None
        if ctx.ports is not None:
            ports.demod = [d for L in layers for d in (L.d1, L.d2)]
            ports.taps = [L.oP for L in layers[3:]]
        return rgb

    @staticmethod
    def backward(ctx, drgb):
        layers, blocks, rgbp, ports = ctx.layers, ctx.blocks, ctx.rgbp, ctx.ports
        nblocks = len(layers)
        B, n = ctx.dims
        sp = ctx.single
        fam = {"single": True} if sp else {}       # the default mode calls the two helpers below exactly as before
        drgb = _c(drgb)
        dev = drgb.device
        drgb2 = drgb.reshape(B * n, 3)
        width = layers[-1].cout
        # per-image dL/dWb of every layer (gwb1, gwb2) and dx0
        gwb = [(torch.empty(B, L.cin, L.cout, device=dev), torch.empty(B, L.cout, L.cout, device=dev)) for L in layers]
        dx0 = torch.empty(B, n, layers[0].cin, device=dev)
        gP = Planes.empty(B, n, width, device=dev)
        # the skip gradient D (un-gated) is either kept as an fp32 copy next to the gated planes every GEMM writes
        # for its successors, or — when every layer has bit-plane gates and the 256x256-tile kernel takes the shapes —
        # recovered from those planes by the consumer: no copy written, same bytes read
        addp = _head_addp(layers, [L.bits for L in layers], n, B, dev, sp)
        k, L = nblocks - 1, layers[-1]
        Dout = None
        if k >= 3 and L.bits and width % 8 == 0:
            # grad wrt out_k = drgb @ T_k (rank 3), gate of a2_k fused: one streaming kernel writing the planes
            Dout = torch.empty(B, n, width, device=dev) if L.skip and not addp else None
            torgb_bwd_x_x3(drgb2, rgbp[2 * (k - 3)], L.gate2, Dout, gP)
        elif k >= 3:
            # ... else as a K=32 zero-padded bf16x3 GEMM
            tpad = torch.zeros(1, width, 32, device=dev); tpad[0, :, :3] = rgbp[2 * (k - 3)].t()
            tP, _ = split_planes(tpad, want_t=False)
            dpad = torch.zeros(B, n, 32, device=dev); dpad[..., :3] = drgb
            dP, _ = split_planes(dpad, want_t=False)
            Dout = torch.empty(B, n, width, device=dev) if L.skip and not addp else None
            gemm_x3(dP, tP, n, width, 32, 32, 32, B, n * 32, 0, P=gP, C_unmasked=Dout, mask=L.gate2,
                    gate_bits=1 if L.bits else 0, single=sp)
        else:
            gP.hi.zero_(); gP.lo.zero_()
            Dout = torch.zeros(B, n, width, device=dev) if L.skip and not addp else None
        # ToRGB weight / bias gradients of all taps: they need only the saved block outputs and drgb
        grads_rgb = []
        if ports is None and nblocks > 3:
            for dT, dtau in torgb_bwd_w_x3_batch([L.oP for L in layers[3:]], drgb2):
                grads_rgb += [dT, dtau]
        for k in range(nblocks - 1, -1, -1):
            L = layers[k]
            cin, cout = L.cin, L.cout
            gP_in = gP              # D_{k+1} gated by a2_k's gate: the planes form of the skip gradient
            # ---- mod2: gradient through the gate of a1 ----
            g1P = Planes.empty(B, n, cout, device=dev)
            # the weights as the B operand of a dX GEMM: wb (in, out) = [N][K], or the forward's wbt (out, in) = [K][N] read k-major
            w2 = (L.wb2, cout) if L.wb2 is not None else (L.wbt2, cout)
            w1 = (L.wb1, cout) if L.wb1 is not None else (L.wbt1, cin)
            km2, km1 = {"b_kmajor": 1} if L.wb2 is None else {}, {"b_kmajor": 1} if L.wb1 is None else {}
            gemm_x3(gP, w2[0], n, cout, cout, cout, w2[1], B, n * cout, cout * cout, P=g1P, mask=L.gate1,
                    gate_bits=1 if L.bits else 0, single=sp, **km2)
            _head_wgrad(L, gP, g1P, *gwb[k], n, **fam)
            if k == 0:
                gemm_x3(g1P, w1[0], n, cin, cout, cout, w1[1], B, n * cout, cin * cout, C=dx0, single=sp, **km1)
            else:
                prev = layers[k - 1]
                newD = torch.empty(B, n, cin, device=dev) if prev.skip and not addp else None
                gP = Planes.empty(B, n, cin, device=dev)
                gemm_x3(g1P, w1[0], n, cin, cout, cout, w1[1], B, n * cout, cin * cout, P=gP, **km1,
                        add=Dout if L.skip and not addp else None, addp=(gP_in, L.gate2) if L.skip and addp else None,
                        rgb_g=drgb2 if k - 1 >= 3 else None, rgb_w=rgbp[2 * (k - 1 - 3)] if k - 1 >= 3 else None,
                        C_unmasked=newD, mask=prev.gate2, gate_bits=1 if prev.bits else 0, single=sp)
                Dout = newD
        if ports is not None:
            _TAIL_GATE[dev.index] = ports        # armed: the next compositing backward publishes its event to the ports
            # the tail runs in the ports' backward nodes (side stream): hand them dL/dWb of every layer and drgb
            return (None, None, None, dx0) + (None,) * (4 * nblocks + len(rgbp)) + tuple(g for pair in gwb for g in pair) + (drgb,)
        pending = []      # (W, s, demod, dL/dWb) of every layer: their prep backward runs as one batch
        for k in range(nblocks - 1, -1, -1):
            W1, s1, W2, s2 = blocks[k]
            pending.append((W2, s2, layers[k].d2, gwb[k][1]))
            pending.append((W1, s1, layers[k].d1, gwb[k][0]))
        res = modfc_prep_bwd_batch(pending)          # pending order: block nblocks-1 (mod2, mod1), ..., block 0
        grads_blocks = [None] * nblocks
        for i, k in enumerate(range(nblocks - 1, -1, -1)):
            (dW2, ds2), (dW1, ds1) = res[2 * i], res[2 * i + 1]
            grads_blocks[k] = (dW1, ds1, dW2, ds2)
        return _head_grads(dx0, grads_blocks, grads_rgb)


class TailPorts:
    """The gradient ports of one head evaluation (see INR_TAIL), from inr_head_open_ports.  `handles`: their outputs, the
    trailing inputs of InrHeadX3Function — one per modulated layer, then the ToRGB one.  The head's forward fills in `demod`
    and `taps`; `gate` is the event of the compositing backward (see _TAIL_GATE), and `waited` records that the ports'
    backward waited for one.  The ports' nodes hold it by weak reference — it holds their outputs, and a strong reference
    back would close a cycle through the autograd graph that Python's collector cannot free; the head's node keeps it
    alive until they have run."""
    __slots__ = ("handles", "demod", "taps", "gate", "waited", "__weakref__")

    def __init__(self):
        self.handles, self.demod, self.taps, self.gate, self.waited = (), None, None, None, False

    def wait(self, dev):
        """in a port's backward, on its stream: disarm the gate, then wait for the event published while it was armed"""
        if _TAIL_GATE.get(dev.index) is self:
            del _TAIL_GATE[dev.index]
        if self.gate is not None:
            torch.cuda.current_stream(dev).wait_event(self.gate)
            self.waited = True


class _ModPrepGradPort(torch.autograd.Function):
    """Gradient port of the head's modulated weights.  forward: no launch — one handle per layer, a stride-0 zero shaped like
    the per-image weights (B, in, out), which InrHeadX3Function takes as an input and answers with dL/dWb; backward: the
    modulation / demodulation backward of all layers (mod_conv_fc.py:392-496) -> (dW, ds) per layer.  The node lives on the
    stream that is current when apply() is called: CIPSNet.forward calls it under the generator's side stream."""

    @staticmethod
    def forward(ctx, ports, B, *ws):
        ctx.ports = weakref.ref(ports)
        ctx.ws = tuple(_c(t.detach()) for t in ws)
        z = _zero_handle(ws[0].device)
        return tuple(z.expand(B, ws[2 * i].shape[0], ws[2 * i].shape[1]) for i in range(len(ws) // 2))

    @staticmethod
    def backward(ctx, *gwb):
        ports = ctx.ports()
        ports.wait(gwb[0].device)
        layers = [(ctx.ws[2 * i], ctx.ws[2 * i + 1], ports.demod[i], _c(gwb[i])) for i in range(len(gwb))]
        res = modfc_prep_bwd_batch(layers, cores=True)
        return (None, None) + tuple(t for pair in res for t in pair)


class _ToRGBGradPort(torch.autograd.Function):
    """Gradient port of the ToRGB taps: forward returns a stride-0 zero shaped like the head's output (its gradient IS drgb),
    backward computes every tap's weight / bias gradient from the block outputs the head kept (TailPorts.taps)."""

    @staticmethod
    def forward(ctx, ports, shape, *rgbp):
        ctx.ports = weakref.ref(ports)
        return _zero_handle(rgbp[0].device).expand(shape)

    @staticmethod
    def backward(ctx, drgb):
        ports = ctx.ports()
        ports.wait(drgb.device)
        drgb2 = _c(drgb).reshape(-1, 3)
        out = []
        for dT, dtau in torgb_bwd_w_x3_batch(ports.taps, drgb2, cores=True):
            out += [dT, dtau]
        return (None, None) + tuple(out)


_ZERO_HANDLE = {}


def _zero_handle(dev):
    """one cached zero element per device (never written): the storage behind every port handle.  Not cached under a graph
    capture (a tensor made inside a capture lives in the graph's pool)."""
    if torch.cuda.is_current_stream_capturing():
        return torch.zeros(1, device=dev)
    z = _ZERO_HANDLE.get(dev)
    if z is None:
        z = _ZERO_HANDLE[dev] = torch.zeros(1, device=dev)
    return z


# The ports' tail must not start while the compositing backward (HBM-bound, on the critical path) is running: it would share the
# bandwidth and delay it by as much as the tail gains.  The head's backward arms the gate of its device with its TailPorts; a
# compositing backward that runs while a gate is armed records an event right after its launch into them (the last one wins).
# The ports' backward nodes — which the engine runs AFTER it when the ports were opened before the ray march in the forward pass
# (lower sequence numbers; GeneratorNerfINR._render does that) — disarm the gate and make their stream wait for that event.  No
# event (no compositing backward, ports opened late): the tail starts as soon as the head's backward is done.
_TAIL_GATE = {}        # device index -> the armed TailPorts


def _tail_gate_publish(dev):
    ports = _TAIL_GATE.get(dev.index)
    if ports is not None:
        ports.gate = torch.cuda.Event()
        ports.gate.record(torch.cuda.current_stream(dev))


def inr_head_ports_ok(nblocks, B, n, in0, params, dev):
    """the gradient-port form applies: split-bf16 head in training, batch within the co-resident kernels' limit, ToRGB taps present"""
    return (INR_TAIL == "side" and INR_MODE in ("bf16x3", "bf16") and torch.device(dev).type == "cuda" and torch.is_grad_enabled()
            and nblocks > 3 and n % 32 == 0 and in0 % 32 == 0 and B <= 64 and any(t.requires_grad for t in params))


def inr_head_open_ports(nblocks, B, n, params, side):
    """the two gradient ports of one head evaluation (see INR_TAIL), their autograd nodes on `side` -> TailPorts"""
    ports = TailPorts()
    ws, rgbp = params[:4 * nblocks], params[4 * nblocks:]
    dev = params[0].device
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        handles = _ModPrepGradPort.apply(ports, B, *ws)
        ports.handles = handles + (_ToRGBGradPort.apply(ports, (B, n, 3), *rgbp),)
    return ports


def inr_head_with_ports(nblocks, x0, params, ports):
    """inr_head with the weight-gradient tail behind the gradient ports `ports` = inr_head_open_ports(...)"""
    det = [t.detach() for t in params]
    return InrHeadX3Function.apply(nblocks, True, ports, x0, *det, *ports.handles)


def inr_head(nblocks, x0, *params):
    # the split-bf16 kernels (both pass counts) tile pixels and features by 32; anything else (part_grad_forward with an
    # arbitrary grad_points, generator.py:1591-1593) runs on the exact fp32 MFMA path, which has no such granule
    x3 = INR_MODE in ("bf16x3", "bf16") and x0.shape[1] % 32 == 0 and x0.shape[2] % 32 == 0
    fn = InrHeadX3Function if x3 else InrHeadFunction
    # the caller's grad mode: under torch.no_grad() nothing is kept for a backward
    return fn.apply(nblocks, torch.is_grad_enabled(), None, x0, *params)


# --------------------------------------------------------------------------------------
# H5 discriminator native ops (same contracts as the reference's pybind ops)
# --------------------------------------------------------------------------------------
_FLOATS = (torch.float32, torch.float16, torch.bfloat16, torch.float64)


def _native_in(t, what):
    """The reference's ops dispatch fp16 / fp32 / fp64 (fused_bias_act_kernel.cu:79, upfirdn2d_kernel.cu:177-211); the
    HIP kernels compute in fp32: other float dtypes make an fp32 round trip (the result is cast back to the INPUT's
    dtype by the caller), anything else is an error."""
    if not t.is_cuda:
        raise RuntimeError(f"{what} must be a CUDA tensor")      # CHECK_CUDA, fused_bias_act.cpp:13
    if t.dtype not in _FLOATS:
        raise RuntimeError(f"{what}: unsupported dtype {t.dtype} (floating point expected)")
    return t.contiguous().float()


def fused_bias_act(input, bias, refer, act, grad, alpha, scale):
    """fused.fused_bias_act(input, bias, refer, act, grad, alpha, scale) -> Tensor of input's dtype and shape
    (exp/comm/op/fused_bias_act.cpp:11-21).  Empty tensor = absent."""
    lib = _lib.load()
    x = _native_in(input, "input")
    b = _native_in(bias, "bias") if (bias is not None and bias.numel()) else None
    r = _native_in(refer, "refer") if (refer is not None and refer.numel()) else None
    if r is not None and r.numel() != x.numel():
        raise RuntimeError("refer must have input's number of elements")
    y = torch.empty_like(x)
    step_b = 1
    for i in range(2, x.dim()):
        step_b *= x.size(i)
    size_b = b.numel() if b is not None else 0
    with torch.cuda.device(x.device):
        check(lib.cips_fused_bias_act(_p(x), _p(b), _p(r), _p(y), x.numel(), size_b, step_b, act, grad, float(alpha),
                                      float(scale), _stream()), "cips_fused_bias_act")
    return y if input.dtype == torch.float32 else y.to(input.dtype)


def lrelu_bwd_bias(grad, refer, alpha, scale):
    """grad, refer (B, C, H, W) fp32 contiguous -> (grad_input, grad_bias (C)): FusedLeakyReLUFunctionBackward.forward
    (exp/comm/op/fused_act.py:26-44: fused_bias_act(grad, empty, out, 3, 1, slope, scale) then grad_input.sum(0, 2, 3)) with
    the bias gradient accumulated in the same pass"""
    lib = _lib.load()
    B, C = grad.shape[0], grad.shape[1]
    hw = grad.numel() // (B * C)
    S = lib.cips_lrelu_bwd_bias_slices(hw)
    gin = torch.empty_like(grad)
    part = torch.empty(B, C, S, device=grad.device)
    with torch.cuda.device(grad.device):
        check(lib.cips_lrelu_bwd_bias(_p(grad), _p(refer), _p(gin), _p(part), B * C, hw, float(alpha), float(scale), _stream()),
              "cips_lrelu_bwd_bias")
        gb = torch.empty(C, device=grad.device)
        check(lib.cips_lrelu_bwd_bias_finish(_p(part), _p(gb), B, C, S, _stream()), "cips_lrelu_bwd_bias_finish")
    return gin, gb


def lrelu_bwd_bias_nhwc(grad, refer, alpha, scale):
    """lrelu_bwd_bias with the gated gradient written as NHWC split planes only (cips_lrelu_bwd_bias_nhwc) -> (Planes, grad_bias)"""
    lib = _lib.load()
    B, C, H, W = grad.shape
    hw = H * W
    S = lib.cips_lrelu_bwd_bias_nhwc_tiles(hw)
    hi = torch.empty(B * hw + 1, C, device=grad.device, dtype=BF)
    lo = torch.empty(B * hw + 1, C, device=grad.device, dtype=BF)
    part = torch.empty(B, C, S, device=grad.device)
    gb = torch.empty(C, device=grad.device)
    with torch.cuda.device(grad.device):
        check(lib.cips_lrelu_bwd_bias_nhwc(_p(grad), _p(refer), _p(hi), _p(lo), _p(part), B, C, hw, float(alpha), float(scale), _stream()),
              "cips_lrelu_bwd_bias_nhwc")
        check(lib.cips_lrelu_bwd_bias_finish(_p(part), _p(gb), B, C, S, _stream()), "cips_lrelu_bwd_bias_finish")
    return Planes(hi, lo), gb


def upfirdn2d_op(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """upfirdn2d_op.upfirdn2d(input[N,H,W,minor], kernel, ...) -> Tensor of input's dtype
    (exp/comm/op/upfirdn2d.cpp:12-23)."""
    lib = _lib.load()
    x = _native_in(input, "input")
    k = _native_in(kernel, "kernel")
    major, in_h, in_w, minor = x.shape
    kh, kw = k.shape
    out_h = (in_h * up_y + pad_y0 + pad_y1 - kh) // down_y + 1
    out_w = (in_w * up_x + pad_x0 + pad_x1 - kw) // down_x + 1
    out = torch.empty(major, out_h, out_w, minor, device=x.device)
    with torch.cuda.device(x.device):
        check(lib.cips_upfirdn2d(_p(x), _p(k), _p(out), major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y,
                                 pad_x0, pad_x1, pad_y0, pad_y1, _stream()), "cips_upfirdn2d")
    return out if input.dtype == torch.float32 else out.to(input.dtype)


# cips_upfirdn2d_form's codes (CIPS_UPFIRDN2D_* of include/cips3d_hip.h), by kernel instantiation
UPFIRDN2D_FORMS = ("none", "generic", "direct<1,8>", "direct<1,16>", "direct<2,8>", "direct<2,16>", "up2<4>", "down2_pairs<4>",
                   "down2_pairs<8>", "up2_pairs<2>", "up2_pairs<4>", "blur<1>", "blur<2>", "blur_spill")


def upfirdn2d_form(in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """the kernel instantiation upfirdn2d_op runs for these arguments, as a name of UPFIRDN2D_FORMS (host only: no GPU needed);
    ValueError for arguments the op refuses"""
    code = _lib.load().cips_upfirdn2d_form(in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
    if code < 0:
        raise ValueError("cips_upfirdn2d refuses these arguments (more than 64 taps, or an up / down factor below 1)")
    return UPFIRDN2D_FORMS[code]


def im2col(x, kh, kw, stride, pad):
    lib = _lib.load()
    B, Cc, H, W = x.shape
    Ho = (H + 2 * pad - kh) // stride + 1
    Wo = (W + 2 * pad - kw) // stride + 1
    col = torch.empty(B, Cc * kh * kw, Ho * Wo, device=x.device)
    check(lib.cips_im2col(_p(x), _p(col), B, Cc, H, W, kh, kw, stride, pad, _stream()), "cips_im2col")
    return col, Ho, Wo


def col2im(col, B, Cc, H, W, kh, kw, stride, pad):
    lib = _lib.load()
    dx = torch.empty(B, Cc, H, W, device=col.device)
    check(lib.cips_col2im(_p(col), _p(dx), B, Cc, H, W, kh, kw, stride, pad, _stream()), "cips_col2im")
    return dx


# --------------------------------------------------------------------------------------
# Pyramid fit loss (csrc/fit_loss.hip): the loss of the projection loop
# --------------------------------------------------------------------------------------
FIT_LOSS_KINDS = ("mse", "charbonnier")


class PyramidLossFunction(torch.autograd.Function):
    """(pred, target, weight or None) -> loss (b,): cips_pyramid_loss_fwd writes the loss and d loss / d pred in one pass; the
    backward scales that stored gradient by the upstream value of each image (one launch, nothing recomputed)."""

    @staticmethod
    def forward(ctx, pred, target, weight, level_weights, kind, eps):
        lib = _lib.load()
        b, Cc, H, W = pred.shape
        L = len(level_weights)
        loss = torch.empty(b, device=pred.device)
        grad = torch.empty_like(pred)
        nscr = lib.cips_pyramid_loss_scratch(b, Cc, H, W, L)
        scratch = torch.empty(max(nscr, 1), device=pred.device)
        lw = (C.c_double * L)(*level_weights)
        check(lib.cips_pyramid_loss_fwd(_p(pred), _p(target), _p(weight), lw, L, kind, eps, _p(loss), _p(grad), _p(scratch),
                                        nscr, b, Cc, H, W, _stream()), "cips_pyramid_loss_fwd")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        grad, = ctx.saved_tensors
        dloss = _c(dloss)
        out = torch.empty_like(grad)
        check(_lib.load().cips_pyramid_loss_bwd(_p(grad), _p(dloss), _p(out), grad.shape[0], grad[0].numel(), _stream()),
              "cips_pyramid_loss_bwd")
        return out, None, None, None, None, None


def pyramid_loss(pred, target, weight=None, level_weights=(1.,), kind="mse", eps=1e-3):
    """Per-image multi-scale fit loss -> (b,), differentiable with respect to `pred` only.
    pred, target (b,C,H,W); weight (b,1,H,W) or None (= 1).  With d_0 = pred - target, w_0 = weight and level l+1 the 2x2 mean
    of level l (of both),   loss_b = sum_l level_weights[l] / (C H_l W_l) * sum_{c,y,x} w_l rho(d_l),
    rho(x) = x^2 (kind "mse") or sqrt(x^2 + eps^2) - eps ("charbonnier").  1 <= len(level_weights) <= 8, H and W multiples of
    2^(levels - 1).  level_weights=(1.,), "mse", no weight: nn.MSELoss per image (the reference Projector's loss).
    Deterministic: fixed summation order, no atomics; an image's result does not depend on its batch."""
    level_weights = tuple(float(v) for v in level_weights)
    L = len(level_weights)
    if kind not in FIT_LOSS_KINDS:
        raise ValueError(f"pyramid_loss: kind {kind!r} (one of {FIT_LOSS_KINDS})")
    if not 1 <= L <= 8 or any(not math.isfinite(v) or v < 0 for v in level_weights):
        raise ValueError("pyramid_loss: 1 to 8 finite, non-negative level weights")
    if pred.dim() != 4 or pred.shape != target.shape or pred.numel() == 0:
        raise ValueError(f"pyramid_loss: pred and target (b,C,H,W) of one shape, got {tuple(pred.shape)} and {tuple(target.shape)}")
    b, Cc, H, W = pred.shape
    if H % (1 << (L - 1)) or W % (1 << (L - 1)):
        raise ValueError(f"pyramid_loss: {L} levels need H and W to be multiples of {1 << (L - 1)}, got {H} x {W}")
    if weight is not None and tuple(weight.shape) != (b, 1, H, W):
        raise ValueError(f"pyramid_loss: weight ({b},1,{H},{W}) expected, got {tuple(weight.shape)}")
    if kind == "charbonnier" and not eps > 0:
        raise ValueError("pyramid_loss: charbonnier needs eps > 0")
    for t in (pred, target, weight):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise RuntimeError("pyramid_loss needs fp32 tensors on the GPU (no CPU fallback)")
    target = target.detach().contiguous()
    weight = weight.detach().contiguous() if weight is not None else None
    _chk(target, weight)
    return PyramidLossFunction.apply(pred.contiguous(), target, weight, level_weights, FIT_LOSS_KINDS.index(kind), float(eps))


# --------------------------------------------------------------------------------------
# View reprojection (csrc/reproject.hip): a source view seen through a target view's depth
# --------------------------------------------------------------------------------------
class ReprojectFunction(torch.autograd.Function):
    """(src, tgt_depth, tgt2src, src_depth or None) -> out, mask, uv or None: cips_reproject_fwd, one launch.  mask and uv are
    not differentiable.  The backward is cips_reproject_bwd on the stored mask: d tgt_depth always (a gather, reproducible);
    d src only where src needs a gradient — its buffer is zeroed and summed with fp32 atomic adds, the one result whose last
    bits can differ from call to call; without it neither the memset nor the adds run."""

    @staticmethod
    def forward(ctx, src, tgt_depth, tgt2src, src_depth, zc_tgt, zc_src, occ_tol, return_uv):
        lib = _lib.load()
        B, Cc, Hs, Ws = src.shape
        Ht, Wt = tgt_depth.shape[2:]
        out = torch.empty(B, Cc, Ht, Wt, device=src.device)
        mask = torch.empty(B, 1, Ht, Wt, dtype=torch.uint8, device=src.device)
        uv = torch.empty(B, 2, Ht, Wt, device=src.device) if return_uv else None
        check(lib.cips_reproject_fwd(_p(src), _p(src_depth), _p(tgt_depth), _p(tgt2src), zc_tgt, zc_src, occ_tol, _p(out),
                                     _p(mask), _p(uv), B, Cc, Hs, Ws, Ht, Wt, _stream()), "cips_reproject_fwd")
        ctx.save_for_backward(src, tgt_depth, tgt2src, mask)
        ctx.zc = (zc_tgt, zc_src)
        ctx.mark_non_differentiable(mask)
        if uv is not None:
            ctx.mark_non_differentiable(uv)
        return out, mask, uv

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, dmask, duv):
        src, tgt_depth, tgt2src, mask = ctx.saved_tensors
        B, Cc, Hs, Ws = src.shape
        Ht, Wt = tgt_depth.shape[2:]
        dout = _c(dout)
        d_src = torch.empty_like(src) if ctx.needs_input_grad[0] else None          # zeroed by the entry point
        d_depth = torch.empty_like(tgt_depth) if ctx.needs_input_grad[1] else None
        check(_lib.load().cips_reproject_bwd(_p(dout), _p(src), _p(tgt_depth), _p(tgt2src), _p(mask), ctx.zc[0], ctx.zc[1],
                                             _p(d_src), _p(d_depth), B, Cc, Hs, Ws, Ht, Wt, _stream()), "cips_reproject_bwd")
        return d_src, d_depth, None, None, None, None, None, None


def reproject(src, tgt_depth, tgt2src, zc_tgt, zc_src=None, src_depth=None, occ_tol=None, return_uv=False):
    """The source view `src` as the target view's pixels see it -> (out, mask) or, with return_uv, (out, mask, uv).
    src (b,C,Hs,Ws); tgt_depth (b,1,Ht,Wt), the target's depth along the normalised ray (render().depth, geometry().depth);
    tgt2src (b,3,4), a rigid transform from target-camera to source-camera space (evaluation.relative_pose); zc_tgt, zc_src
    (default zc_tgt): the two cameras' image-plane constants, generator._zc(fov); src_depth (b,1,Hs,Ws) with occ_tol >= 0: the
    occlusion test — a pixel whose point lies more than occ_tol behind the source's own depth there is occluded.
      out  (b,C,Ht,Wt)        the bilinear sample of src where mask == 1, exact zeros elsewhere
      mask (b,1,Ht,Wt) uint8  1 visible, 0 not in the source's frame (or no valid depth), 2 in frame but occluded
      uv   (b,2,Ht,Wt)        the source pixel coordinates (column u, row v) every target pixel lands on, NaN where mask == 0
    The definition, step by step: include/cips3d_hip.h (cips_reproject_fwd).  Differentiable with respect to src and tgt_depth
    where mask == 1, zero elsewhere; nothing flows through mask, uv, src_depth, tgt2src or the plane constants, and there is no
    double backward.  out, mask, uv and the gradient of tgt_depth are bit-reproducible; the gradient of src is a sum of fp32
    atomic adds, whose last bits can differ from call to call (it is not computed when src needs no gradient)."""
    if src.dim() != 4 or src.numel() == 0 or src.shape[2] < 2 or src.shape[3] < 2:
        raise ValueError(f"reproject: src (b,C,Hs,Ws) with Hs, Ws >= 2 expected, got {tuple(src.shape)}")
    b, Cc, Hs, Ws = src.shape
    if tgt_depth.dim() != 4 or tgt_depth.shape[1] != 1 or tgt_depth.shape[2] < 2 or tgt_depth.shape[3] < 2:
        raise ValueError(f"reproject: tgt_depth (b,1,Ht,Wt) with Ht, Wt >= 2 expected, got {tuple(tgt_depth.shape)}")
    if tgt_depth.shape[0] != b or tuple(tgt2src.shape) != (b, 3, 4):
        raise ValueError(f"reproject: batch {b} of src needs tgt_depth ({b},1,Ht,Wt) and tgt2src ({b},3,4), got "
                         f"{tuple(tgt_depth.shape)} and {tuple(tgt2src.shape)}")
    if src_depth is not None and tuple(src_depth.shape) != (b, 1, Hs, Ws):
        raise ValueError(f"reproject: src_depth ({b},1,{Hs},{Ws}) expected, got {tuple(src_depth.shape)}")
    if src_depth is not None and occ_tol is None:
        raise ValueError("reproject: src_depth needs an occ_tol (>= 0, in units of depth)")
    zc_tgt = float(zc_tgt)
    zc_src = zc_tgt if zc_src is None else float(zc_src)
    occ_tol = 0. if occ_tol is None else float(occ_tol)
    if not (math.isfinite(zc_tgt) and math.isfinite(zc_src) and zc_tgt != 0 and zc_src != 0):
        raise ValueError(f"reproject: zc_tgt and zc_src must be finite and non-zero, got {zc_tgt} and {zc_src}")
    if not (math.isfinite(occ_tol) and occ_tol >= 0):
        raise ValueError(f"reproject: occ_tol must be finite and >= 0, got {occ_tol}")
    for t in (src, tgt_depth, tgt2src, src_depth):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32):
            raise ValueError("reproject needs fp32 tensors on the GPU (no CPU fallback)")
    tgt2src = tgt2src.detach().contiguous()
    src_depth = src_depth.detach().contiguous() if src_depth is not None else None
    src, tgt_depth = src.contiguous(), tgt_depth.contiguous()
    _chk(src, tgt_depth, tgt2src, src_depth)
    out, mask, uv = ReprojectFunction.apply(src, tgt_depth, tgt2src, src_depth, zc_tgt, zc_src, occ_tol, bool(return_uv))
    return (out, mask, uv) if return_uv else (out, mask)


# --------------------------------------------------------------------------------------
# Mesh rasterisation (csrc/raster.hip): an indexed triangle mesh seen through the camera of the ray set-up
# --------------------------------------------------------------------------------------
RASTER_CULL = {None: 0, 'back': 1}


def _raster_tensor(who, t, name, dtype, shape):
    """one argument of the rasteriser: dtype and shape as the entry points want them (shape: None matches any size)"""
    if not torch.is_tensor(t) or t.dtype != dtype:
        raise ValueError(f"{who}: {name} must be a {str(dtype).replace('torch.', '')} tensor")
    if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
        raise ValueError(f"{who}: {name} {tuple('*' if s is None else s for s in shape)} expected, got {tuple(t.shape)}")
    return t.detach().contiguous()


def _raster_on_gpu(who, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise ValueError(f"{who} needs tensors on the GPU (no CPU fallback)")
    _chk(*tensors)


def rasterize(vertices, faces, world2cam, zc, H, W, near=1e-4, far=float('inf'), cull=None):
    """One indexed triangle mesh seen from b cameras -> (face, bary, depth, mask): per pixel the first triangle the pixel's
    ray hits and where.  vertices (V,3) fp32, faces (T,3) int32, world2cam (b,3,4) fp32 = [R | t], the inverse of cam2world
    (evaluation.world2cam composes it in fp64), zc = generator._zc(fov) < 0, H, W >= 2; the camera is the one of the ray set-up
    (pixel_grids' xg, yg).
      face  (b,H,W) int32    the winning triangle, -1 where the ray meets none
      bary  (b,H,W,3)        its perspective-correct barycentrics (raster_interpolate takes them), zeros for none
      depth (b,H,W)          the distance along the unit ray — surface().depth's and render().depth's quantity; `far` for none
      mask  (b,H,W) uint8    1 / 0
    near: a triangle with a vertex closer than that (or behind the camera) is dropped whole, there is no clipping.  cull:
    None or 'back' (drop triangles whose geometric normal points away from the camera; extract_mesh winds towards lower
    density).  The rule, decision by decision: include/cips3d_hip.h (cips_raster_fwd).  Forward only: nothing here has a
    gradient.  Every output is bit-reproducible, whatever the order of the triangles; no host synchronisation."""
    who = "rasterize"
    if cull not in RASTER_CULL:
        raise ValueError(f"{who}: cull must be None or 'back', got {cull!r}")
    H, W, zc, near, far = int(H), int(W), float(zc), float(near), float(far)
    if H < 2 or W < 2:
        raise ValueError(f"{who}: H, W >= 2 expected, got {H} x {W}")
    if not (math.isfinite(zc) and zc < 0):
        raise ValueError(f"{who}: zc must be finite and negative, got {zc}")
    if not (math.isfinite(near) and near > 0):
        raise ValueError(f"{who}: near must be finite and positive, got {near}")
    if math.isnan(far):
        raise ValueError(f"{who}: far must not be NaN")
    vertices = _raster_tensor(who, vertices, "vertices", torch.float32, (None, 3))
    faces = _raster_tensor(who, faces, "faces", torch.int32, (None, 3))
    world2cam = _raster_tensor(who, world2cam, "world2cam", torch.float32, (None, 3, 4))
    B, V, T = world2cam.shape[0], vertices.shape[0], faces.shape[0]
    if max(B * H * W, B * V, B * T) > 0x7fffffff:
        raise ValueError(f"{who}: b*H*W, b*V and b*T must fit in int32, got b = {B}, H x W = {H} x {W}, V = {V}, T = {T}")
    _raster_on_gpu(who, vertices, faces, world2cam)
    dev = vertices.device
    xg, yg, _ = pixel_grids(W, H, 2, 0., 1., dev)
    face = torch.empty(B, H, W, dtype=torch.int32, device=dev)
    bary = torch.empty(B, H, W, 3, device=dev)
    depth = torch.empty(B, H, W, device=dev)
    mask = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    if B == 0:
        return face, bary, depth, mask
    # scratch: written by the entry point before it is read
    screen = torch.empty(max(B * V, 1), 4, device=dev)
    keys = torch.empty(B * H * W, dtype=torch.int64, device=dev)
    big = torch.empty(max(B * T, 1) + 1, dtype=torch.int32, device=dev)           # the list, then its counter
    check(_lib.load().cips_raster_fwd(_p(vertices) if V else None, _p(faces) if T else None, _p(world2cam), _p(xg), _p(yg), zc,
                                      near, far, RASTER_CULL[cull], _p(screen), _p(keys), _p(big), _p(big[-1:]), B * T, _p(face),
                                      _p(bary), _p(depth), _p(mask), B, V, T, H, W, _stream()), "cips_raster_fwd")
    return face, bary, depth, mask


def raster_interpolate(face, bary, faces, attr, fill=0.):
    """A per-vertex attribute attr (V,C) fp32 over rasterize's (face (b,H,W) int32, bary (b,H,W,3)) and the mesh's faces (T,3)
    int32 -> (b,C,H,W): sum_i bary_i * attr[faces[face][i]] where a triangle was hit, `fill` elsewhere.  Any C >= 1.  Forward
    only, bit-reproducible, no host synchronisation."""
    who = "raster_interpolate"
    face = _raster_tensor(who, face, "face", torch.int32, (None, None, None))
    B, H, W = face.shape
    bary = _raster_tensor(who, bary, "bary", torch.float32, (B, H, W, 3))
    faces = _raster_tensor(who, faces, "faces", torch.int32, (None, 3))
    attr = _raster_tensor(who, attr, "attr", torch.float32, (None, None))
    V, Cc = attr.shape
    if Cc < 1:
        raise ValueError(f"{who}: attr (V,C) with C >= 1 expected, got {tuple(attr.shape)}")
    if H < 2 or W < 2 or B * H * W > 0x7fffffff:
        raise ValueError(f"{who}: face (b,H,W) with H, W >= 2 and b*H*W within int32 expected, got {tuple(face.shape)}")
    _raster_on_gpu(who, face, bary, faces, attr)
    out = torch.empty(B, Cc, H, W, device=face.device)
    if B == 0:
        return out
    T = faces.shape[0]
    check(_lib.load().cips_raster_interp(_p(face), _p(bary), _p(faces) if T else None, _p(attr) if V else None, float(fill), _p(out),
                                         B, H, W, T, V, Cc, _stream()), "cips_raster_interp")
    return out


# --------------------------------------------------------------------------------------
# Baked radiance volumes (csrc/volume.hip): sigma and colour on a lattice, volume-rendered without the network
# --------------------------------------------------------------------------------------
VOLUME_BRICK = 8          # cells per axis of one occupancy brick


def _volume_box(who, lo, hi):
    try:
        lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: lo and hi must be three numbers each") from None
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError(f"{who}: lo and hi must be three numbers each, got {len(lo)} and {len(hi)}")
    if not all(math.isfinite(v) for v in lo + hi) or not all(h > l for l, h in zip(lo, hi)):
        raise ValueError(f"{who}: a finite box with hi > lo on every axis expected, got lo = {lo}, hi = {hi}")
    return (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)


def bake_volume(sigma, rgb):
    """sigma (Bv,nx,ny,nz) and rgb (Bv,nx,ny,nz,3), fp32 on the GPU (density_grid's and color_grid's layout) -> (packed, occ):
      packed (Bv,nx,ny,nz,4)  r, g, b, sigma per node, bits copied: one 16-byte record, what render_volume gathers
      occ    (Bv, ceil((nx-1)/8), ceil((ny-1)/8), ceil((nz-1)/8))  per brick of 8 x 8 x 8 cells the maximum of sigma over every
             node a trilinear lookup inside the brick can read (nodes 8I .. min(8I+8, nx-1) per axis): render_volume's
             empty-space skip reads it.  Exact.
    The volume is taken to be finite.  The rule: include/cips3d_hip.h (cips_volume_bake).  No host synchronisation."""
    who = "bake_volume"
    sigma = _raster_tensor(who, sigma, "sigma", torch.float32, (None, None, None, None))
    Bv, nx, ny, nz = sigma.shape
    rgb = _raster_tensor(who, rgb, "rgb", torch.float32, (Bv, nx, ny, nz, 3))
    if min(nx, ny, nz) < 2 or nx * ny * nz > 0x7fffffff:
        raise ValueError(f"{who}: a lattice of at least 2 nodes per axis and at most 2^31 - 1 nodes expected, got {nx} x {ny} x {nz}")
    _raster_on_gpu(who, sigma, rgb)
    dev = sigma.device
    packed = torch.empty(Bv, nx, ny, nz, 4, device=dev)
    occ = torch.empty(Bv, *(-(-(n - 1) // VOLUME_BRICK) for n in (nx, ny, nz)), device=dev)
    if Bv:
        check(_lib.load().cips_volume_bake(_p(sigma), _p(rgb), _p(packed), _p(occ), Bv, nx, ny, nz, _stream()), "cips_volume_bake")
    return packed, occ


def volume_occupancy(packed):
    """bake_volume's occ for a packed volume (Bv,nx,ny,nz,4) whose nodes have moved: the brick maxima of packed[..., 3], the same
    bits bake_volume returns for the same sigma (one launch, sigma read in place).  fit_volume refreshes the occupancy with it
    before every forward, so that render_volume's skip stays exact while sigma moves.  No gradient, no host synchronisation."""
    who = "volume_occupancy"
    packed = _raster_tensor(who, packed, "packed", torch.float32, (None, None, None, None, 4))
    Bv, nx, ny, nz = packed.shape[:4]
    if min(nx, ny, nz) < 2 or nx * ny * nz > 0x7fffffff:
        raise ValueError(f"{who}: a lattice of at least 2 nodes per axis and at most 2^31 - 1 nodes expected, got {nx} x {ny} x {nz}")
    _raster_on_gpu(who, packed)
    if packed.data_ptr() % 16:
        raise ValueError(f"{who}: packed must be 16-byte aligned")
    occ = torch.empty(Bv, *(-(-(n - 1) // VOLUME_BRICK) for n in (nx, ny, nz)), device=packed.device)
    if Bv:
        check(_lib.load().cips_volume_occupancy(_p(packed), _p(occ), Bv, nx, ny, nz, _stream()), "cips_volume_occupancy")
    return occ


def _volume_render_launch(packed, occ, lo_c, hi_c, xg, yg, zg, cam2world, zc, clamp, flags, H, W):
    b, dev = cam2world.shape[0], packed.device
    Bv, nx, ny, nz = packed.shape[:4]
    rgb = torch.empty(b, 3, H, W, device=dev)
    depth = torch.empty(b, 1, H, W, device=dev)
    opacity = torch.empty(b, 1, H, W, device=dev)
    check(_lib.load().cips_volume_render(_p(packed), _p(occ), lo_c, hi_c, _p(xg), _p(yg), _p(zg), _p(cam2world), zc, clamp, flags,
                                         _p(rgb), _p(depth), _p(opacity), b, Bv, nx, ny, nz, H, W, zg.shape[0], _stream()),
          "cips_volume_render")
    return rgb, depth, opacity


VOLUME_SCATTER_PER_LANE = False      # scripts/bench_volume_backward.py measures both shapes of the backward's atomic adds


class VolumeRenderFunction(torch.autograd.Function):
    """packed, cam2world -> rgb, depth, opacity: cips_volume_render, the launch render_volume makes without autograd; the
    backward is cips_volume_render_bwd (the nodes) and / or cips_volume_render_bwd_cam (the cameras) on the saved volume,
    occupancy, cameras and depths: only what needs_input_grad asks for is launched.  An output nothing was computed from
    arrives as None and is passed as NULL.  Only packed and cam2world have a gradient."""

    @staticmethod
    def forward(ctx, packed, occ, cam2world, zg, xg, yg, lo_c, hi_c, zc, clamp, flags, H, W):
        out = _volume_render_launch(packed, occ, lo_c, hi_c, xg, yg, zg, cam2world, zc, clamp, flags, H, W)
        ctx.save_for_backward(packed, occ, cam2world, zg, xg, yg)
        ctx.consts = (lo_c, hi_c, zc, clamp, flags, H, W)
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, drgb, ddepth, dopacity):
        packed, occ, cam2world, zg, xg, yg = ctx.saved_tensors
        lo_c, hi_c, zc, clamp, flags, H, W = ctx.consts
        lib = _lib.load()
        b, S = cam2world.shape[0], zg.shape[0]
        Bv, nx, ny, nz = packed.shape[:4]
        drgb, ddepth, dopacity = _c(drgb), _c(ddepth), _c(dopacity)
        if drgb is None:
            drgb = torch.zeros(b, 3, H, W, device=packed.device)
        dpacked = dcam = None
        if ctx.needs_input_grad[0]:
            dpacked = torch.empty_like(packed)                                      # zeroed by the entry point
            scratch = torch.empty(max(lib.cips_volume_render_bwd_scratch(b, H, W, S) // 4, 4), device=packed.device)
            check(lib.cips_volume_render_bwd(_p(packed), _p(occ), lo_c, hi_c, _p(xg), _p(yg), _p(zg), _p(cam2world), zc, clamp,
                                             flags | (8 if VOLUME_SCATTER_PER_LANE else 0), _p(drgb), _p(ddepth), _p(dopacity),
                                             _p(dpacked), _p(scratch), b, Bv, nx, ny, nz, H, W, S, _stream()),
                  "cips_volume_render_bwd")
        if ctx.needs_input_grad[2]:
            dcam = torch.empty_like(cam2world)                                      # fully written: no memset, no atomics
            scratch = torch.empty(max(lib.cips_volume_render_bwd_cam_scratch(b, H, W, S) // 4, 4), device=packed.device)
            check(lib.cips_volume_render_bwd_cam(_p(packed), _p(occ), lo_c, hi_c, _p(xg), _p(yg), _p(zg), _p(cam2world), zc,
                                                 clamp, flags, _p(drgb), _p(ddepth), _p(dopacity), _p(dcam), _p(scratch), b, Bv,
                                                 nx, ny, nz, H, W, S, _stream()),
                  "cips_volume_render_bwd_cam")
        return (dpacked, None, dcam) + (None,) * 10


def _volume_render_args(who, volume, aligned, occ, lo, hi, cam2world, zc, H, W, zg, ray_start, ray_end, num_steps, clamp_mode, last_back,
                        white_back, skip):
    """The checks and refusals render_volume and render_feature_volume share, in one order.  volume(who) checks the caller's
    own node tensors and returns them as a list, the one that fixes the lattice (Bv, nx, ny, nz, ...) and must be 16-byte
    aligned LAST (`aligned` is its name in that message).  -> SimpleNamespace(volume,
    occ, cam2world, zg, lo_c, hi_c, zc, H, W, b, S, clamp, flags), every tensor detached, contiguous and on the GPU."""
    if clamp_mode not in ('relu', 'softplus'):
        raise ValueError(f"{who}: clamp_mode must be 'relu' or 'softplus', got {clamp_mode!r}")
    skip = bool(skip)
    if skip and clamp_mode == 'softplus':
        raise ValueError(f"{who}: skip=True needs clamp_mode='relu' (softplus(sigma) > 0 everywhere: nothing is empty)")
    H, W, zc = int(H), int(W), float(zc)
    if H < 2 or W < 2:
        raise ValueError(f"{who}: H, W >= 2 expected, got {H} x {W}")
    if not (math.isfinite(zc) and zc < 0):
        raise ValueError(f"{who}: zc must be finite and negative, got {zc}")
    lo_c, hi_c = _volume_box(who, lo, hi)
    nodes = volume(who)
    main = nodes[-1]
    Bv, (nx, ny, nz) = main.shape[0], main.shape[-4:-1]
    cam2world = _raster_tensor(who, cam2world, "cam2world", torch.float32, (None, 4, 4))
    b = cam2world.shape[0]
    if min(nx, ny, nz) < 2 or nx * ny * nz > 0x7fffffff:
        raise ValueError(f"{who}: a lattice of at least 2 nodes per axis and at most 2^31 - 1 nodes expected, got {nx} x {ny} x {nz}")
    if Bv != 1 and Bv != b:
        raise ValueError(f"{who}: one volume or one per camera expected, got {Bv} volumes and {b} cameras")
    if zg is None:
        if ray_start is None or ray_end is None or num_steps is None:
            raise ValueError(f"{who}: give zg, or ray_start, ray_end and num_steps")
        if int(num_steps) < 2:
            raise ValueError(f"{who}: num_steps >= 2 expected, got {num_steps}")
        if not main.is_cuda:
            raise ValueError(f"{who} needs tensors on the GPU (no CPU fallback)")
        zg = pixel_grids(W, H, int(num_steps), ray_start, ray_end, main.device)[2]
    zg = _raster_tensor(who, zg, "zg", torch.float32, (None,))
    S = zg.shape[0]
    if S < 2:
        raise ValueError(f"{who}: at least 2 sample depths expected, got {S}")
    if b * H * W > 0x7fffffff or H * W * S > 0x7fffffff:
        raise ValueError(f"{who}: b*H*W and H*W*S must fit in int32, got b = {b}, H x W = {H} x {W}, S = {S}")
    tensors = list(nodes) + [cam2world, zg]
    if occ is not None or skip:
        if occ is None:
            raise ValueError(f"{who}: skip=True needs occ")
        occ = _raster_tensor(who, occ, "occ", torch.float32, (Bv, *(-(-(n - 1) // VOLUME_BRICK) for n in (nx, ny, nz))))
        tensors.append(occ)
    _raster_on_gpu(who, *tensors)
    if main.data_ptr() % 16:
        raise ValueError(f"{who}: {aligned} must be 16-byte aligned")
    return SimpleNamespace(volume=nodes, occ=occ, cam2world=cam2world, zg=zg, lo_c=lo_c, hi_c=hi_c, zc=zc, H=H, W=W, b=b, S=S,
                           clamp=0 if clamp_mode == 'relu' else 1,
                           flags=(1 if last_back else 0) | (2 if white_back else 0) | (4 if skip else 0))


def render_volume(packed, occ, lo, hi, cam2world, zc, H, W, zg=None, ray_start=None, ray_end=None, num_steps=None,
                  clamp_mode='relu', last_back=False, white_back=False, skip=True):
    """A baked volume seen from b cameras -> (rgb (b,3,H,W), depth (b,1,H,W), opacity (b,1,H,W)): trilinear samples of
    bake_volume's packed (Bv,nx,ny,nz,4) along the rays of the ray set-up, composited by forward()'s rule without noise.
    occ: bake_volume's brick occupancy (may be None with skip=False); lo, hi: three numbers each, the box of the lattice (node i
    of axis a at lo[a] + i (hi[a] - lo[a]) / (n_a - 1)); cam2world (b,4,4) fp32; zc = generator._zc(fov) < 0; H, W >= 2.  The
    sample depths are zg (S,) fp32 on the GPU, or linspace(ray_start, ray_end, num_steps) — pixel_grids', the depths forward()
    uses before jitter; S >= 2.  Bv is 1 (every camera sees the one volume) or b.  A sample outside the box contributes nothing.
    clamp_mode 'relu' or 'softplus', last_back, white_back: forward()'s.  opacity is sum w before last_back's top-up.
    skip (relu only; with 'softplus' skip=True is refused, there is no empty space): samples in bricks with occ <= 0 are not
    fetched; the outputs are the same bits with and without.  The rule: include/cips3d_hip.h (cips_volume_render).  The forward
    is bit-reproducible, with or without autograd; no host synchronisation.
    Gradients: when autograd is on and packed or cam2world requires a gradient, the three outputs are differentiable with
    respect to whichever of the two asks (each on its own: the backward launches only what is asked for), and to nothing else:
    zg, lo, hi and zc get none (the sample depths are constants), occ is read as given (it must be the occupancy of packed's
    sigma: volume_occupancy), and there is no double backward.
      packed (the nodes: colours and sigma): with Bv = 1 all b cameras add into the one volume.  A sum of fp32 atomic adds
    (cips_volume_render_bwd), whose last bits can differ from call to call, like reproject's source gradient.
      cam2world (b,4,4): rows 0..2 receive sum_rays [B dir^T | A] with A = sum_k dp_k, B = sum_k z_k dp_k and dp_k the gradient
    with respect to the sample's world position (the slope of the trilinear interpolant in the sample's cell); row 3 is zero.
    No atomics and no memset (cips_volume_render_bwd_cam): the same bits on every call, with skip on or off, and for a camera
    alone or in a batch.  The slope jumps at cell faces and, under relu, where sigma crosses 0.
    Without a gradient request this is the forward launch alone, the same bits."""
    want_grad = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (packed, cam2world))
    packed_in, cam_in = packed, cam2world
    q = _volume_render_args("render_volume", lambda who: [_raster_tensor(who, packed, "packed", torch.float32, (None, None, None, None, 4))],
                            "packed", occ, lo, hi, cam2world, zc, H, W, zg, ray_start, ray_end, num_steps, clamp_mode, last_back, white_back,
                            skip)
    (packed,), occ, cam2world, zg, H, W = q.volume, q.occ, q.cam2world, q.zg, q.H, q.W
    dev = packed.device
    if q.b == 0:
        return torch.empty(0, 3, H, W, device=dev), torch.empty(0, 1, H, W, device=dev), torch.empty(0, 1, H, W, device=dev)
    xg, yg, _ = pixel_grids(W, H, 2, 0., 1., dev)
    lo_c, hi_c, zc, clamp, flags = q.lo_c, q.hi_c, q.zc, q.clamp, q.flags
    if want_grad:
        return VolumeRenderFunction.apply(packed_in.contiguous(), occ, cam_in.contiguous(), zg, xg, yg, lo_c, hi_c, zc, clamp,
                                          flags, H, W)
    return _volume_render_launch(packed, occ, lo_c, hi_c, xg, yg, zg, cam2world, zc, clamp, flags, H, W)


# --------------------------------------------------------------------------------------
# Baked feature volumes (csrc/volume.hip): the SIREN's 32 colour features on the lattice, composited into the head's pixel rows
# --------------------------------------------------------------------------------------
FEATURE_GROUPS = 8        # planes of 4 channels: 32 features


def _feature_lattice(who, sigma):
    sigma = _raster_tensor(who, sigma, "sigma", torch.float32, (None, None, None, None))
    nx, ny, nz = sigma.shape[1:]
    if min(nx, ny, nz) < 2 or nx * ny * nz > 0x7fffffff:
        raise ValueError(f"{who}: a lattice of at least 2 nodes per axis and at most 2^31 - 1 nodes expected, got {nx} x {ny} x {nz}")
    return sigma


def _bake_feature_slab(sigma, rows, planes, occ, x0):
    """x-planes x0 .. of a feature volume: rows (Bv, sx*ny*nz, 32) -> planes[:, :, x0:x0+sx]; the slab that ends the lattice
    writes occ from the whole sigma (cips_feature_volume_bake_slab).  GeneratorNerfINR.bake_features packs slab by slab."""
    Bv, nx, ny, nz = sigma.shape
    sx = rows.shape[1] // (ny * nz)
    if Bv:
        check(_lib.load().cips_feature_volume_bake_slab(_p(sigma), _p(rows), _p(planes), _p(occ), Bv, nx, ny, nz, x0, sx, _stream()),
              "cips_feature_volume_bake_slab")


def feature_volume_buffers(Bv, nx, ny, nz, device):
    """the empty tensors of a feature volume -> sigma (Bv,nx,ny,nz), planes (Bv,8,nx,ny,nz,4), occ (Bv, bricks per axis)"""
    return (torch.empty(Bv, nx, ny, nz, device=device), torch.empty(Bv, FEATURE_GROUPS, nx, ny, nz, 4, device=device),
            torch.empty(Bv, *(-(-(n - 1) // VOLUME_BRICK) for n in (nx, ny, nz)), device=device))


def bake_feature_volume(sigma, feat):
    """sigma (Bv,nx,ny,nz) and feat (Bv,nx,ny,nz,32) or (Bv,nx*ny*nz,32) — NeRFNetwork.evaluate's rows on the lattice, x
    outermost — fp32 on the GPU -> (planes, occ):
      planes (Bv,8,nx,ny,nz,4)  channel-group-major: planes[v, g, i, j, k] holds channels 4g .. 4g+3 of node (i, j, k), bits
             copied; every plane has bake_volume's packed layout, so one group's interpolation is the rgb renderer's gather
      occ    bake_volume's brick occupancy of sigma, the same bits
    sigma itself is the third tensor of the volume; render_feature_volume reads it as it is.  The volume is taken to be finite.
    A volume costs 132 bytes per node with its sigma.  The rule: include/cips3d_hip.h (cips_feature_volume_bake).  No host
    synchronisation, no gradient."""
    who = "bake_feature_volume"
    sigma = _feature_lattice(who, sigma)
    Bv, nx, ny, nz = sigma.shape
    if torch.is_tensor(feat) and feat.dim() == 5:
        feat = _raster_tensor(who, feat, "feat", torch.float32, (Bv, nx, ny, nz, 4 * FEATURE_GROUPS))
    else:
        feat = _raster_tensor(who, feat, "feat", torch.float32, (Bv, nx * ny * nz, 4 * FEATURE_GROUPS))
    _raster_on_gpu(who, sigma, feat)
    if feat.data_ptr() % 16:
        raise ValueError(f"{who}: feat must be 16-byte aligned")
    _, planes, occ = feature_volume_buffers(Bv, nx, ny, nz, sigma.device)
    _bake_feature_slab(sigma, feat.view(Bv, nx * ny * nz, 4 * FEATURE_GROUPS), planes, occ, 0)
    return planes, occ


def render_feature_volume(sigma, planes, occ, lo, hi, cam2world, zc, H, W, zg=None, ray_start=None, ray_end=None, num_steps=None,
                          clamp_mode='relu', last_back=False, white_back=False, skip=True):
    """A baked feature volume seen from b cameras -> (fea (b,H*W,32), depth (b,1,H,W), opacity (b,1,H,W)): what the NeRF stage of
    forward() hands to the INR head, from trilinear samples of the lattice instead of the SIREN.  sigma (Bv,nx,ny,nz), planes
    (Bv,8,nx,ny,nz,4) and occ: bake_feature_volume's; every other argument, every check and refusal: render_volume's (skip=True
    with 'softplus' is refused).  The rule is render_volume's with 32 channels in place of 3, white_back adding 1 - sum w to every
    channel (include/cips3d_hip.h, cips_feature_volume_render); a sample gathers its features only where its weight is not
    zero, which changes no bit.  The outputs are the same bits on every call, with skip on or off.
    Forward only: gradients are not built.  It runs as under no_grad — the outputs carry no grad_fn — and an input that requires
    grad is refused.  No host synchronisation."""
    who = "render_feature_volume"
    for name, t in (("sigma", sigma), ("planes", planes), ("occ", occ), ("cam2world", cam2world), ("zg", zg)):
        if torch.is_tensor(t) and t.requires_grad:
            raise ValueError(f"{who}: {name} requires grad, but gradients are not built for feature volumes (forward only): "
                             f"pass {name}.detach()")

    def volume(who):
        sig = _raster_tensor(who, sigma, "sigma", torch.float32, (None, None, None, None))
        return [sig, _raster_tensor(who, planes, "planes", torch.float32, (sig.shape[0], FEATURE_GROUPS, *sig.shape[1:], 4))]

    q = _volume_render_args(who, volume, "planes", occ, lo, hi, cam2world, zc, H, W, zg, ray_start, ray_end, num_steps, clamp_mode, last_back,
                            white_back, skip)
    (sigma, planes), occ, cam2world, zg, H, W, b, S = q.volume, q.occ, q.cam2world, q.zg, q.H, q.W, q.b, q.S
    Bv, nx, ny, nz = sigma.shape
    dev = planes.device
    fea = torch.empty(b, H * W, 4 * FEATURE_GROUPS, device=dev)
    depth = torch.empty(b, 1, H, W, device=dev)
    opacity = torch.empty(b, 1, H, W, device=dev)
    if b == 0:
        return fea, depth, opacity
    xg, yg, _ = pixel_grids(W, H, 2, 0., 1., dev)
    check(_lib.load().cips_feature_volume_render(_p(sigma), _p(planes), _p(occ), q.lo_c, q.hi_c, _p(xg), _p(yg), _p(zg), _p(cam2world),
                                                 q.zc, q.clamp, q.flags, _p(fea), _p(depth), _p(opacity), b, Bv, nx, ny, nz, H, W, S,
                                                 _stream()), "cips_feature_volume_render")
    return fea, depth, opacity
