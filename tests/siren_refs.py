"""Plain-torch references of the FiLM-SIREN (cips3d_amd.ops.SirenFunction) for the fp64 tests of its kernels: the function in
any dtype, an emulation of the kernels' split operands, the inputs and the error measures.

The rule is oracle/cips3d_oracle.py::siren: x = points * 2 / 0.24, then sin(g * (W h + b) + p) for the two hidden layers and
the colour sine layer, sigma = ws h2 + bs, feat = Wf hc + bf.  The 16 tensors are taken in ops._SIREN_NAMES order, the FiLM
vectors (gain g*, phase p*) already formed — what the kernels read.

`planes` emulates what a kernel that runs its three dense products (W1, Wc, Wf) on split 16-bit operands does to them:
  "bf16x2"  x -> bf16(x) + bf16(x - bf16(x)), 16 significant bits, both operands (siren_x3_common.h: split2; the fused backward
            recomputes the forward on these planes and contracts its weight gradients on them, siren_bwd_x3.hip:11-12; the staged
            backward stores its rows as such planes, siren.hip: store_layoutN);
  "fp16x2"  fp16 planes, 22 significant bits: the activations as they are (sines, siren_x3_common.h: split2h), the weights as
            W * 2^k with k per matrix such that max |W| * 2^k lies in [2^13, 2^14) and k = 0 for an all-zero matrix
            (siren_x3_common.h: the comment above pow2_scale_for, and its `!(m > 0.f)` branch).
The products themselves accumulate in the dtype of the call, so an fp64 call shows the operand rounding alone and an fp32 call
what a kernel on an fp32 accumulator can reach.  The backward of a `planes` call follows the fused backward kernel: every
gradient that kernel stages as planes is rounded where it is staged, the per-feature sums over the points are taken over those
planes and the aux row [1, x, y, z, 1, dsigma] is rounded too (siren_bwd_x3.hip:11-28, :398-408; see the Functions below).

`sine_error` models the kernels' sines: hardware v_sin_f32 / v_cos_f32 behind a Cody-Waite reduction, or the minimax polynomial,
measured at 1.2e-6 and 1.3e-6 (cips3d_amd/ops.py:165-166, the comment of TRIG_MODE) where torch's fp32 sine is good to 6e-8.  A
sine and the cosine its backward uses each move by a draw, uniform in +- sine_error and fixed by the seed; sin(0) = 0 and
cos(0) = 1 stay exact, as they are in the kernels.  It is the yardstick of the all-fp32 backward, which has no operand rounding
above it: there a feature whose argument carries 150 times its input's error (the spike regime) shows the sines and nothing
else.  Not modelled: the sine argument formed in revolutions (stage_weights_x3<PRE>), fp32-sized.
"""
import functools
import math

import torch
import torch.nn.functional as F

from conftest import seeded_generator

NAMES = ("g0", "p0", "g1", "p1", "gc", "pc", "w0", "b0", "w1", "b1", "ws", "bs", "wc", "bc", "wf", "bf")   # ops._SIREN_NAMES
FILM = NAMES[:6]                 # per-image (B, n) tensors
BOX_SCALE = 2.0 / 0.24
QUANTITIES = ("feat", "sigma") + tuple("d" + n for n in NAMES)
NO_PRODUCT = ("dbs", "dbf")      # sums of the upstream gradient alone (the fused backward takes dbf over dfeat's planes)
# How far above the "bf16x2" yardstick a kernel may sit (tests/test_gpu_siren_fp64.py): the step of 2, 3, 4, 6, 8 that keeps 1.5
# times the spread between two realisations of that yardstick, which tests/test_siren_refs_cpu.py measures and asserts —
# reference-only numbers, never a kernel's — and (2, 3) at the least.  Gradients, per regime, (rms, peak): the spike regime is
# ill-conditioned (one feature's sine argument swings by ~150 rad, a few elements carry the whole error), its realisations
# spread 3.1 / 4.9 where every other regime's stay under 1.35.  The forward's rms multiplier is 2 everywhere.
M_FWD_PEAK = 3
M_GRAD = {"init": (2, 3), "wide": (2, 3), "scaled37": (2, 3), "scaled3e-4": (2, 3), "spike": (6, 8), "wc0": (2, 3)}
M_GRAD_FEW = (3, 4)              # fewer than 512 live rows of upstream (one-hot patterns, the smallest shapes): little or nothing
                                 # averages, two realisations spread up to 1.47 / 2.46


def grad_multipliers(regime, pattern="dense", rows=512):
    """(m_rms, m_peak) of a gradient against the "bf16x2" yardstick; rows = B * P of the case"""
    m = M_GRAD[regime]
    return tuple(max(a, b) for a, b in zip(m, M_GRAD_FEW)) if isinstance(pattern, tuple) or rows < 512 else m


# ----------------------------------------------------------------------------------------------------------------------------
# the split operands
# ----------------------------------------------------------------------------------------------------------------------------
def _two_planes(x, dt):
    hi = x.to(dt).to(x.dtype)
    return hi + (x - hi).to(dt).to(x.dtype)


def _pow2_for(x):
    """2^k with max |x| * 2^k in [2^13, 2^14); 1 for an all-zero (or non-finite) tensor — pow2_scale_for"""
    m = float(x.detach().abs().max()) if x.numel() else 0.0
    if not (m > 0.0) or not math.isfinite(m):
        return 1.0
    return 2.0 ** (13 - math.frexp(m)[1] + 1)      # frexp: m = f * 2^e with f in [0.5, 1), so floor(log2 m) = e - 1


def round_planes(x, planes, scaled):
    """x as the sum of its two 16-bit planes; `scaled`: fp16 planes of x * 2^k (weights, gradients), else of x itself"""
    if planes is None:
        return x
    if planes == "bf16x2":
        return _two_planes(x, torch.bfloat16)
    if planes == "fp16x2":
        s = _pow2_for(x) if scaled else 1.0
        return _two_planes(x * s, torch.float16) / s
    raise ValueError(planes)


class _PlanesLinear(torch.autograd.Function):
    """y = x W^T + b on rounded operands: x (..., in) and W (out, in) are rounded in the forward, the incoming gradient in the
    backward, which multiplies it with the two rounded operands (tests/test_gpu_inr_bf16.py::_BmmBf16 is the precedent) and
    sums it, rounded, for the bias: in the fused backward the per-feature sums over the points ride on the staged planes of the
    gradient against a column of ones (siren_bwd_x3.hip:25-28).  The kernels have no fp16 backward; "fp16x2" scales the
    incoming gradient like a weight so that the emulation stays in range."""

    @staticmethod
    def forward(ctx, x, W, b, planes):
        xr, Wr = round_planes(x, planes, False), round_planes(W, planes, True)
        ctx.save_for_backward(xr, Wr)
        ctx.planes = planes
        return xr @ Wr.t() + b

    @staticmethod
    def backward(ctx, g):
        xr, Wr = ctx.saved_tensors
        gr = round_planes(g, ctx.planes, True)
        g2 = gr.reshape(-1, gr.shape[-1])
        return gr @ Wr, g2.t() @ xr.reshape(-1, xr.shape[-1]), g2.sum(0), None


class _PlanesFilm(torch.autograd.Function):
    """a = g (x W^T + b) + p, a FiLM layer's sine argument, as the fused backward differentiates it (siren_bwd_x3.hip:11-28):
    the gradient da is staged once as planes; the weight gradient contracts those planes with the input's over the points and
    is scaled by the gain afterwards, dW = sum_b g_b (da_b^T x_b); the phase gradient is the planes' column sum and the gain's
    and the bias's follow from the two, dg = (G . W) + b dp, db = sum_b g_b dp_b (the staged form's assembly, ops.py:
    _siren_backward_staged, spells the same formulas out); the data gradient multiplies the planes of g da with W's."""

    @staticmethod
    def forward(ctx, x, W, b, g, p, planes):
        xr, Wr = round_planes(x, planes, False), round_planes(W, planes, True)
        ctx.save_for_backward(xr, Wr, W, b, g)
        ctx.planes = planes
        return g.unsqueeze(1) * (xr @ Wr.t() + b) + p.unsqueeze(1)

    @staticmethod
    def backward(ctx, da):
        xr, Wr, W, b, g = ctx.saved_tensors
        dar = round_planes(da, ctx.planes, True)
        dp = dar.sum(1)
        G = dar.transpose(1, 2) @ xr                                         # (B, out, in)
        dx = round_planes(g.unsqueeze(1) * dar, ctx.planes, True) @ Wr
        return dx, (g.unsqueeze(-1) * G).sum(0), (g * dp).sum(0), (G * W).sum(-1) + b * dp, dp, None


class _PlanesLayer0(torch.autograd.Function):
    """a0 = g0 (W0 x + b0) + p0 with x = BOX_SCALE * points: plain arithmetic forward (the kernels' layer 0 is an fp32 fma
    chain); backward on the planes of da0 and of the aux row [1, x, y, z] (siren_bwd_x3.hip:25-28, :398-404)"""

    @staticmethod
    def forward(ctx, points, w0, b0, g0, p0, planes):
        ctx.save_for_backward(points, w0, b0, g0)
        ctx.planes = planes
        return g0.unsqueeze(1) * F.linear(points * BOX_SCALE, w0, b0) + p0.unsqueeze(1)

    @staticmethod
    def backward(ctx, da):
        points, w0, b0, g0 = ctx.saved_tensors
        dar = round_planes(da, ctx.planes, True)
        dp = dar.sum(1)
        S0 = dar.transpose(1, 2) @ round_planes(points, ctx.planes, True) * BOX_SCALE      # (B, 128, 3)
        return None, (g0.unsqueeze(-1) * S0).sum(0), (g0 * dp).sum(0), (S0 * w0).sum(-1) + b0 * dp, dp, None


class _PlanesSigma(torch.autograd.Function):
    """sigma = ws h2 + bs: dws contracts the planes of h2 with those of the aux row's dsigma (siren_bwd_x3.hip:25-28, :398-404);
    dbs is a plain sum (:405) and ws * dsigma enters d h2 in fp32 (:408)"""

    @staticmethod
    def forward(ctx, h2, ws, bs, planes):
        ctx.save_for_backward(h2, ws)
        ctx.planes = planes
        return F.linear(h2, ws, bs)

    @staticmethod
    def backward(ctx, ds):
        h2, ws = ctx.saved_tensors
        dsr, h2r = round_planes(ds, ctx.planes, True), round_planes(h2, ctx.planes, False)
        return ds * ws, dsr.reshape(-1, 1).t() @ h2r.reshape(-1, h2r.shape[-1]), ds.sum().reshape(1), None


# ----------------------------------------------------------------------------------------------------------------------------
# the function
# ----------------------------------------------------------------------------------------------------------------------------
SINE_ERROR = 1.2e-6              # cips3d_amd/ops.py:165-166


class _CoarseSin(torch.autograd.Function):
    """sin(x) + e1 forward, g * (cos(x) + e2) backward, e uniform in +- err and zero where x is (see the module docstring)"""

    @staticmethod
    def forward(ctx, x, err, seed):
        g = torch.Generator(device=x.device).manual_seed(seed)
        live = (x != 0).to(x.dtype)
        e = (torch.rand((2,) + x.shape, generator=g, dtype=x.dtype, device=x.device) * 2 - 1) * err * live
        ctx.save_for_backward(torch.cos(x) + e[1])
        return torch.sin(x) + e[0]

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


def _sin(x, sine_error, seed):
    return torch.sin(x) if sine_error is None else _CoarseSin.apply(x, sine_error, seed)


def siren_ref(points, t, planes=None, return_args=False, sine_error=None, sine_seed=0):
    """points (B,P,3), t: the 16 tensors in NAMES order (any float dtype, the points') -> (B,P,33) = [feat (32), sigma (1)];
    differentiable w.r.t. t.  return_args: also the three sine arguments (B,P,128), (B,P,128), (B,P,64).  sine_error: see the module docstring (sine_seed: one draw per call).  planes None is
    oracle/cips3d_oracle.py::siren operation for operation."""
    g0, p0, g1, p1, gc, pc, w0, b0, w1, b1, ws, bs, wc, bc, wf, bf = t
    if planes is None:
        a0 = g0.unsqueeze(1) * F.linear(points * BOX_SCALE, w0, b0) + p0.unsqueeze(1)
        h1 = _sin(a0, sine_error, 3 * sine_seed)
        a1 = g1.unsqueeze(1) * F.linear(h1, w1, b1) + p1.unsqueeze(1)
        h2 = _sin(a1, sine_error, 3 * sine_seed + 1)
        sigma = F.linear(h2, ws, bs)
        ac = gc.unsqueeze(1) * F.linear(h2, wc, bc) + pc.unsqueeze(1)
        feat = F.linear(_sin(ac, sine_error, 3 * sine_seed + 2), wf, bf)
    else:
        a0 = _PlanesLayer0.apply(points, w0, b0, g0, p0, planes)
        h1 = _sin(a0, sine_error, 3 * sine_seed)
        a1 = _PlanesFilm.apply(h1, w1, b1, g1, p1, planes)
        h2 = _sin(a1, sine_error, 3 * sine_seed + 1)
        sigma = _PlanesSigma.apply(h2, ws, bs, planes)
        ac = _PlanesFilm.apply(h2, wc, bc, gc, pc, planes)
        feat = _PlanesLinear.apply(_sin(ac, sine_error, 3 * sine_seed + 2), wf, bf, planes)
    out = torch.cat([feat, sigma], dim=-1)
    return (out, (a0, a1, ac)) if return_args else out


def evaluate(points, t, up, dtype, planes=None, device="cpu", images=None, sine_error=None):
    """forward and the gradients of (siren_ref * up).sum() -> {quantity: tensor of `dtype` on `device`} for QUANTITIES.
    `up` (B,P,33) or None (forward only).  images: evaluate that many images at a time (the per-image FiLM gradients are rows,
    the weight gradients add)."""
    B = points.shape[0]
    step = images or B
    cast = lambda v: v.detach().to(device=device, dtype=dtype)
    w = [cast(v).requires_grad_(up is not None) for v in t[6:]]
    outs, film_g = [], [[] for _ in FILM]
    wsum = [torch.zeros_like(v) for v in w]
    for i in range(0, B, step):
        f = [cast(v[i:i + step]).requires_grad_(up is not None) for v in t[:6]]
        out = siren_ref(cast(points[i:i + step]), f + w, planes, sine_error=sine_error, sine_seed=i)
        outs.append(out.detach())
        if up is not None:
            gr = torch.autograd.grad((out * cast(up[i:i + step])).sum(), f + w)
            for k in range(6):
                film_g[k].append(gr[k])
            for k in range(10):
                wsum[k] += gr[6 + k]
    out = torch.cat(outs)
    res = {"feat": out[..., :32], "sigma": out[..., 32]}
    if up is not None:
        for k, n in enumerate(NAMES):
            res["d" + n] = torch.cat(film_g[k]) if k < 6 else wsum[k - 6]
    return res


# ----------------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------------
REGIMES = {
    "init": "a seeded generator's own tensors: the corner every older SIREN test runs in, which ties these tests to them",
    "wide": "gains 30 + 15 N(0,1), phases 8 N(0,1): negative and near-zero gains, up to ten revolutions; image 1 all-zero FiLM",
    "scaled37": "W1, Wc, Wf times 37, compensated in the gains: the images must not depend on the weights' magnitude",
    "scaled3e-4": "the same with 3e-4: the small end of the fp16 planes' power-of-two scale",
    "spike": "one element of W1, Wc, Wf at 2^10 times the matrix rms: the per-matrix scale leaves the bulk 10 bits down",
    "wc0": "Wc all zero: the k = 0 branch of pow2_scale_for, a colour branch that is constant per image",
}


@functools.lru_cache(maxsize=None)
def _generator(seed):
    return seeded_generator(seed)


def generator_tensors(G, style):
    """the 16 tensors of generator G for styles (B,128), attached to G's parameters (NeRFNetwork._siren_args in plain torch)"""
    s = G.siren
    lay = (s.network[0], s.network[1], s.color_layer_sine)
    film = [v for l in lay for v in (l.gain_fc(style) * 15 + 30, l.bias_fc(style))]
    return film + [lay[0].linear.weight, lay[0].linear.bias, lay[1].linear.weight, lay[1].linear.bias, s.final_layer.weight,
                   s.final_layer.bias, lay[2].linear.weight, lay[2].linear.bias, s.color_layer_linear[0].weight,
                   s.color_layer_linear[0].bias]


def make_style(B, seed):
    return torch.randn(B, 128, generator=torch.Generator().manual_seed(1000 + seed))


def make_tensors(regime, B, seed):
    """the 16 SIREN tensors (fp32, CPU, detached) of a regime, see REGIMES"""
    assert regime in REGIMES, regime
    with torch.no_grad():
        t = dict(zip(NAMES, (v.clone() for v in generator_tensors(_generator(seed), make_style(B, seed)))))
    g = torch.Generator().manual_seed(2000 + seed)
    if regime == "wide":
        for n in FILM:
            r = torch.randn(t[n].shape, generator=g)
            t[n] = 30 + 15 * r if n[0] == "g" else 8 * r
            if B > 1:
                t[n][1] = 0.0
    elif regime != "init":
        s = {"scaled37": 37.0, "scaled3e-4": 3e-4}.get(regime, 1.0)
        # W -> s W with the gain divided by s and the bias scaled along (test_siren_forward_x3_sigma_is_fp32_class): the sine
        # arguments keep their values; Wf has nothing behind it, feat scales by s
        for w_, b_, g_ in (("w1", "b1", "g1"), ("wc", "bc", "gc")):
            t[w_] *= s; t[b_] *= s; t[g_] /= s
        t["wf"] *= s
        if regime == "spike":
            for n in ("w1", "wc", "wf"):
                i = int(torch.randint(t[n].numel(), (1,), generator=g))
                t[n].view(-1)[i] = 2.0 ** 10 * float(t[n].pow(2).mean().sqrt())
        if regime == "wc0":
            t["wc"].zero_()
    return [t[n].contiguous() for n in NAMES]


def make_points(kind, B, P, seed):
    """box: uniform in +-0.15.  edge: one tensor of exact zeros, box corners +-0.12, points out to +-0.36 (three times the box) and
    duplicated rows, in runs of eight"""
    g = torch.Generator().manual_seed(3000 + seed)
    pts = (torch.rand(B, P, 3, generator=g) - 0.5) * 0.3
    if kind == "edge":
        sel = (torch.arange(P) // 8) % 5          # 0 box, 1 zeros, 2 corners, 3 far, 4 a copy of the row eight before
        corner = (torch.randint(0, 2, (B, P, 3), generator=g) * 2 - 1) * 0.12
        far = (torch.rand(B, P, 3, generator=g) - 0.5) * 0.72
        pts = torch.where((sel == 1)[None, :, None], torch.zeros(()), pts)
        pts = torch.where((sel == 2)[None, :, None], corner, pts)
        pts = torch.where((sel == 3)[None, :, None], far, pts)
        if P > 8:
            pts = torch.where((sel == 4)[None, :, None], pts.roll(8, 1), pts)
    else:
        assert kind == "box", kind
    return pts.contiguous()


def make_upstream(B, P, seed, pattern="dense"):
    """(B,P,33) upstream of [feat, sigma]: randn + 0.5 (the bias sums do not cancel to nothing), then the pattern: dense,
    dsigma / dfeat (the other part zero), or ("onehot", image, point): one live row"""
    up = torch.randn(B, P, 33, generator=torch.Generator().manual_seed(4000 + seed)) + 0.5
    if pattern == "dsigma":
        up[..., :32] = 0
    elif pattern == "dfeat":
        up[..., 32] = 0
    elif pattern != "dense":
        _, b, p = pattern
        keep = up[b, p].clone()
        up.zero_()
        up[b, p] = keep
    return up


# ----------------------------------------------------------------------------------------------------------------------------
# measures
# ----------------------------------------------------------------------------------------------------------------------------
def distances(q, q64, per_image=False, value_rms=None):
    """{"rms": |q - q64| / |q64|, "peak": max |q - q64| / rms value of q64}, in fp64 on q64's device.  per_image ((B, n) FiLM
    tensors): rms is the largest of the images' own, so that one wrong image among hundreds shows.  Where q64 (an image's row
    of it) is identically zero the measure is 0 for an exactly zero q and inf otherwise.  value_rms: the rms value to measure
    against in place of q64's own, for a q64 of too few numbers to have one (a single sigma can be 0.01 of sigma's rms)."""
    q = q.detach().to(device=q64.device, dtype=torch.float64)
    q64 = q64.detach().double()
    e = q - q64

    def ratio(num, den):
        return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, math.inf, 0.0).to(num.dtype))
    if value_rms is not None:
        assert not per_image
        v = torch.as_tensor(value_rms, dtype=torch.float64, device=q64.device)
        return {"rms": float(e.pow(2).mean().sqrt() / v), "peak": float(e.abs().max() / v)}
    if per_image:
        rms = float(ratio(e.flatten(1).norm(dim=1), q64.flatten(1).norm(dim=1)).max())
    else:
        rms = float(ratio(e.norm(), q64.norm()))
    peak = float(ratio(e.abs().max(), q64.pow(2).mean().sqrt()))
    return {"rms": rms, "peak": peak}


def all_distances(res, truth):
    """{quantity: distances} of an evaluate()-shaped dict against the fp64 one"""
    return {k: distances(res[k], truth[k], per_image=k[1:] in FILM) for k in truth if k in res}
