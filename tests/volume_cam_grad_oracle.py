"""An fp64 yardstick for the gradient of the baked-volume renderer with respect to its CAMERAS (cips_volume_render_bwd_cam in
include/cips3d_hip.h), in plain torch on the CPU.

THE YARDSTICK is torch.autograd.grad of sum(up out) through volume_oracle.render(case, dtype=float64) with the case's cam2world
requiring a gradient: that renderer is plain torch and differentiable through the camera as it stands (floor carries no
gradient, tt = u - cell does; the sample depths are constants).  -> (b,4,4), row 3 exactly zero.  The cases are those of
volume_grad_oracle.all_cases() and four two-blob volumes of 26 x 19 x 10 nodes (4 x 3 x 2 bricks).

FLAGGED PIXELS.  The render is continuous in the camera but its gradient is not: the slope of the trilinear interpolant jumps at
every cell face, and relu' jumps at sigma = 0.  fp32 may decide either the other way, so the upstreams (seeded randn, those of
volume_grad_oracle) are zeroed on a pixel when
    near   the oracle's flag: some sample within e_u of a box face;
    face   some inside sample has |u_a - round(u_a)| <= e_u on some axis (an interior cell face);
    zero   under relu, some inside sample has |sigma| <= e_sigma.
e_u and e_sigma are volume_oracle's bar expressions, restated here: with A_a = sum_k |R_ak p_k| + |t_a|,
    e_pos = 12 eps A,    e_u = inv_h (e_pos + eps (|x| + |lo|)) + 4 eps |u|,    e_sigma = L (e_ux + e_uy + e_uz) + 12 eps m
with L and m the range and the largest magnitude of sigma over the 4 x 4 x 4 nodes around the cell.  A flagged pixel adds exactly
nothing on either side.  At most CAP = 5 % of a camera's pixels may be flagged (a condition on the cases, asserted in
tests/test_volume_cam_grad_oracle_cpu.py: a case beyond it moves its camera, not the cap).

THE RULE BY HAND (hand_rule), restated and not imported.  The march and the reverse scan are volume_grad_oracle's: w_k the
colour weight (top-up included for the last sample under last_back), dx_k the gradient of the interpolated sigma, G the pixel's
rgb upstream; gd and go reach the camera only through dx_k.  For an inside sample in cell (i, j, k) with weights t the slope of
v(t) = (c, sigma) along axis a is the difference of the cell's two bilinear faces, times inv_h[a].  Then
    dp_k = w_k (G . grad c_k) + dx_k grad sigma_k;    A = sum_k dp_k;    B = sum_k z_k dp_k
    d cam2world[:3,:3] = sum_rays B dir^T;    d cam2world[:3,3] = sum_rays A;    row 3 = 0.

variant: deliberately WRONG rules, to show that the bar below means something (can_show says where each can):
    inv_h_x      inv_h dropped on the x axis                       (wherever the gradient is not zero)
    no_z         B formed without z_k                              (wherever the gradient is not zero)
    transposed   d R transposed                                    (wherever the gradient is not zero)
    no_top_up    the top-up missing from the last colour weight    (the last_back cases where every ray's last sample lies inside
                 the box; where only a few rays end inside, the term can stay below the largest entry's bar)
    gd_z         gd added as if the depth z_k were the distance of the world point along the ray, d z / d x = R dir
                                                                   (wherever some weight is not zero)
    no_sigma     the grad sigma term dropped                       (wherever some dx is not zero: not on the non-positive
                 volumes, where relu' = 0 at every sample)

THE ERROR MEASURE, per case and camera: max|g - g64| / max|g64| over the 3 x 4 block, exactly 0 for 0 / 0.  THE BAR is measured
from the reference rule, never from the code under test: the same measure for fp32 torch autograd of
volume_oracle.render(dtype=float32) on that case and those upstreams, times 8, with a floor of 16 * 2^-24 — the convention and
the reasons of volume_grad_oracle (a kernel sums in another fixed order than torch, and expf / log1pf may differ by a few ulp)."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import volume_grad_oracle as go
import volume_oracle as vo

VARIANTS = (None, "inv_h_x", "no_z", "transposed", "no_top_up", "gd_z", "no_sigma")
EPS32 = 2.0 ** -24
FLOOR = 16 * 2.0 ** -24
FACTOR = 8.0
CAP = 0.05


@functools.lru_cache(maxsize=None)
def blob_cases():
    return dict(
        blobs_16_s12_relu_white=go.blob_case(False, white_back=True),
        blobs_16_s12_relu_last=go.blob_case(False, last_back=True),
        nonpositive_16_s12_relu_white=go.blob_case(True, white_back=True),
        nonpositive_inside_16_s12_relu_last=go.blob_case(True, True, last_back=True),
    )


@functools.lru_cache(maxsize=None)
def all_cases():
    return {**go.all_cases(), **blob_cases()}


def _geometry(case, dtype):
    """volume_oracle's module text, restated -> the pieces of every sample (b,H,W,S,...)"""
    vol = torch.cat([case.rgb, case.sigma.unsqueeze(-1)], -1).to(dtype)
    Bv, nx, ny, nz = vol.shape[:4]
    n = torch.tensor([nx, ny, nz])
    M = case.cam2world.to(dtype)
    b, H, W, S = M.shape[0], case.H, case.W, case.S
    xg, yg, zg = torch.linspace(-1, 1, W).to(dtype), torch.linspace(1, -1, H).to(dtype), case.zg.to(dtype)
    zc = torch.tensor(case.zc, dtype=dtype)
    x, y = xg.view(1, W).expand(H, W), yg.view(H, 1).expand(H, W)
    nrm = torch.sqrt(x * x + y * y + zc * zc)
    d = torch.stack([x / nrm, y / nrm, zc / nrm], -1)                                          # (H,W,3)
    p = d.view(1, H, W, 1, 3) * zg.view(1, 1, 1, S, 1)
    R, t = M[:, :3, :3].view(b, 1, 1, 1, 3, 3), M[:, :3, 3].view(b, 1, 1, 1, 3)
    world = (R * p.unsqueeze(-2)).sum(-1) + t
    lo, hi = torch.tensor(case.lo, dtype=dtype), torch.tensor(case.hi, dtype=dtype)
    top = (n - 1).to(dtype)
    inv_h = top / (hi - lo)
    u = (world - lo) * inv_h
    inside = ((u >= 0) & (u <= top)).all(-1)
    cell = torch.minimum(torch.floor(u).clamp_min(0).long(), (n - 2).expand_as(u)).clamp_min(0)
    cell = torch.where(inside.unsqueeze(-1), cell, torch.zeros_like(cell))
    tt = u - cell.to(dtype)
    bi = (torch.arange(b) if Bv == b and Bv > 1 else torch.zeros(b, dtype=torch.long)).view(b, 1, 1, 1).expand(b, H, W, S)
    i, j, k = cell.unbind(-1)
    flat = vol.reshape(-1, 4)
    corner = lambda di, dj, dk: flat[((bi * nx + i + di) * ny + j + dj) * nz + k + dk]         # (b,H,W,S,4)
    return SimpleNamespace(vol=vol, zg=zg, d=d, p=p, R=R, t=t, world=world, lo=lo, inv_h=inv_h, top=top, u=u, inside=inside,
                           cell=cell, tt=tt, bi=bi, corner=corner, b=b, H=H, W=W, S=S)


def _interpolate(g):
    """-> v (b,H,W,S,4) and its slope along t_x, t_y, t_z (b,H,W,S,3,4), both zero outside the box"""
    lerp = lambda a_, b_, w_: a_ + w_.unsqueeze(-1) * (b_ - a_)
    tx, ty, tz = g.tt.unbind(-1)
    c = [[[g.corner(di, dj, dk) for dk in (0, 1)] for dj in (0, 1)] for di in (0, 1)]
    cz = [[lerp(c[di][dj][0], c[di][dj][1], tz) for dj in (0, 1)] for di in (0, 1)]
    dz = [[c[di][dj][1] - c[di][dj][0] for dj in (0, 1)] for di in (0, 1)]
    v = lerp(lerp(cz[0][0], cz[0][1], ty), lerp(cz[1][0], cz[1][1], ty), tx)
    sx = lerp(cz[1][0], cz[1][1], ty) - lerp(cz[0][0], cz[0][1], ty)
    sy = lerp(cz[0][1] - cz[0][0], cz[1][1] - cz[1][0], tx)
    sz = lerp(lerp(dz[0][0], dz[0][1], ty), lerp(dz[1][0], dz[1][1], ty), tx)
    slope = torch.stack([sx, sy, sz], -2)
    keep = g.inside.unsqueeze(-1)
    return torch.where(keep, v, torch.zeros_like(v)), torch.where(keep.unsqueeze(-1), slope, torch.zeros_like(slope))


def _neighbourhood(v):
    """vol_oracle's: per cell, over the 4 x 4 x 4 nodes around it, (range, largest magnitude) of v (Bv,nx,ny,nz)"""
    v = v.unsqueeze(1)
    hi = F.max_pool3d(F.pad(v, (1, 1, 1, 1, 1, 1), value=-math.inf), 4, 1)
    lo = -F.max_pool3d(F.pad(-v, (1, 1, 1, 1, 1, 1), value=-math.inf), 4, 1)
    return (hi - lo)[:, 0], torch.maximum(hi.abs(), lo.abs())[:, 0]


def flags(case):
    """-> SimpleNamespace(near, face, zero, any: (b,H,W) bool) in fp64, by the module text"""
    g = _geometry(case, torch.float64)
    eps = EPS32
    A = (g.R.abs() * g.p.abs().unsqueeze(-2)).sum(-1) + g.t.abs()
    e_u = g.inv_h * (12 * eps * A + eps * (g.world.abs() + g.lo.abs())) + 4 * eps * g.u.abs()   # (b,H,W,S,3)
    near = vo.render(case, bars=True).near
    face = (g.inside.unsqueeze(-1) & ((g.u - torch.round(g.u)).abs() <= e_u)).any(-1).any(-1)
    zero = torch.zeros_like(face)
    if case.clamp_mode != 'softplus':
        rng, mag = _neighbourhood(g.vol[..., 3])
        i, j, k = g.cell.unbind(-1)
        e_sigma = rng[g.bi, i, j, k] * e_u.sum(-1) + 12 * eps * mag[g.bi, i, j, k]
        sigma = _interpolate(g)[0][..., 3]
        zero = (g.inside & (sigma.abs() <= e_sigma)).any(-1)
    return SimpleNamespace(near=near, face=face, zero=zero, any=near | face | zero)


@functools.lru_cache(maxsize=None)
def named_flags(name):
    return flags(all_cases()[name])


def named_upstreams(name, seed=0, which=("rgb", "depth", "opacity")):
    """volume_grad_oracle's seeded randn upstreams, zeroed on every flagged pixel"""
    return go.upstreams(all_cases()[name], named_flags(name).any, seed, which)


def autograd_gradient(case, ups, dtype=torch.float64):
    """the yardstick (dtype=float64) or the reference rule's own fp32 error (float32) -> (b,4,4) of `dtype`"""
    leaf = SimpleNamespace(**vars(case))
    leaf.cam2world = case.cam2world.detach().to(dtype).clone().requires_grad_(True)
    out = vo.render(leaf, dtype=dtype)
    loss = sum((u.to(dtype) * o).sum() for u, o in zip(ups, (out.rgb, out.depth, out.opacity)) if u is not None)
    g, = torch.autograd.grad(loss, leaf.cam2world, allow_unused=True)
    return torch.zeros_like(leaf.cam2world) if g is None else g


def scan(case, ups, dtype=torch.float64, variant=None):
    """volume_grad_oracle's march and reverse scan -> (g: the geometry, slope (b,H,W,S,3,4) in world units, wc (b,H,W,S) the
    colour weights, dx (b,H,W,S), G (b,H,W,3), gd (b,H,W)), all zero where a sample is outside the box"""
    g = _geometry(case, dtype)
    b, H, W, S, zg = g.b, g.H, g.W, g.S, g.zg
    v, slope = _interpolate(g)
    inv_h = g.inv_h.clone()
    if variant == "inv_h_x":
        inv_h[0] = 1.0
    slope = slope * inv_h.view(3, 1)
    c, xs = v[..., :3], v[..., 3]
    if case.clamp_mode == 'softplus':
        dens, dclamp = F.softplus(xs), torch.where(xs > 20, torch.ones_like(xs), torch.sigmoid(xs))
    else:
        dens, dclamp = F.relu(xs), (xs > 0).to(dtype)
    delta = torch.cat([zg[1:] - zg[:-1], torch.tensor([1e10], dtype=dtype)])
    E = torch.exp(-delta * dens)
    alpha = 1 - E
    f = 1 - alpha + 1e-10
    T = torch.cat([torch.ones_like(f[..., :1]), torch.cumprod(f, -1)[..., :-1]], -1)
    w = alpha * T
    zero = torch.zeros(b, H, W, dtype=dtype)
    G = ups[0].to(dtype).permute(0, 2, 3, 1) if ups[0] is not None else torch.zeros(b, H, W, 3, dtype=dtype)
    gd = ups[1].to(dtype)[:, 0] if ups[1] is not None else zero
    go_ = ups[2].to(dtype)[:, 0] if ups[2] is not None else zero
    s = (G.unsqueeze(-2) * c).sum(-1) + gd.unsqueeze(-1) * zg
    s_off = (s[..., S - 1] if case.last_back else zero) + (G.sum(-1) if case.white_back else zero) - go_
    Q, dx = zero, [None] * S
    for q in range(S - 1, -1, -1):
        sp = s[..., q] - s_off
        dalpha = T[..., q] * (sp - Q)
        Q = alpha[..., q] * sp + f[..., q] * Q
        dx[q] = dalpha * delta[q] * E[..., q] * dclamp[..., q]
    dx = torch.stack(dx, -1)
    wc = w.clone()
    if case.last_back and variant != "no_top_up":
        wc[..., S - 1] += 1 - w.sum(-1)
    keep = g.inside.to(dtype)
    return g, slope, wc * keep, dx * keep, G, gd


def hand_rule(case, ups, dtype=torch.float64, variant=None):
    """the rule of the module text in `dtype` arithmetic -> (b,4,4)"""
    assert variant in VARIANTS
    g, slope, wc, dx, G, gd = scan(case, ups, dtype, variant)
    colour = (slope[..., :3] * G.view(g.b, g.H, g.W, 1, 1, 3)).sum(-1)                           # G . grad c: (b,H,W,S,3)
    dp = wc.unsqueeze(-1) * colour
    if variant != "no_sigma":
        dp = dp + dx.unsqueeze(-1) * slope[..., 3]
    if variant == "gd_z":
        along = (g.R * g.d.view(1, g.H, g.W, 1, 1, 3)).sum(-1)                                   # R dir: (b,H,W,1,3)
        dp = dp + (gd.unsqueeze(-1) * wc).unsqueeze(-1) * along
    A = dp.sum(-2)                                                                              # (b,H,W,3)
    B = dp.sum(-2) if variant == "no_z" else (g.zg.view(g.S, 1) * dp).sum(-2)
    dR = (B.unsqueeze(-1) * g.d.view(1, g.H, g.W, 1, 3)).sum((1, 2))                             # (b,3,3)
    if variant == "transposed":
        dR = dR.transpose(1, 2)
    out = torch.zeros(g.b, 4, 4, dtype=dtype)
    out[:, :3, :3] = dR
    out[:, :3, 3] = A.sum((1, 2))
    return out


def can_show(case, ups, variant):
    """can the wrong rule `variant` differ from the right one on this case and these upstreams?  Derived from the rule in fp64,
    per camera -> list of bool"""
    g, slope, wc, dx, G, gd = scan(case, ups)
    per_cam = lambda t: [bool(t[i].any()) for i in range(g.b)]
    moves = per_cam(autograd_gradient(case, ups) != 0)
    if variant in ("inv_h_x", "no_z", "transposed"):
        return moves
    if variant == "no_top_up":
        every = bool(go.last_sample_inside(case, every=True))
        return [bool(case.last_back) and every and m for m in moves]
    if variant == "gd_z":
        return per_cam((wc != 0) & (gd != 0).unsqueeze(-1))
    if variant == "no_sigma":
        return per_cam(dx != 0)
    raise ValueError(variant)


def measure(g, g64):
    """-> per camera: max|g - g64| / max|g64| over the 3 x 4 block; exactly 0 for 0 / 0; inf for a NaN"""
    g, g64 = g.detach().cpu().double()[:, :3], g64.double()[:, :3]
    out = []
    for i in range(g64.shape[0]):
        err, ref = (g[i] - g64[i]).abs(), float(g64[i].abs().max())
        err = float(torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err).max())
        out.append(0.0 if err == 0 else (err / ref if ref > 0 else float('inf')))
    return out


def bar_of(case, ups, g64):
    """-> per camera: FACTOR x the reference rule's own fp32 error on this case and these upstreams, at least FLOOR"""
    return [max(FACTOR * v, FLOOR) for v in measure(autograd_gradient(case, ups, torch.float32), g64)]


@functools.lru_cache(maxsize=None)
def reference(name, seed=0, which=("rgb", "depth", "opacity")):
    """a named case's upstreams, fp64 gradient and bar: computed once, shared, never modified"""
    case = all_cases()[name]
    ups = named_upstreams(name, seed, which)
    g64 = autograd_gradient(case, ups)
    return SimpleNamespace(case=case, ups=ups, g64=g64, bar=bar_of(case, ups, g64), flags=named_flags(name))


def within(m, bar):
    return all(a <= b for a, b in zip(m, bar))
