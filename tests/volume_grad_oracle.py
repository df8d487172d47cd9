"""An fp64 yardstick for the GRADIENT of the baked-volume renderer with respect to its nodes (cips_volume_render_bwd in
include/cips3d_hip.h), in plain torch on the CPU.

THE YARDSTICK is torch.autograd.grad through volume_oracle.render(case, dtype=float64) with the case's sigma and rgb requiring a
gradient: that renderer is plain torch and differentiable as it stands.  The loss is sum(up_rgb rgb) + sum(up_depth depth) +
sum(up_opacity opacity) with seeded randn upstreams (any of the three may be None), zeroed on pixels the oracle flags `near` a
box face (the inside test is the rule's one discontinuity; no case here has such a pixel).  Gradients are returned in the
packed layout (Bv,nx,ny,nz,4): r, g, b, sigma per node.

THE RULE BY HAND (hand_rule), restated and not imported: per ray, with x_k the interpolated sigma, c_k the interpolated colour
(both 0 outside the box), G the upstream of rgb at the pixel, gd and go those of depth and opacity, gsum = G_r + G_g + G_b:
    s_k = G . c_k + gd z_k;    s_off = [last_back] s_{S-1} + [white_back] gsum - go;    Q = 0
    for k = S-1 .. 0:   s' = s_k - s_off;  dalpha = T_k (s' - Q);  Q = alpha_k s' + (1 - alpha_k + 1e-10) Q
                        dx_k = dalpha delta_k exp(-delta_k dens_k) clamp'(x_k)
                        w_k = alpha_k T_k (+ 1 - sum w for k = S-1 under last_back);   dc_k = w_k G
and every inside sample adds omega (dc_k, dx_k) to the eight nodes of its cell, omega the product over the axes of t or 1 - t
(index_add_).  clamp' is 1 for x > 0 else 0 (relu), sigmoid(x) up to 20 and 1 above (softplus).  No division by 1 - alpha.

variant: deliberately WRONG rules, to show that the bar below means something:
    no_top_up    the top-up 1 - sum w missing from the last colour weight            (the last_back cases where some ray's last
                 sample lies inside the box: outside it no node receives that weight)
    go_sign      go enters s_off with the wrong sign                                 (the relu cases that see the volume.  Under
                 softplus the last alpha is 1 - exp(-1e10 softplus(x)) = 1 exactly: opacity is 1 whatever the nodes are and
                 has no gradient — Q starts at s'_last and a constant added to every s' cancels in s' - Q)
    swap_t       t and 1 - t swapped on the y axis                                   (wherever the volume is seen)
    relu_one     relu' taken as 1 everywhere                                         (the relu cases that see the volume)
    delta_prev   the last delta 1e10 replaced by the previous one                    (where the last sample has a density: the
                 softplus cases, whose softplus(0) > 0 even outside the box, and the relu cases whose last samples all lie inside it:
                 where only a few rays end inside, the term can stay below the largest gradient's bar)

THE ERROR MEASURE, per case and per channel group (sigma; colour): max|g - g64| / max|g64|, and exactly 0 for 0 / 0 (a case that
sees nothing).  THE BAR is measured from the reference rule, never from the code under test: the same measure for fp32 torch
autograd of volume_oracle.render(dtype=float32) on that case and those upstreams, times 8 (a kernel sums up to hundreds of
contributions per node in arrival order where index_put sums in a fixed one, and expf / log1pf may differ from torch's by a
few ulp), with a floor of 16 * 2^-24 (two inside-camera cases sit at 2 - 3e-7 by the luck of few terms)."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import volume_oracle as vo

VARIANTS = (None, "no_top_up", "go_sign", "swap_t", "relu_one", "delta_prev")
FLOOR = 16 * 2.0 ** -24
FACTOR = 8.0


@functools.lru_cache(maxsize=None)
def extra_cases():
    """next to volume_oracle.cases(): 9 x 10 pixels (a partial tile in both directions) with a second image behind the first"""
    return dict(
        pairs_9x10_s12_relu_last=vo.make_case(*vo.random_volume(21, 1, 5, 6, 7), vo.cameras([0.9, 2.0], [1.2, 1.7]), 16, 9, 10, 0.8,
                                              1.2, 12, last_back=True),
    )


BLOBS = (((14, 19), (2, 6), (6, 10)), ((1, 5), (10, 18), (1, 4)))            # per volume, per axis: the node range [from, to)


def blob_case(all_nonpositive, inside_camera=False, **kw):
    """test_gpu_volume's two volumes of 26 x 19 x 10 nodes (4 x 3 x 2 bricks), rebuilt: sigma in [-2, -1) except at a few exact
    zeros of both signs, plus — unless all_nonpositive — one positive blob per volume across brick faces."""
    g = torch.Generator().manual_seed(77)
    sigma = -1 - torch.rand(2, 26, 19, 10, generator=g)
    sigma[:, 25, 17, 1], sigma[:, 1, 16, 9], sigma[:, 24, 2, 9] = 0.0, -0.0, 0.0
    if not all_nonpositive:
        for v, ((x0, x1), (y0, y1), (z0, z1)) in enumerate(BLOBS):
            sigma[v, x0:x1, y0:y1, z0:z1] = 400 * torch.rand(x1 - x0, y1 - y0, z1 - z0, generator=g)
    rgb = torch.rand(2, 26, 19, 10, 3, generator=g) * 2 - 1
    if inside_camera:            # every sample lies within 0.06 of the origin, the box reaches 0.10 and more on every side
        return vo.make_case(sigma, rgb, vo.cameras([0.9, 2.1], [1.25, 1.7], radius=0.05), 50, 16, 16, 0.01, 0.09, 12, **kw)
    return vo.make_case(sigma, rgb, vo.cameras([0.8, 2.2], [1.2, 1.9]), 16, 16, 16, 0.8, 1.2, 12, **kw)


@functools.lru_cache(maxsize=None)
def all_cases():
    return {**vo.cases(), **extra_cases()}


@functools.lru_cache(maxsize=None)
def _near_of(name):
    return vo.reference(name).near if name in vo.cases() else vo.render(all_cases()[name], bars=True).near


def upstreams(case, near, seed=0, which=("rgb", "depth", "opacity")):
    """seeded randn for the outputs named in `which` (None for the others), zeroed on near pixels -> (up_rgb, up_depth, up_opacity)"""
    g = torch.Generator().manual_seed(1000 + seed)
    b = case.cam2world.shape[0]
    keep = (~near).unsqueeze(1).float()
    full = (torch.randn(b, 3, case.H, case.W, generator=g) * keep, torch.randn(b, 1, case.H, case.W, generator=g) * keep,
            torch.randn(b, 1, case.H, case.W, generator=g) * keep)
    return tuple(t if n in which else None for n, t in zip(("rgb", "depth", "opacity"), full))


def named_upstreams(name, seed=0, which=("rgb", "depth", "opacity")):
    return upstreams(all_cases()[name], _near_of(name), seed, which)


def autograd_gradient(case, ups, dtype=torch.float64):
    """the yardstick (dtype=float64) or the reference rule's own fp32 error (float32) -> (Bv,nx,ny,nz,4) of `dtype`"""
    leaf = SimpleNamespace(**vars(case))
    leaf.sigma = case.sigma.detach().to(dtype).clone().requires_grad_(True)        # leaves of `dtype`: so is their gradient
    leaf.rgb = case.rgb.detach().to(dtype).clone().requires_grad_(True)
    out = vo.render(leaf, dtype=dtype)
    loss = sum((u.to(dtype) * o).sum() for u, o in zip(ups, (out.rgb, out.depth, out.opacity)) if u is not None)
    d_sigma, d_rgb = torch.autograd.grad(loss, (leaf.sigma, leaf.rgb), allow_unused=True)
    d_sigma = torch.zeros_like(leaf.sigma) if d_sigma is None else d_sigma
    d_rgb = torch.zeros_like(leaf.rgb) if d_rgb is None else d_rgb
    return torch.cat([d_rgb, d_sigma.unsqueeze(-1)], -1).to(dtype)


def _geometry(case, dtype):
    """-> vol (Bv,nx,ny,nz,4), zg (S,), inside (b,H,W,S), cell (b,H,W,S,3) long (zeros outside), tt = u - cell, bi: the volume of
    every sample — volume_oracle's module text, restated"""
    vol = torch.cat([case.rgb, case.sigma.unsqueeze(-1)], -1).to(dtype)
    Bv, nx, ny, nz = vol.shape[:4]
    n = torch.tensor([nx, ny, nz])
    M = case.cam2world.to(dtype)
    b, H, W, S = M.shape[0], case.H, case.W, case.S
    xg, yg, zg = torch.linspace(-1, 1, W).to(dtype), torch.linspace(1, -1, H).to(dtype), case.zg.to(dtype)
    zc = torch.tensor(case.zc, dtype=dtype)
    x, y = xg.view(1, W).expand(H, W), yg.view(H, 1).expand(H, W)
    nrm = torch.sqrt(x * x + y * y + zc * zc)
    d = torch.stack([x / nrm, y / nrm, zc / nrm], -1)
    p = d.view(1, H, W, 1, 3) * zg.view(1, 1, 1, S, 1)
    R, t = M[:, :3, :3].view(b, 1, 1, 1, 3, 3), M[:, :3, 3].view(b, 1, 1, 1, 3)
    world = (R * p.unsqueeze(-2)).sum(-1) + t
    lo, hi = torch.tensor(case.lo, dtype=dtype), torch.tensor(case.hi, dtype=dtype)
    top = (n - 1).to(dtype)
    u = (world - lo) * (top / (hi - lo))
    inside = ((u >= 0) & (u <= top)).all(-1)                                                  # (b,H,W,S)
    cell = torch.minimum(torch.floor(u).clamp_min(0).long(), (n - 2).expand_as(u)).clamp_min(0)
    cell = torch.where(inside.unsqueeze(-1), cell, torch.zeros_like(cell))
    tt = u - cell.to(dtype)
    bi = (torch.arange(b) if Bv == b and Bv > 1 else torch.zeros(b, dtype=torch.long)).view(b, 1, 1, 1).expand(b, H, W, S)
    return vol, zg, inside, cell, tt, bi


def last_sample_inside(case, every=False):
    """does some (every=True: every) ray's LAST sample lie inside the box?  (only there can last_back's top-up, or the last delta
    under relu, reach a node)"""
    last = _geometry(case, torch.float64)[2][..., -1]
    return bool(last.all() if every else last.any())


def hand_rule(case, ups, dtype=torch.float64, variant=None):
    """the rule of the module text in `dtype` arithmetic -> (Bv,nx,ny,nz,4)"""
    assert variant in VARIANTS
    vol, zg, inside, cell, tt, bi = _geometry(case, dtype)
    Bv, nx, ny, nz = vol.shape[:4]
    b, H, W, S = case.cam2world.shape[0], case.H, case.W, case.S
    i, j, k = cell.unbind(-1)
    tx, ty, tz = tt.unbind(-1)
    corners = []
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                wy = (1 - ty if dj else ty) if variant == "swap_t" else (ty if dj else 1 - ty)
                om = (tx if di else 1 - tx) * wy * (tz if dk else 1 - tz)
                corners.append((((bi * nx + i + di) * ny + j + dj) * nz + k + dk, om))
    flat = vol.reshape(-1, 4)
    right = [(idx, ((tx if c & 4 else 1 - tx) * (ty if c & 2 else 1 - ty) * (tz if c & 1 else 1 - tz))) for c, (idx, _) in
             enumerate(corners)]                                                              # the forward is never the wrong one
    v = sum(om.unsqueeze(-1) * flat[idx] for idx, om in right)
    v = torch.where(inside.unsqueeze(-1), v, torch.zeros_like(v))
    c, xs = v[..., :3], v[..., 3]
    if case.clamp_mode == 'softplus':
        dens, dclamp = F.softplus(xs), torch.where(xs > 20, torch.ones_like(xs), torch.sigmoid(xs))
    else:
        dens, dclamp = F.relu(xs), (xs > 0).to(dtype)
    if variant == "relu_one" and case.clamp_mode != 'softplus':
        dclamp = torch.ones_like(xs)
    last = zg[S - 1] - zg[S - 2] if variant == "delta_prev" else torch.tensor(1e10, dtype=dtype)
    delta = torch.cat([zg[1:] - zg[:-1], last.view(1)])
    E = torch.exp(-delta * dens)
    alpha = 1 - E
    f = 1 - alpha + 1e-10
    T = torch.cat([torch.ones_like(f[..., :1]), torch.cumprod(f, -1)[..., :-1]], -1)
    w = alpha * T
    wsum = w.sum(-1)
    zero = torch.zeros(b, H, W, dtype=dtype)
    G = ups[0].to(dtype).permute(0, 2, 3, 1) if ups[0] is not None else torch.zeros(b, H, W, 3, dtype=dtype)
    gd = ups[1].to(dtype)[:, 0] if ups[1] is not None else zero
    go = ups[2].to(dtype)[:, 0] if ups[2] is not None else zero
    s = (G.unsqueeze(-2) * c).sum(-1) + gd.unsqueeze(-1) * zg
    s_off = (s[..., S - 1] if case.last_back else zero) + (G.sum(-1) if case.white_back else zero)
    s_off = s_off + go if variant == "go_sign" else s_off - go
    Q, dx = zero, [None] * S
    for q in range(S - 1, -1, -1):
        sp = s[..., q] - s_off
        dalpha = T[..., q] * (sp - Q)
        Q = alpha[..., q] * sp + f[..., q] * Q
        dx[q] = dalpha * delta[q] * E[..., q] * dclamp[..., q]
    dx = torch.stack(dx, -1)
    wc = w.clone()
    if case.last_back and variant != "no_top_up":
        wc[..., S - 1] += 1 - wsum
    g4 = torch.cat([wc.unsqueeze(-1) * G.unsqueeze(-2), dx.unsqueeze(-1)], -1)
    g4 = torch.where(inside.unsqueeze(-1), g4, torch.zeros_like(g4))
    out = torch.zeros(Bv * nx * ny * nz, 4, dtype=dtype)
    for idx, om in corners:
        out.index_add_(0, idx.reshape(-1), (om.unsqueeze(-1) * g4).reshape(-1, 4))
    return out.view(Bv, nx, ny, nz, 4)


def measure(g, g64):
    """-> (sigma, colour): max|g - g64| / max|g64| per channel group; exactly 0 for 0 / 0; inf for a NaN"""
    g, g64 = g.detach().cpu().double(), g64.double()
    out = []
    for sl in (slice(3, 4), slice(0, 3)):
        err, ref = (g[..., sl] - g64[..., sl]).abs(), g64[..., sl].abs().max()
        err = float(torch.where(torch.isnan(err), torch.full_like(err, float('inf')), err).max())
        out.append(0.0 if err == 0 else (err / float(ref) if float(ref) > 0 else float('inf')))
    return tuple(out)


def bar_of(case, ups, g64):
    """-> (sigma, colour): FACTOR x the reference rule's own fp32 error on this case and these upstreams, at least FLOOR"""
    m = measure(autograd_gradient(case, ups, torch.float32), g64)
    return tuple(max(FACTOR * v, FLOOR) for v in m)


@functools.lru_cache(maxsize=None)
def reference(name, seed=0, which=("rgb", "depth", "opacity")):
    """a named case's upstreams, fp64 gradient and bar: computed once, shared, never modified"""
    case = all_cases()[name]
    ups = named_upstreams(name, seed, which)
    g64 = autograd_gradient(case, ups)
    return SimpleNamespace(case=case, ups=ups, g64=g64, bar=bar_of(case, ups, g64))


def within(m, bar):
    return m[0] <= bar[0] and m[1] <= bar[1]
