"""An fp64 yardstick for the baked-volume renderer (csrc/volume.hip, cips_volume_render in include/cips3d_hip.h), in plain torch
on the CPU, taking the fp32 inputs (volume, box, camera matrices, the three linspace grids, zc) as given.

THE RULE (restated, not imported).  Pixel (r, c) of camera b has the unit direction d = (xg[c], yg[r], zc) / |.| and samples
z_s = zg[s]; the world point is x = R (d z_s) + t.  The lattice spreads n_a nodes uniformly over [lo_a, hi_a]:
u_a = (x_a - lo_a) (n_a - 1) / (hi_a - lo_a).  A sample is inside iff 0 <= u_a <= n_a - 1 on all axes; its cell is
min(floor(u_a), n_a - 2) and the four channels r, g, b, sigma are interpolated by nested lerps p + t (q - p) along z, y, x.
Outside: sigma = 0, colour 0.  Then oracle/cips3d_oracle.py::integrate without noise: delta_s = z_{s+1} - z_s (last 1e10),
alpha = 1 - exp(-delta clamp(sigma)), w_s = alpha_s prod_{t<s} (1 - alpha_t + 1e-10), opacity = sum w, last_back adds 1 - sum w
to the last weight, rgb = sum w c, depth = sum w z, white_back adds 1 - sum w to rgb.

THE ERROR BAR, per pixel and output, from eps = 2^-24 (fp32 round-to-nearest: every operation is off by at most eps times its
result; fused or not, both stay inside the counts below).  Nothing in it comes from the code under test.
  position   d: three products, two sums, a square root, a division, and one eps for a linspace built on another device: 6 eps
             relative per component; p = d z: 7 eps; each of the three products of a matrix row with p: 8 eps, three additions
             on top.  With A_a = sum_k |R_ak p_k| + |t_a|:   e_x = 12 eps A_a.
  index      u is computed as fl(fl(x - lo) * inv_h) with inv_h = fl(fl(n - 1) / fl(hi - lo)), 2 eps relative:
                 e_u = inv_h (e_x + eps (|x| + |lo|)) + 4 eps |u|
             — it scales with |x| / h: a fine lattice far from the origin is located worse, in units of its cells.
  near       the inside test is the rule's only discontinuity.  A sample is NEAR a face if every u_a lies in
             [-e_u, n_a - 1 + e_u] and some u_a within e_u of 0 or n_a - 1; a pixel with such a sample is flagged `near` and
             exempt (fp32 may decide the test the other way).  Cell boundaries are no discontinuity: the interpolant is continuous.
  trilinear  t = u - cell is exact.  Each channel is Lipschitz in u_a with the largest corner difference of the cell hit; an
             index error may cross into a neighbouring cell, so with L and m the range and the largest magnitude of the channel
             over the 4 x 4 x 4 nodes around the cell:   e_v = L (e_ux + e_uy + e_uz) + 12 eps m
             (three levels of lerps, three roundings each of a quantity <= 2 m, propagated with factors <= 1).
  clamp      softplus is 1-Lipschitz and log1p(exp(.)) adds 4 eps relative:  e_dens = e_sigma + 4 eps dens.  relu is
             1-Lipschitz too, but EXACTLY zero with no error below zero: a sigma further than e_sigma below zero stays
             clamped whatever fp32 does to it, so   e_dens = min(e_sigma, relu(sigma + e_sigma)) + 4 eps dens   (the largest
             value relu can take within e_sigma of sigma, which is 0 in the dead zone).
  alpha      x = delta dens: one eps for the difference of depths, one for the product:  e_x = delta e_dens + 2 eps x.
             E = exp(-x) moves by at most E (exp(e_x) - 1); expf and the subtraction from one add 4 eps (nothing where x = 0 and
             e_x = 0: exp(-0) = 1 and 1 - 1 = 0 are exact):   e_alpha = min(1, E expm1(e_x) + 4 eps).
             Under the last delta = 1e10 a sigma within e_sigma of zero has e_alpha = 1: the bar says so rather than hide it.
  weights    f = 1 - alpha + 1e-10, where fp32 drops the 1e-10:  e_f = e_alpha + 2 eps + 1e-10.  T' = T f:
                 e_T' = e_T f + T e_f + e_T e_f + 2 eps T'     (the kernel keeps T in double; an fp32 product is covered)
             w = alpha fl32(T):   e_w = e_alpha T + alpha e_T + e_alpha e_T + 2 eps w.
  sums       S terms, a top-up and a background term accumulated in fp32 in any order: (S + 4) eps times the sum of the
             magnitudes of the terms.  opacity: sum e_w;  depth: sum e_w z;  rgb: sum (e_w |c| + w e_c + e_w e_c);
             extra = 1 - sum w has e_extra = e_opacity + eps (1 + |extra|) and enters with |c_last|, z_last resp. 1.

tests/test_volume_oracle_cpu.py shows that the bar means something: the same rule in fp32 torch arithmetic stays inside it, and
three deliberately wrong rules (nearest node, samples fetched one depth further than reported, x and z axes swapped) leave it on most
pixels; a fourth (last_back's top-up dropped from the colour) leaves it wherever the top-up is larger than the bar."""
import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from raster_oracle import zc_of

EPS32 = 2.0 ** -24
VARIANTS = (None, "nearest", "shift", "swap_xz", "no_top_up")
BOX_LO, BOX_HI = (-0.15, -0.12, -0.10), (0.15, 0.12, 0.14)


def random_volume(seed, Bv, nx, ny, nz, scale=40.0):
    """seeded: sigma (Bv,nx,ny,nz) ~ scale * N(0, 1), both signs; rgb (Bv,nx,ny,nz,3) uniform in [-1, 1]"""
    g = torch.Generator().manual_seed(seed)
    sigma = torch.randn(Bv, nx, ny, nz, generator=g) * scale
    rgb = torch.rand(Bv, nx, ny, nz, 3, generator=g) * 2 - 1
    return sigma, rgb


def cameras(yaws, pitches, radius=1.0, lookat=(0., 0., 0.)):
    from cips3d_amd import evaluation
    return evaluation.orbit_cameras(yaws, pitches, radius=radius, lookat=lookat, device='cpu')


def make_case(sigma, rgb, cam2world, fov, H, W, ray_start, ray_end, S, clamp_mode='relu', last_back=False, white_back=False,
              lo=BOX_LO, hi=BOX_HI):
    f32 = lambda v: tuple(float(torch.tensor(x, dtype=torch.float32)) for x in v)          # the box as the kernel receives it
    return SimpleNamespace(sigma=sigma, rgb=rgb, cam2world=cam2world, zc=zc_of(fov), H=H, W=W, S=S,
                           zg=torch.linspace(ray_start, ray_end, S), clamp_mode=clamp_mode, last_back=last_back,
                           white_back=white_back, lo=f32(lo), hi=f32(hi))


@functools.lru_cache(maxsize=None)
def cases():
    """Three-quarter views only: no camera axis is parallel to a box face, no ray_start lies on one.  The box is BOX_LO..BOX_HI."""
    small, big = (5, 6, 7), (9, 17, 10)
    corner = BOX_HI
    out = dict(
        outside_5x7_s12_relu=make_case(*random_volume(1, 1, *small), cameras([1.1], [1.3]), 16, 5, 7, 0.8, 1.2, 12),
        outside_16_s12_softplus_last=make_case(*random_volume(2, 1, *big), cameras([0.7], [1.9]), 16, 16, 16, 0.8, 1.2, 12,
                                               'softplus', last_back=True),
        outside_16_s2_relu_white=make_case(*random_volume(3, 1, *big), cameras([2.3], [1.2]), 12, 16, 16, 0.96, 1.04, 2,
                                           white_back=True),
        inside_16_s12_relu_last_white=make_case(*random_volume(4, 1, *small), cameras([0.9], [1.25], radius=0.05), 60, 16, 16,
                                                0.01, 0.3, 12, last_back=True, white_back=True),
        inside_5x7_s2_softplus=make_case(*random_volume(5, 1, *small, scale=8.0), cameras([2.6], [1.8], radius=0.04), 40, 5, 7, 0.02, 0.12,
                                         2, 'softplus'),
        miss_5x7_s12_relu_white=make_case(*random_volume(6, 1, *small), cameras([1.1], [1.3], lookat=(2., 2., 2.)), 24, 5, 7, 0.8,
                                          1.2, 12, white_back=True),
        corner_16_s12_relu_last=make_case(*random_volume(7, 1, *big), cameras([0.6], [1.1], lookat=corner), 12, 16, 16, 0.8, 1.2,
                                          12, last_back=True),
        corner_16_s12_softplus_white=make_case(*random_volume(8, 1, *small), cameras([2.0], [2.0], lookat=corner), 12, 16, 16, 0.8,
                                               1.2, 12, 'softplus', white_back=True),
        turntable_16_s12_relu=make_case(*random_volume(9, 1, *big), cameras([0.5, 1.2, 2.4], [1.3, 1.0, 1.9]), 16, 16, 16, 0.8,
                                        1.2, 12),
        # a smooth, thin volume seen from inside with every last sample inside the box: last_back's top-up carries most of the
        # colour, and the bars are small (sigma of scale 4: ten times less range per cell than the others)
        inside_16_s12_relu_last_smooth=make_case(*random_volume(11, 1, *small, scale=4.0), cameras([0.9], [1.25], radius=0.05), 50,
                                                 16, 16, 0.01, 0.09, 12, last_back=True),
        pairs_5x7_s12_softplus_last=make_case(*random_volume(10, 2, *small), cameras([1.0, 2.2], [1.2, 1.8]), 16, 5, 7, 0.8, 1.2,
                                              12, 'softplus', last_back=True),
    )
    return out


def _gather(vol, b_idx, i, j, k):
    """vol (Bv,nx,ny,nz,C), index tensors of one shape -> (..., C)"""
    return vol[b_idx, i, j, k]


def _neighbourhood(vol):
    """per cell, over the 4 x 4 x 4 nodes around it and per channel: (range, largest magnitude), each (Bv,nx-1,ny-1,nz-1,C)"""
    v = vol.permute(0, 4, 1, 2, 3)
    hi = F.max_pool3d(F.pad(v, (1, 1, 1, 1, 1, 1), value=-math.inf), 4, 1)
    lo = -F.max_pool3d(F.pad(-v, (1, 1, 1, 1, 1, 1), value=-math.inf), 4, 1)
    back = lambda t: t.permute(0, 2, 3, 4, 1)
    return back(hi - lo), back(torch.maximum(hi.abs(), lo.abs()))


def render(case, dtype=torch.float64, variant=None, bars=False):
    """The rule in `dtype` arithmetic -> SimpleNamespace(rgb (b,3,H,W), depth (b,1,H,W), opacity (b,1,H,W), sees (b,H,W): some
    sample is inside).  variant: None, or one of the deliberately wrong rules.  bars=True (fp64, the right rule only) adds
    bar_rgb, bar_depth, bar_opacity (shapes of the outputs) and near (b,H,W)."""
    assert variant in VARIANTS and not (bars and (variant is not None or dtype != torch.float64))
    eps = EPS32
    vol = torch.cat([case.rgb, case.sigma.unsqueeze(-1)], -1).to(dtype)                      # (Bv,nx,ny,nz,4)
    if variant == "swap_xz":
        vol = vol.permute(0, 3, 2, 1, 4).contiguous()
    Bv, n = vol.shape[0], torch.tensor(vol.shape[1:4])
    M = case.cam2world.to(dtype)
    b, H, W, S = M.shape[0], case.H, case.W, case.S
    xg, yg, zg = torch.linspace(-1, 1, W).to(dtype), torch.linspace(1, -1, H).to(dtype), case.zg.to(dtype)
    # the wrong rule "shift": sample s is fetched at the depth of sample s + 1 and reported at its own (shifting positions AND
    # depths together would only rename the samples: the ends of a ray that crosses the whole box lie outside it)
    z_at = zg + (zg[1] - zg[0]) if variant == "shift" else zg
    zc = torch.tensor(case.zc, dtype=dtype)
    x, y = xg.view(1, W).expand(H, W), yg.view(H, 1).expand(H, W)
    nrm = torch.sqrt(x * x + y * y + zc * zc)
    d = torch.stack([x / nrm, y / nrm, zc / nrm], -1)                                        # (H,W,3)
    p = d.view(1, H, W, 1, 3) * z_at.view(1, 1, 1, S, 1)                                      # camera space
    R, t = M[:, :3, :3].view(b, 1, 1, 1, 3, 3), M[:, :3, 3].view(b, 1, 1, 1, 3)
    world = (R * p.unsqueeze(-2)).sum(-1) + t                                                # (b,H,W,S,3)
    lo, hi = torch.tensor(case.lo, dtype=dtype), torch.tensor(case.hi, dtype=dtype)
    top = (n - 1).to(dtype)
    inv_h = top / (hi - lo)
    u = (world - lo) * inv_h
    inside = ((u >= 0) & (u <= top)).all(-1)                                                 # (b,H,W,S)
    cell = torch.minimum(torch.floor(u).clamp_min(0).long(), (n - 2).expand_as(u)).clamp_min(0)
    cell = torch.where(inside.unsqueeze(-1), cell, torch.zeros_like(cell))                   # any valid index for the gather
    tt = u - cell.to(dtype)
    bi = (torch.arange(b) if Bv == b and Bv > 1 else torch.zeros(b, dtype=torch.long)).view(b, 1, 1, 1).expand(b, H, W, S)
    i, j, k = cell.unbind(-1)
    if variant == "nearest":
        near_node = torch.minimum(torch.round(u).clamp_min(0).long(), (n - 1).expand_as(u))
        near_node = torch.where(inside.unsqueeze(-1), near_node, torch.zeros_like(near_node))
        v = _gather(vol, bi, *near_node.unbind(-1))
    else:
        lerp = lambda a_, b_, w_: a_ + w_.unsqueeze(-1) * (b_ - a_)
        tx, ty, tz = tt.unbind(-1)
        c = [[lerp(_gather(vol, bi, i + di, j + dj, k), _gather(vol, bi, i + di, j + dj, k + 1), tz) for dj in (0, 1)]
             for di in (0, 1)]
        v = lerp(lerp(c[0][0], c[0][1], ty), lerp(c[1][0], c[1][1], ty), tx)
    v = torch.where(inside.unsqueeze(-1), v, torch.zeros_like(v))                            # (b,H,W,S,4)
    col, sigma = v[..., :3], v[..., 3]

    if bars:
        A = (R.abs() * p.abs().unsqueeze(-2)).sum(-1) + t.abs()
        e_pos = 12 * eps * A
        e_u = inv_h * (e_pos + eps * (world.abs() + lo.abs())) + 4 * eps * u.abs()            # (b,H,W,S,3)
        within = ((u >= -e_u) & (u <= top + e_u)).all(-1)
        at_face = ((u.abs() <= e_u) | ((u - top).abs() <= e_u)).any(-1)
        near = (within & at_face).any(-1)                                                    # (b,H,W)
        rng, mag = _neighbourhood(vol)
        e_v = _gather(rng, bi, i, j, k) * e_u.sum(-1, keepdim=True) + 12 * eps * _gather(mag, bi, i, j, k)
        e_v = torch.where(inside.unsqueeze(-1), e_v, torch.zeros_like(e_v))
        e_col, e_sigma = e_v[..., :3], e_v[..., 3]

    dens = F.softplus(sigma) if case.clamp_mode == 'softplus' else F.relu(sigma)
    one = torch.ones((), dtype=dtype)
    T = torch.ones(b, H, W, dtype=dtype)
    rgb, depth, opa = torch.zeros(b, H, W, 3, dtype=dtype), torch.zeros(b, H, W, dtype=dtype), torch.zeros(b, H, W, dtype=dtype)
    if bars:
        e_T = torch.zeros_like(T)
        b_rgb, b_depth, b_opa = torch.zeros_like(rgb), torch.zeros_like(depth), torch.zeros_like(opa)
        m_rgb, m_depth, m_opa = torch.zeros_like(rgb), torch.zeros_like(depth), torch.zeros_like(opa)   # sums of magnitudes
    for s in range(S):
        delta = (zg[s + 1] - zg[s]) if s + 1 < S else torch.tensor(1e10, dtype=dtype)
        xx = delta * dens[..., s]
        E = torch.exp(-xx)
        alpha = one - E
        w = alpha * T
        if bars:
            e_dens = e_sigma[..., s]
            if case.clamp_mode != 'softplus':                # relu's dead zone: no error where sigma + e_sigma <= 0
                e_dens = torch.minimum(e_dens, F.relu(sigma[..., s] + e_dens))
            e_dens = e_dens + 4 * eps * dens[..., s]
            e_x = delta * e_dens + 2 * eps * xx
            live = ((xx > 0) | (e_x > 0)).to(dtype)
            e_alpha = (E * torch.expm1(e_x.clamp_max(50.)) + 4 * eps * live).clamp_max(1.)
            e_w = e_alpha * T + alpha * e_T + e_alpha * e_T + 2 * eps * w
            e_f = e_alpha + (2 * eps + 1e-10) * live
            f = one - alpha + 1e-10
            e_T = e_T * f + T * e_f + e_T * e_f + 2 * eps * T * f * live
            cs, zs = col[..., s, :].abs(), zg[s].abs()
            b_opa = b_opa + e_w
            b_depth = b_depth + e_w * zs
            b_rgb = b_rgb + e_w.unsqueeze(-1) * cs + (w + e_w).unsqueeze(-1) * e_col[..., s, :]
            m_opa, m_depth, m_rgb = m_opa + w, m_depth + w * zs, m_rgb + w.unsqueeze(-1) * cs
        rgb = rgb + w.unsqueeze(-1) * col[..., s, :]
        depth = depth + w * zg[s]
        opa = opa + w
        T = T * (one - alpha + 1e-10)
    extra = one - opa
    if bars:
        e_extra = b_opa + (S + 4) * eps * m_opa + eps * (1 + extra.abs())
    if case.last_back:
        if variant != "no_top_up":           # the wrong rule: the last weight's top-up reaches the depth but not the colour
            rgb = rgb + extra.unsqueeze(-1) * col[..., S - 1, :]
        depth = depth + extra * zg[S - 1]
        if bars:
            cl = col[..., S - 1, :].abs()
            b_rgb = b_rgb + e_extra.unsqueeze(-1) * cl + (extra.abs() + e_extra).unsqueeze(-1) * e_col[..., S - 1, :]
            b_depth = b_depth + e_extra * zg[S - 1].abs()
            m_rgb, m_depth = m_rgb + extra.abs().unsqueeze(-1) * cl, m_depth + extra.abs() * zg[S - 1].abs()
    if case.white_back:
        rgb = rgb + extra.unsqueeze(-1)
        if bars:
            b_rgb = b_rgb + e_extra.unsqueeze(-1)
            m_rgb = m_rgb + extra.abs().unsqueeze(-1)
    out = SimpleNamespace(rgb=rgb.permute(0, 3, 1, 2).contiguous(), depth=depth.unsqueeze(1), opacity=opa.unsqueeze(1),
                          sees=inside.any(-1))
    if bars:
        out.bar_rgb = (b_rgb + (S + 4) * eps * m_rgb).permute(0, 3, 1, 2).contiguous()
        out.bar_depth = (b_depth + (S + 4) * eps * m_depth).unsqueeze(1)
        out.bar_opacity = (b_opa + (S + 4) * eps * m_opa).unsqueeze(1)
        out.near = near
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the fp64 oracle of a case with its bars: computed once, shared, never modified"""
    return render(cases()[name], bars=True)


def compare(ref, rgb, depth, opacity):
    """outputs of any dtype / device against reference() -> SimpleNamespace(rgb, depth, opacity: the largest |err| / bar over the
    pixels that are not near (0 where err and bar are both 0, inf where only the bar is), over (b,H,W): err > bar per pixel for
    any output, near pixels False)"""
    keep = ~ref.near.unsqueeze(1)
    worst, over = {}, torch.zeros_like(ref.near)
    for name, got, want, bar in (("rgb", rgb, ref.rgb, ref.bar_rgb), ("depth", depth, ref.depth, ref.bar_depth),
                                 ("opacity", opacity, ref.opacity, ref.bar_opacity)):
        err = (got.detach().cpu().double() - want).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
        ratio = torch.where(keep.expand_as(ratio), ratio, torch.zeros_like(ratio))
        worst[name] = float(ratio.max()) if ratio.numel() else 0.0
        over |= (ratio > 1).any(1)
    return SimpleNamespace(over=over, **worst)
