"""Test infrastructure (like mesh_oracle.py): the iso-surface ray search of cips_siren_surface_x3, stated in vectorised torch for
any density callable and any dtype.  This is the normative statement of the rule of DESIGN.md section 3 "Surface ray casting";
the HIP kernel is compared against it — decisions exactly, depths to the width of the final bracket — and its own debug trace is
replayed through it bit for bit (fp32: every operation below rounds once, as the kernel's do).

Per ray, with zg the S unjittered depths and sigma(t) the density at the point of depth t:
  coarse  s = 0, 1, ...: sigma(zg[0]) >= level -> hit 2 (the ray starts inside), depth zg[0]; else the first s >= 1 with
          sigma(zg[s-1]) < level <= sigma(zg[s]) -> hit 1, bracket [lo, hi] = [zg[s-1], zg[s]]; none -> hit 0, depth zg[S-1];
          a ray that has found its crossing no longer changes
  refine  `refine` times on a hit-1 ray: mid = 0.5 * (lo + hi); sigma(mid) >= level -> hi = mid, else lo = mid
  secant  depth = lo + (level - sigma_lo) / (sigma_hi - sigma_lo) * (hi - lo)
NaN compares false everywhere, as in the kernel."""
from types import SimpleNamespace

import torch


def search(evaluate, zg, level, refine, shape):
    """evaluate(t, slot) -> sigma, both of `shape`, for the depths t of evaluation `slot` (0..S-1 the coarse walk, S + k the
    bisection step k); zg (S,) in the dtype of the search; level a number (converted to that dtype).
    -> SimpleNamespace(hit int64 0 / 1 / 2, index int64 (the s of the coarse bracket [zg[s-1], zg[s]], -1 without one), depth,
    lo, hi, slo, shi (the final bracket and the densities at its ends; meaningful where hit == 1), visited: a list of
    (t, sigma, own) per slot, own = the ray's own search made this evaluation (a ray that is decided evaluates nothing more;
    the kernel's wave goes on for its other rays))"""
    S, dt = zg.numel(), zg.dtype
    level = torch.as_tensor(level, dtype=dt)
    hit = torch.full(shape, -1, dtype=torch.int64)
    index = torch.full(shape, -1, dtype=torch.int64)
    lo = zg[0].expand(shape).clone()
    hi, depth = lo.clone(), lo.clone()
    slo, shi = torch.zeros(shape, dtype=dt), torch.zeros(shape, dtype=dt)
    visited = []
    for s in range(S):
        t = zg[s].expand(shape)
        sig = evaluate(t, s)
        searching = hit < 0
        visited.append((t, sig, searching.clone()))
        if s == 0:
            decided = searching & (sig >= level)
            hit[decided] = 2
        else:
            decided = searching & (slo < level) & (level <= sig)
            hit[decided] = 1
            index[decided] = s
            hi, shi = torch.where(decided, t, hi), torch.where(decided, sig, shi)
        cont = searching & ~decided
        lo, slo = torch.where(cont, t, lo), torch.where(cont, sig, slo)
    none = hit < 0
    hit[none] = 0
    depth = torch.where(none, zg[S - 1].expand(shape), depth)
    one = hit == 1
    for k in range(refine):
        t = torch.where(one, 0.5 * (lo + hi), depth)
        sig = evaluate(t, S + k)
        visited.append((t, sig, one.clone()))
        up = one & (sig >= level)
        dn = one & ~(sig >= level)
        hi, shi = torch.where(up, t, hi), torch.where(up, sig, shi)
        lo, slo = torch.where(dn, t, lo), torch.where(dn, sig, slo)
    f = ((level - slo).double() / (shi - slo).double()).to(dt)       # a correctly rounded quotient in fp32 too, on any host
    depth = torch.where(one, lo + f * (hi - lo), depth)
    return SimpleNamespace(hit=hit, index=index, depth=depth, lo=lo, hi=hi, slo=slo, shi=shi, visited=visited)


def camera_rays(xg, yg, zc, cam2world, dtype):
    """the rays of the pixel grids xg (W), yg (H) (ray = row * W + col), zc = -1 / tan(fov / 2) and cam2world (b,4,4), in
    `dtype`: origin (b,1,3), world directions (b,n,3) — the camera-space direction normalised, then rotated"""
    x = xg.to(dtype).view(1, -1).expand(yg.numel(), -1).reshape(-1)
    y = yg.to(dtype).view(-1, 1).expand(-1, xg.numel()).reshape(-1)
    d = torch.stack([x, y, torch.full_like(x, zc)], -1)
    d = d / d.norm(dim=-1, keepdim=True)
    M = cam2world.to(dtype)
    return M[:, None, :3, 3], torch.einsum('bij,nj->bni', M[:, :3, :3], d)


def surface_search(sigma_fn, origin, dirs, zg, level, refine):
    """search() along the rays origin (b,1,3) + dirs (b,n,3) * t for a density sigma_fn(points (b,P,3)) -> (b,P), in zg's dtype"""
    b, n, _ = dirs.shape
    return search(lambda t, slot: sigma_fn(origin + dirs * t.unsqueeze(-1)), zg, level, refine, (b, n))


def fma32(a, b, c):
    """fmaf(a, b, c) of fp32 tensors, exactly: the product is exact in fp64, the sum is rounded to odd there (TwoSum gives the
    rounding error's sign), and 53 bits rounded to odd round to fp32 like the exact value does"""
    p, cd = a.double() * b.double(), c.double().expand(torch.broadcast_shapes(a.shape, b.shape, c.shape))
    s = p + cd
    bb = s - p
    e = (p - (s - bb)) + (cd - bb)
    si = s.contiguous().view(torch.int64)
    step = torch.where((e > 0) == (s > 0), 1, -1)
    si = torch.where((e != 0) & ((si & 1) == 0), si + step, si)
    return si.view(torch.float64).float()


def kernel_rays(xg, yg, zc, cam2world):
    """camera_rays in fp32 with the roundings of the kernel's ray set-up (gen_point_materialised's zvals form, raygen.h): every
    product and sum rounded on its own except the written-out fmaf chains -> origin (b,1,3), directions (b,n,3), CPU fp32"""
    xg, yg, M = xg.float().cpu(), yg.float().cpu(), cam2world.float().cpu()
    x = xg.view(1, -1).expand(yg.numel(), -1).reshape(1, -1)
    y = yg.view(-1, 1).expand(-1, xg.numel()).reshape(1, -1)
    z = torch.tensor(zc, dtype=torch.float32)
    # square root and quotients through fp64 and back: correctly rounded fp32 results by construction (53 >= 2 * 24 + 2 bits),
    # which the GPU's are — torch's own fp32 sqrt on the CPU is 1 ulp off on some hosts
    nrm = torch.sqrt(((x * x + y * y) + z * z).double()).float()
    dx, dy, dz = ((v.double() / nrm.double()).float() for v in (x, y, z))
    m = lambda i: M[:, i // 4, i % 4].view(-1, 1)
    rx = fma32(dz, m(2), fma32(dy, m(1), dx * m(0)))
    ry = fma32(dz, m(6), fma32(dx, m(4), dy * m(5)))
    rz = fma32(dz, m(10), fma32(dx, m(8), dy * m(9)))
    return M[:, None, :3, 3], torch.stack([rx, ry, rz], -1)


def kernel_points(origin, dirs, t):
    """the kernel's point at depth t (b,n[,k]) of the rays of kernel_rays: fmaf(direction, t, origin) per component -> (..., 3)"""
    while origin.dim() < t.dim() + 1:
        origin, dirs = origin.unsqueeze(-2), dirs.unsqueeze(-2)
    return torch.stack([fma32(dirs[..., i].expand(t.shape), t, origin[..., i].expand(t.shape)) for i in range(3)], -1)
