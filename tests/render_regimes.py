"""Inputs for the renderer tests in the regimes a trained generator renders: opaque surfaces, rays that go dark behind a wall,
empty background rays, exact zeros at the relu gate, softplus at both ends of its range.  A plain module (no fixtures): the
CPU file tests/test_render_regimes_cpu.py checks on the oracle that every class does what its name says, the GPU file
tests/test_gpu_render_regimes.py feeds the same tensors to the kernels.

A ray's class is its index within the image mod 6 (CLASSES order).  With k = S // 2:

  surface    x <= -1 in front of k; x[k] * delta >= 20 for the smallest delta build() can make, so alpha_k = 1 - exp(-20) rounds
             to 1.0f (exp(-20) = 2e-9 < 2^-25); as drawn behind k.  One weight of ~1, everything behind it sees T = 1e-10.
  wall       such values at every sample from k on; as drawn in front.  T loses ten decades per sample: (float)T == 0 after
             five of them (1e-50 < 1.4e-45, the smallest fp32 subnormal), so the samples behind have x > 0 and w == 0.
  empty      every x <= -1: all weights 0, sum 0; last_back / white_back add exactly 1.
  last_only  empty, but x[S-1] = 0.37: delta_last = 1e10, alpha_last = 1 and T = 1 there, so w_last == 1.
  zeros      +0.0 at the even positions, then -0.0 at every third one (0, 3, 6, ...); as drawn elsewhere.
  thin       as drawn, N(0, 3^2): the regime of the older tests, as a control.

No class had to be changed for the reference's sake: the fp32 oracle's gradients are finite on all of them (asserted by the
CPU file)."""
import torch

CLASSES = ("surface", "wall", "empty", "last_only", "zeros", "thin")
Z0, Z1 = 0.88, 1.12
JITTER = 0.4            # of the mean spacing (Z1 - Z0) / S
OPAQUE = 20.0           # x * delta of an opaque sample, at least
LAST_ONLY_X = 0.37


def min_delta(S):
    """the smallest spacing of two neighbouring depths build() can make: the grid's step minus twice the largest jitter"""
    return (Z1 - Z0) / (S - 1) - 2 * JITTER * (Z1 - Z0) / S


def depths(b, n, S, g):
    grid = torch.linspace(Z0, Z1, S).view(1, 1, S)
    return grid + (torch.rand(b, n, S, generator=g) * 2 - 1) * (JITTER * (Z1 - Z0) / S)


def ray_classes(b, n):
    """(b, n) long: index into CLASSES"""
    return (torch.arange(n) % len(CLASSES)).view(1, n).expand(b, n).contiguous()


def build(b, n, S, seed):
    """-> dict(x (b, n, S) pre-activations, z (b, n, S) depths, ascending along a ray, cls (b, n) long)"""
    g = torch.Generator().manual_seed(seed)
    z = depths(b, n, S, g)
    drawn = torch.randn(b, n, S, generator=g) * 3
    opaque = OPAQUE / min_delta(S) * (1 + 0.5 * torch.rand(b, n, S, generator=g))
    clamped = -1 - drawn.abs()
    cls = ray_classes(b, n)
    k = S // 2
    pos = torch.arange(S).view(1, 1, S).expand(b, n, S)
    c = cls.view(b, n, 1).expand(b, n, S)
    x = drawn.clone()

    def put(name, where, value):
        m = (c == CLASSES.index(name)) & where
        x[m] = value[m] if torch.is_tensor(value) else value

    put("surface", pos < k, clamped)
    put("surface", pos == k, opaque)
    put("wall", pos >= k, opaque)
    put("empty", pos >= 0, clamped)
    put("last_only", pos < S - 1, clamped)
    put("last_only", pos == S - 1, LAST_ONLY_X)
    put("zeros", pos % 2 == 0, 0.0)
    put("zeros", pos % 3 == 0, -0.0)
    return dict(x=x, z=z, cls=cls)


SOFT_HI, SOFT_LO = 25.0, -110.0     # above F.softplus's threshold of 20; exp(-110) = 1.7e-48 is 0 in fp32


def build_softplus(b, n, S, seed):
    """the same depths with softplus pre-activations: N(0, 3^2), SOFT_HI where (ray + sample) % 4 == 0, SOFT_LO where it is 2,
    and SOFT_LO at every sample of the rays with index % 6 == 2 ("void": density, weights and gradient are exactly 0 in fp32)
    -> dict(x, z, void (b, n) bool)"""
    g = torch.Generator().manual_seed(seed)
    z = depths(b, n, S, g)
    x = torch.randn(b, n, S, generator=g) * 3
    ray = torch.arange(n).view(1, n, 1).expand(b, n, S)
    ph = (ray + torch.arange(S).view(1, 1, S)) % 4
    x[ph == 0] = SOFT_HI
    x[ph == 2] = SOFT_LO
    void = ray % 6 == 2
    x[void] = SOFT_LO
    return dict(x=x, z=z, void=void[..., 0].contiguous())


def is_class(r, name):
    return r["cls"] == CLASSES.index(name)


def min_gate_margin(r):
    """the smallest |x| over the samples whose gate the GPU tests leave unpinned: everything but the zeros class's zeros"""
    x = r["x"].double().abs()
    x = torch.where((r["x"] == 0) & is_class(r, "zeros").unsqueeze(-1), torch.full_like(x, float("inf")), x)
    return float(x.min())


# ---- the seeds every test uses: picked so that min_gate_margin >= 1e-4 (asserted by the CPU file) ----
SEED_COARSE = 101
SEED_FINE = 202
SEED_SOFT = 303
SEED_SOFT_FINE = 404
B, N = 2, 67
FLAT_S = (3, 9, 24)
HIER_S = (9, 24, 48)


# --------------------------------------------------------------------------------------
# the references: oracle.integrate / oracle.fine_points on these inputs, in the precision asked for
# --------------------------------------------------------------------------------------
def features(b, n, S, seed):
    """-> feat (b, n, S, 32), upstream gradient up (b, n, 32)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, n, S, 32, generator=g), torch.randn(b, n, 32, generator=g)


def oracle_composite(feat, x, z, up, clamp, flags, dtype, noise=None, noise_std=0.0):
    """oracle.integrate forward + backward of sum(fea * up) on feat (b, n, E, 32), x / z / noise (b, n, E), already in compositing
    order -> dict(fea, depth, w, dfeat, dx) in `dtype`"""
    from oracle import cips3d_oracle as orc
    f = feat.to(dtype).clone().requires_grad_(True)
    s = x.to(dtype).clone().requires_grad_(True)
    nz = (noise if noise is not None else torch.zeros_like(x)).to(dtype).unsqueeze(-1)
    fea, depth, w = orc.integrate(torch.cat([f, s.unsqueeze(-1)], -1), z.to(dtype).unsqueeze(-1), nz, noise_std, clamp_mode=clamp,
                                  last_back=bool(flags & 1), white_back=bool(flags & 2))
    (fea * up.to(dtype)).sum().backward()
    return dict(fea=fea.detach(), depth=depth.detach().squeeze(-1), w=w.detach().squeeze(-1), dfeat=f.grad, dx=s.grad)


def oracle_resample(x, z, u, dtype, clamp="relu"):
    """oracle.fine_points on pre-activations x, depths z (b, n, S) and draws u (b * n, S) -> fine_z (b * n, S), book (weights
    (b * n, S), cdf (b * n, S - 1), inds (b * n, S))"""
    from oracle import cips3d_oracle as orc
    b, n, S = x.shape
    coarse = torch.zeros(b, n, S, 33, dtype=dtype)
    coarse[..., 32] = x.to(dtype)
    zero = torch.zeros(b, n, 3, dtype=dtype)
    with torch.no_grad():
        _, fz, book = orc.fine_points(coarse, z.to(dtype).unsqueeze(-1), torch.zeros(b, n, S, 1, dtype=dtype), 0.0, u.to(dtype),
                                      zero, zero, clamp)
    book["weights"] = book["weights"].reshape(b * n, S)
    return fz.reshape(b * n, S), book


def uniform_draws(R, S, seed):
    return torch.rand(R, S, generator=torch.Generator().manual_seed(seed))


SEED_U = 505


def resample_distance(fz, inds, fz64, inds64):
    """(share of indices that differ from the fp64 oracle's, max |fine_z - fine_z64| / max |fine_z64| where they agree)"""
    good = inds.cpu() == inds64
    a, r = fz.detach().double().cpu()[good], fz64[good]
    return float((~good).double().mean()), float((a - r).abs().max() / r.abs().max())


# --------------------------------------------------------------------------------------
# the fused march: the class pre-activations ride on the noise input (noise_std = 1), the depths on the jitter input
# --------------------------------------------------------------------------------------
MARCH_CASES = [(8, 8, 24, 0, 611), (5, 8, 9, 3, 622)]      # H, W, S, flags, seed
MARCH_B = 3


def build_march(H, W, S, flags, seed):
    """-> dict(noise (3, n, S), jitter (3, n, S) uniforms that reproduce build()'s depths, cls (3, n), style (3, 128), theta, phi
    (3, 1), up (3, n, 32)).  In the flags-0 case every ray of image 0 is of class empty."""
    n = H * W
    r = build(MARCH_B, n, S, seed)
    x, cls = r["x"], r["cls"]
    if flags == 0:
        x[0] = -1 - x[0].abs()
        cls[0] = CLASSES.index("empty")
    grid = torch.linspace(Z0, Z1, S)
    jitter = 0.5 + (r["z"] - grid.view(1, 1, S)) / (grid[1] - grid[0])
    assert float(jitter.min()) > 0.05 and float(jitter.max()) < 0.95
    g = torch.Generator().manual_seed(seed + 1)
    return dict(noise=x, jitter=jitter, cls=cls, style=torch.randn(MARCH_B, 128, generator=g), theta=torch.randn(MARCH_B, 1, generator=g),
                phi=torch.randn(MARCH_B, 1, generator=g), up=torch.randn(MARCH_B, n, 32, generator=g))


FOV = 12


def _rays64(orc, b, H, W, S, m):
    """oracle.rays for an H x W image (the oracle's is square): its camera matrix, and its ray / jitter / transform steps
    restated on the row-major pixel grid -> dict(points (b, n, S, 3), z (b, n, S, 1), cam2world)"""
    import math
    c2w = orc.rays(b, 2, FOV, Z0, Z1, S, torch.full((b, 4, S, 1), 0.5), m["theta"].double(), m["phi"].double(), 0.3, 0.155)["cam2world"]
    x = torch.linspace(-1, 1, W).view(1, W).expand(H, W).reshape(-1)
    y = torch.linspace(1, -1, H).view(H, 1).expand(H, W).reshape(-1)
    zc = -torch.ones_like(x) / math.tan((2 * math.pi * FOV / 360) / 2)
    d = torch.stack([x, y, zc], -1)
    d = d / d.norm(dim=-1, keepdim=True)                                    # (n, 3)
    grid = torch.linspace(Z0, Z1, S)
    z = grid.view(1, 1, S) + (m["jitter"].double() - 0.5) * (grid[1] - grid[0])           # (b, n, S)
    cam = d.view(1, -1, 1, 3) * z.unsqueeze(-1)
    pts = torch.einsum("bij,bnsj->bnsi", c2w[:, :3, :3], cam) + c2w[:, :3, 3].view(b, 1, 1, 3)
    return dict(points=pts, z=z.unsqueeze(-1), cam2world=c2w)


def oracle_march64(G, m, H, W, S, flags):
    """rays -> siren -> integrate in fp64 on the parameters of generator G (left untouched) -> dict(out (b, n, S, 33), z, x = sigma +
    noise, fea, depth, w, grads {siren parameter name: gradient}, dstyle) for the loss sum(fea * up)"""
    from oracle import cips3d_oracle as orc
    b, n = MARCH_B, H * W
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in G.named_parameters() if k.startswith("siren.")}
    style = m["style"].double().clone().requires_grad_(True)
    torch.set_default_dtype(torch.float64)
    try:
        r = _rays64(orc, b, H, W, S, m)
        out = orc.siren(sd, r["points"].reshape(b, n * S, 3), style).reshape(b, n, S, 33)
        noise = m["noise"].double().unsqueeze(-1)
        fea, depth, w = orc.integrate(out, r["z"], noise, 1.0, clamp_mode="relu", last_back=bool(flags & 1), white_back=bool(flags & 2))
        (fea * m["up"].double()).sum().backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return dict(out=out.detach(), z=r["z"].squeeze(-1), x=(out[..., 32] + noise[..., 0]).detach(), fea=fea.detach(),
                depth=depth.detach().squeeze(-1), w=w.detach().squeeze(-1), cam2world=r["cam2world"],
                grads={k[len("siren."):]: v.grad for k, v in sd.items()}, dstyle=style.grad)
