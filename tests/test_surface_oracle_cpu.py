"""CPU: the yardstick of the surface ray cast (tests/surface_oracle.py) on a field whose answer is known in closed form —
sigma(p) = r0 - |p - c|, whose level set sigma = level is the sphere of radius r0 - level around c — and the exact fmaf the GPU
test rebuilds the kernel's points with."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import surface_oracle as so
from oracle import cips3d_oracle as orc

FOV, T0, T1 = 12, 0.88, 1.12


def _rays(b, img, S, seed):
    g = torch.Generator().manual_seed(seed)
    r = orc.rays(b, img, FOV, T0, T1, S, torch.full((b, img * img, S, 1), 0.5), torch.randn(b, 1, generator=g),
                 torch.randn(b, 1, generator=g), 0.3, 0.155)
    zg = torch.linspace(T0, T1, S, dtype=torch.float64)
    return r["origins"][:, :1].double(), r["dirs"].double(), zg


def _sphere(c, r0):
    return lambda p: r0 - (p - c).norm(dim=-1)


def _roots(origin, dirs, c, R):
    """depths of the two intersections of origin + dirs * t (unit dirs) with the sphere |p - c| = R; NaN where there is none"""
    oc = origin - c
    bq = (oc * dirs).sum(-1)
    disc = bq * bq - ((oc * oc).sum(-1) - R * R)
    root = torch.sqrt(torch.where(disc >= 0, disc, torch.full_like(disc, float("nan"))))
    return -bq - root, -bq + root


@pytest.mark.parametrize("refine", [0, 3, 8])
@pytest.mark.parametrize("centre_depth,R", [(1.0, 0.05), (0.9, 0.06)])
def test_sphere_depth_mask_and_bracket(centre_depth, R, refine):
    """a sphere in front of the camera (rays miss or hit) and one that contains the start of the central rays (mask 2).  A ray is
    judged where the closed form leaves no doubt: it misses the sphere (mask 0), its first depth is inside (mask 2), or its chord
    is at least one coarse step long, so that a sample falls inside (mask 1, and the first crossing's bracket holds exactly the
    entry root).  Depth: within the final bracket's width step / 2^refine of the entry root — the root and the secant point both
    lie in that bracket."""
    b, img, S = 2, 16, 12
    origin, dirs, zg = _rays(b, img, S, 3)
    step = float(zg[1] - zg[0])
    r0, level = 0.5, 0.5 - R
    c = origin + centre_depth * dirs[:, (img // 2) * img + img // 2].unsqueeze(1)      # on the central ray
    out = so.surface_search(_sphere(c, r0), origin, dirs, zg, level, refine)
    t_in, t_out = _roots(origin, dirs, c, R)
    miss = torch.isnan(t_in) | (t_out < T0) | (t_in > T1)
    inside = (t_in <= T0) & (T0 < t_out)
    clear = ~miss & ~inside & (t_in > T0) & (t_out < T1) & (t_out - t_in >= step)
    assert int(miss.sum()) > 20 and (int(clear.sum()) > 20 or centre_depth < 0.95)
    assert bool((out.hit[miss] == 0).all()) and bool((out.depth[miss] == zg[-1]).all())
    assert bool((out.hit[clear] == 1).all())
    if centre_depth < 0.95:
        assert int(inside.sum()) > 5
        assert bool((out.hit[inside] == 2).all()) and bool((out.depth[inside] == zg[0]).all())
    else:
        assert not bool(inside.any())
    k = out.index[clear]
    assert bool((zg[k - 1] < t_in[clear]).all()) and bool((t_in[clear] <= zg[k]).all())
    if not bool(clear.any()):
        return
    err = (out.depth[clear] - t_in[clear]).abs()
    print(f"sphere R={R} refine={refine}: max |depth - root| {float(err.max()):.3e}, bracket {step / 2 ** refine:.3e}")
    assert float(err.max()) <= step / 2 ** refine
    assert bool(((out.hi - out.lo)[clear] <= step / 2 ** refine * (1 + 1e-12)).all())
    assert len(out.visited) == S + refine
    if refine == 0:                                     # the pure secant step on the coarse bracket
        sig = torch.stack([v[1] for v in out.visited[:S]], -1)[clear]
        s0, s1 = sig.gather(-1, (k - 1).unsqueeze(-1)).squeeze(-1), sig.gather(-1, k.unsqueeze(-1)).squeeze(-1)
        assert torch.equal(out.depth[clear], zg[k - 1] + (level - s0) / (s1 - s0) * (zg[k] - zg[k - 1]))


def test_a_decided_ray_no_longer_changes_and_nan_compares_false():
    """two crossings along a ray: the first one is kept; a NaN density is neither inside nor a crossing"""
    zg = torch.linspace(0., 1., 6, dtype=torch.float64)
    table = torch.tensor([[0., 2., 0., 3., 0., 0.],                # crosses 1.0 at step 1 and again at step 3
                          [float("nan"), 0., 2., 0., 0., 0.],      # NaN at the start: not inside; crossing at step 2
                          [0., float("nan"), 2., 0., 0., 0.],      # NaN before a high value: NaN < level is false, no crossing there
                          [5., 0., 0., 0., 0., 0.]], dtype=torch.float64)
    out = so.search(lambda t, slot: table[:, slot], zg, 1.0, 0, (4,))
    assert out.hit.tolist() == [1, 1, 0, 2] and out.index.tolist() == [1, 2, -1, -1]
    assert float(out.depth[0]) == pytest.approx(0.1) and float(out.depth[2]) == 1.0 and float(out.depth[3]) == 0.0
    assert [bool(v[2][0]) for v in out.visited] == [True, True, False, False, False, False]


def _round32(q):
    """the fp32 nearest to the rational q, ties to the even mantissa"""
    f = np.float32(float(q))
    cands = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    errs = sorted((abs(Fraction(float(v)) - q), int(np.float32(v).view(np.int32)) & 1, float(v)) for v in cands)
    return errs[0][2]


def test_fma32_is_the_exact_fused_multiply_add():
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(4000, generator=g), torch.randn(4000, generator=g)
    c = -(a.double() * b.double()).float() * (1 + torch.randn(4000, generator=g) * 1e-7)          # heavy cancellation
    c[::3] = torch.randn(4000, generator=g)[::3]
    got = so.fma32(a, b, c)
    for i in range(0, 4000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        assert float(got[i]) == _round32(exact), i
