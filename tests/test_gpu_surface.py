"""GPU: the surface ray cast — siren_surface_x3_kernel (cips_siren_surface_x3): its densities against the sigma kernel and its
decisions against its own debug trace BIT FOR BIT (points rebuilt on the host with an exact fmaf, the search rule replayed in
torch: tests/surface_oracle.py), hit mask, bracket and depth against the fp64 oracle on the rays no rounding can decide
differently, the degenerate levels, and the Python entry points on top of it (ops.siren_surface, ops.siren_surface_composed,
NeRFNetwork.surface_rays, GeneratorNerfINR.surface, evaluation.shade_surface)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import surface_oracle as so
from conftest import seeded_generator
from oracle import cips3d_oracle as orc
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
FOV, T0, T1 = 12, 0.88, 1.12
ZC = float((-torch.ones(1) / np.tan((2 * math.pi * FOV / 360) / 2)).item())
BAR = 1e-4            # the project's standing bar for free-running SIREN values (DESIGN sections 0 / 4)
# name -> seed, b, img, S, refines: a ragged last wave (81 rays); the smallest grid (S = 2); 289 rays cross a 256-ray pass
CASES = {"ragged": (5, 2, 9, 12, (6,)), "smallest": (7, 1, 5, 2, (0, 6)), "two_passes": (5, 3, 17, 7, (4,))}
CASE_REFINE = [(name, r) for name, c in CASES.items() for r in c[4]]
# The styles and cameras are drawn from torch.Generator().manual_seed(INPUT_SEED + seed).  Bisection drives sigma(mid) towards the
# level, so its last steps often land within 1e-4 max |sigma| of it: over twelve such seeds the fp64 oracle calls 2.5 % to 8 % of
# the 162 rays of "ragged" (refine 6) ambiguous, around the 5 % cap of test_oracle_leaves_few_rays_to_rounding.  This seed was
# chosen on the oracle alone, on the CPU: 4 of 162, 0 of 25, 7 of 867 ambiguous rays and a miss / hit / inside split of
# 0.44 / 0.43 / 0.12, 0.44 / 0.32 / 0.24 and 0.46 / 0.40 / 0.14.
INPUT_SEED = 109


def _styles(st):
    return {"nerf_w0": st, "nerf_w1": st, "nerf_rgb": st}


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


_CASE, _REF = {}, {}


def _case(name):
    """inputs of one shape, made once on the CPU: the generator, a style per image, one camera per image (orc.rays' gaussian
    camera from two draws), the pixel grids, the rays in fp64 / fp32 and as the kernel rounds them, the oracle's density
    functions, and `level`: the 0.7 quantile of the fp64 oracle's coarse densities, rounded to fp32"""
    if name in _CASE:
        return _CASE[name]
    seed, b, img, S, _ = CASES[name]
    G = seeded_generator(seed)
    g = torch.Generator().manual_seed(INPUT_SEED + seed)
    style = torch.randn(b, 128, generator=g)
    theta, phi = torch.randn(b, 1, generator=g), torch.randn(b, 1, generator=g)
    c2w = orc.rays(b, img, FOV, T0, T1, S, torch.full((b, img * img, S, 1), 0.5), theta, phi, 0.3, 0.155)["cam2world"].contiguous()
    if b > 1:
        assert not torch.equal(c2w[0], c2w[1])
    xg, yg, zg = torch.linspace(-1, 1, img), torch.linspace(1, -1, img), torch.linspace(T0, T1, S)
    c = dict(name=name, G=G, style=style, c2w=c2w, xg=xg, yg=yg, zg=zg, b=b, img=img, n=img * img, S=S, step=(T1 - T0) / (S - 1))
    for dt in (torch.float64, torch.float32):
        sd = {k: v.detach().to(dt) for k, v in G.named_parameters()}
        c[dt] = (*so.camera_rays(xg, yg, ZC, c2w, dt), (lambda sd, st: lambda p: orc.siren(sd, p, st)[..., 32])(sd, style.to(dt)))
    o, d, f = c[torch.float64]
    with torch.no_grad():
        coarse = f((o.unsqueeze(2) + d.unsqueeze(2) * zg.double().view(1, 1, S, 1)).reshape(b, -1, 3))
    c["level"] = float(np.float32(torch.quantile(coarse.flatten(), 0.7)))
    c["smax"] = float(coarse.abs().max())
    c["kernel_rays"] = so.kernel_rays(xg, yg, ZC, c2w)
    _CASE[name] = c
    return c


def _oracle(name, refine, dt):
    """the oracle's search of a case in dtype `dt`, once"""
    key = (name, refine, dt)
    if key not in _REF:
        c = _case(name)
        o, d, f = c[dt]
        with torch.no_grad():
            _REF[key] = so.surface_search(f, o, d, c["zg"].to(dt), c["level"], refine)
    return _REF[key]


def _ambiguous(c, visited):
    """rays whose OWN search visited a density within BAR * max |sigma| of the level"""
    amb = torch.zeros(c["b"], c["n"], dtype=torch.bool)
    for t, sig, own in visited:
        amb |= own & ~((sig - c["level"]).abs() > BAR * c["smax"])          # a NaN density counts as ambiguous
    return amb


def _siren(ops, c):
    Gd = seeded_generator(CASES[c["name"]][0], device=dev())          # the weights of c["G"], which stays on the CPU
    with torch.no_grad():
        args = Gd.siren._siren_args(_styles(c["style"].to(dev())))
    return args


def _geom(c):
    d = dev()
    return (c["b"], c["img"], c["img"], c["S"], ZC), c["xg"].to(d), c["yg"].to(d), c["zg"].to(d), c["c2w"].to(d)


def _raw(ops, t, c, level, refine, sigma=True, points=True, trace=True, null_colour=False):
    """cips_siren_surface_x3 through ctypes into NaN-filled (hit: 255-filled) buffers with 64 trailing sentinels each
    -> dict of the outputs (None where NULL was passed) and of the tails"""
    from cips3d_amd import _lib
    d = dev()
    B, n, S = c["b"], c["n"], c["S"]
    sizes = dict(depth=B * n, sigma=B * n, points=B * n * 3, trace=B * n * (S + refine) * 2)
    buf = {k: torch.full((v + 64,), float("nan"), device=d) for k, v in sizes.items()}
    for k, v in sizes.items():
        buf[k][v:] = SENTINEL
    hit = torch.full((B * n + 64,), 255, dtype=torch.uint8, device=d)
    hit[B * n:] = 77
    geom, xg, yg, zg, c2w = _geom(c)
    sw = ops._siren_struct(t)
    if null_colour:
        for nm in ("wc", "bc", "wf", "bf", "gc", "pc"):
            setattr(sw, nm, None)
    rp = ops._ray_params(xg, yg, zg, ZC, c2w, None, c["img"], c["img"], S)
    _lib.check(_lib.load().cips_siren_surface_x3(C.byref(sw), C.byref(rp), float(level), refine, ops._p(buf["depth"]), ops._p(hit),
                                                 ops._p(buf["sigma"]) if sigma else None, ops._p(buf["points"]) if points else None,
                                                 ops._p(buf["trace"]) if trace else None, B, ops._stream()), "cips_siren_surface_x3")
    torch.cuda.synchronize()
    out = {k: buf[k][:v] for k, v in sizes.items()}
    out = dict(depth=out["depth"].view(B, n), sigma=out["sigma"].view(B, n), points=out["points"].view(B, n, 3),
               trace=out["trace"].view(B, n, S + refine, 2), hit=hit[:B * n].view(B, n))
    tails = {k: buf[k][v:] for k, v in sizes.items()}
    assert all(bool((v == SENTINEL).all()) for v in tails.values()) and bool((hit[B * n:] == 77).all())     # nothing written behind
    return out


def _replay(c, trace, refine):
    """the search rule on the kernel's own trace (CPU fp32) -> the oracle's namespace; the depths the rule asks for at a ray's own
    evaluations must be the trace's, and those entries must not be NaN"""
    tr = trace.cpu()

    def evaluate(t, slot):
        return tr[..., slot, 1]
    out = so.search(evaluate, c["zg"], np.float32(c["level"]), refine, (c["b"], c["n"]))
    for slot, (t, sig, own) in enumerate(out.visited):
        assert bool(torch.isfinite(sig[own]).all()), slot
        assert torch.equal(tr[..., slot, 0][own], t[own]), slot
    return out


@pytest.mark.parametrize("trig", [0, 1, 3])
@pytest.mark.parametrize("name,refine", CASE_REFINE)
def test_kernel_is_exact_against_the_sigma_kernel_and_its_own_trace(name, refine, trig, x3, monkeypatch):
    """no tolerance anywhere: (1) every element is written, nothing behind the buffers; (2) the densities — the final one and
    every trace entry — are ops.siren_sigma's at the kernel's points, which the host rebuilds bit for bit (fmaf(direction, t,
    origin), tests/surface_oracle.py); (3) the search rule replayed on the trace gives the kernel's hit, bracket (the bisection
    depths it asked for) and depth; (4) NULL outputs, NULL colour pointers and a second call change no bit."""
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    c = _case(name)
    args = _siren(ops, c)
    t = ops._siren_prep(args)
    level = c["level"]
    out = _raw(ops, t, c, level, refine)
    B, n, S = c["b"], c["n"], c["S"]
    assert torch.isfinite(out["depth"]).all() and torch.isfinite(out["sigma"]).all() and torch.isfinite(out["points"]).all()
    assert bool((out["hit"] <= 2).all())
    trace = out["trace"]
    assert torch.equal(torch.isnan(trace[..., 0]), torch.isnan(trace[..., 1]))          # a slot is evaluated or it is not
    assert bool(torch.isfinite(trace[:, :, 0]).all())                                    # the first step is everyone's

    # (2) points and densities
    origin, dirs = c["kernel_rays"]
    assert torch.equal(out["points"].cpu(), so.kernel_points(origin, dirs, out["depth"].cpu()))
    assert torch.equal(ops.siren_sigma(out["points"].contiguous(), *args), out["sigma"])
    tt = trace[..., 0].cpu()
    seen = ~torch.isnan(tt)
    pts = so.kernel_points(origin, dirs, torch.where(seen, tt, c["zg"][0]))              # (B, n, S + refine, 3)
    sig = ops.siren_sigma(pts.reshape(B, -1, 3).to(dev()), *args).view(B, n, S + refine)
    assert torch.equal(sig[seen.to(dev())], trace[..., 1][seen.to(dev())])

    # (3) the rule on the trace
    rep = _replay(c, trace, refine)
    assert torch.equal(rep.hit, out["hit"].cpu().long())
    assert torch.equal(rep.depth, out["depth"].cpu())
    frac = [float((rep.hit == k).float().mean()) for k in (0, 1, 2)]
    print(f"surface {name} refine={refine} trig={trig}: miss / hit / inside {frac[0]:.2f} / {frac[1]:.2f} / {frac[2]:.2f}, "
          f"trace slots evaluated {float(seen.float().mean()):.2f}")

    # (4) what must not matter
    for kw in (dict(sigma=False), dict(points=False), dict(trace=False), dict(sigma=False, points=False, trace=False),
               dict(null_colour=True), dict()):
        o2 = _raw(ops, t, c, level, refine, **kw)
        assert torch.equal(o2["depth"], out["depth"]) and torch.equal(o2["hit"], out["hit"]), kw
        for k in ("sigma", "points", "trace"):
            if kw.get(k, True):
                assert torch.equal(o2[k].view(torch.int32), out[k].view(torch.int32)), (kw, k)
            else:
                assert bool(torch.isnan(o2[k]).all()), (kw, k)                           # NULL: not written
    d5 = ops.siren_surface(level, refine, *_geom(c), *args, trace=True)
    assert d5[0].shape == (B, n) and d5[1].dtype == torch.uint8 and d5[3].shape == (B, n, 3) and d5[4].shape == trace.shape
    assert all(v.grad_fn is None and not v.requires_grad for v in d5)
    for got, k in zip(d5, ("depth", "hit", "sigma", "points", "trace")):
        bits = (lambda v: v) if k == "hit" else (lambda v: v.view(torch.int32))            # NaN slots of the trace compare as bits
        assert torch.equal(bits(got), bits(out[k])), k


@pytest.mark.parametrize("name,refine", CASE_REFINE)
def test_oracle_leaves_few_rays_to_rounding(name, refine):
    """the cap of the comparison below, on the oracle alone: at most 5 % of the rays visit a density within 1e-4 max |sigma| of
    the level during their own search; and the level splits the rays into misses, hits and starts-inside"""
    c = _case(name)
    ref = _oracle(name, refine, torch.float64)
    amb = _ambiguous(c, ref.visited)
    frac = [float((ref.hit == k).float().mean()) for k in (0, 1, 2)]
    print(f"oracle {name} refine={refine}: level {c['level']:.4f}, max |sigma| {c['smax']:.2f}, ambiguous {int(amb.sum())} of {amb.numel()}, "
          f"miss / hit / inside {frac[0]:.2f} / {frac[1]:.2f} / {frac[2]:.2f}")
    assert float(amb.float().mean()) <= 0.05
    assert all(f > 0.05 for f in frac)


@pytest.mark.parametrize("trig", [0, 1, 3])
@pytest.mark.parametrize("name,refine", CASE_REFINE)
def test_kernel_against_the_fp64_oracle(name, refine, trig, x3, monkeypatch):
    """on every ray that is not ambiguous (the test above caps them): the oracle's hit mask and bracket index, and a depth within
    the final bracket's width step / 2^refine of the oracle's — both lie in the same bracket.  On every ray both call a hit: the
    fp64 density at the kernel's surface point misses the level by at most the oracle's own residual plus 1e-4 max |sigma|.  The
    fp32 oracle's figures are printed next to the kernel's."""
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    c = _case(name)
    ref, ref32 = _oracle(name, refine, torch.float64), _oracle(name, refine, torch.float32)
    ok = ~_ambiguous(c, ref.visited)
    assert float((~ok).float().mean()) <= 0.05
    args = _siren(ops, c)
    depth, hit, sigma, points, trace = ops.siren_surface(c["level"], refine, *_geom(c), *args, trace=True)
    rep = _replay(c, trace, refine)
    depth, hit = depth.cpu().double(), hit.cpu().long()
    assert torch.equal(hit[ok], ref.hit[ok])
    assert torch.equal(rep.index[ok], ref.index[ok])
    width = c["step"] / 2 ** refine
    err, err32 = (depth - ref.depth).abs()[ok], (ref32.depth.double() - ref.depth).abs()[ok & (ref32.hit == ref.hit)]
    o, d, f = c[torch.float64]
    both = (hit == 1) & (ref.hit == 1)
    both32 = (ref32.hit == 1) & (ref.hit == 1)
    with torch.no_grad():
        res_k = (f(o + d * depth.unsqueeze(-1)) - c["level"]).abs()
        res_o = (f(o + d * ref.depth.unsqueeze(-1)) - c["level"]).abs()
        res_32 = (f(o + d * ref32.depth.double().unsqueeze(-1)) - c["level"]).abs()
    print(f"surface {name} refine={refine} trig={trig}: max |depth - depth64| kernel {float(err.max()):.2e} oracle(fp32) {float(err32.max()):.2e} "
          f"(bracket {width:.2e}) | worst |sigma64(point) - level| kernel {float(res_k[both].max()):.2e} oracle(fp32) "
          f"{float(res_32[both32].max()):.2e} oracle(fp64) {float(res_o[both].max()):.2e} | max |sigma| {c['smax']:.2f}")
    assert float(err.max()) <= width
    assert bool((res_k[both] <= res_o[both] + BAR * c["smax"]).all())


@pytest.mark.parametrize("trig", [0, 3])
def test_degenerate_levels_and_refinement_counts(trig, x3, monkeypatch):
    ops = x3
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    c = _case("ragged")
    args = _siren(ops, c)
    zg = c["zg"].to(dev())
    geom = _geom(c)
    depth, hit, sigma, points = ops.siren_surface(1e30, 5, *geom, *args)                  # above every density: no ray hits
    assert bool((hit == 0).all()) and bool((depth == zg[-1]).all()) and torch.isfinite(sigma).all()
    depth, hit, sigma, points = ops.siren_surface(-1e30, 5, *geom, *args)                 # below every density: all start inside
    assert bool((hit == 2).all()) and bool((depth == zg[0]).all()) and torch.isfinite(sigma).all()
    d0, h0, _, _, tr0 = ops.siren_surface(c["level"], 0, *geom, *args, trace=True)        # refine = 0: the pure secant step
    rep = _replay(c, tr0, 0)
    assert tr0.shape[2] == c["S"] and torch.equal(rep.depth, d0.cpu()) and torch.equal(rep.hit, h0.cpu().long())
    d32, h32, s32, _ = ops.siren_surface(c["level"], 32, *geom, *args)                    # refine = 32: the bracket collapses
    one = rep.hit == 1
    assert int(one.sum()) > 10 and torch.equal(h32, h0) and torch.isfinite(d32).all() and torch.isfinite(s32).all()
    lo, hi = c["zg"][rep.index[one] - 1], c["zg"][rep.index[one]]
    assert bool((lo <= d32.cpu()[one]).all()) and bool((d32.cpu()[one] <= hi).all())
    with pytest.raises(ValueError):
        ops.siren_surface(c["level"], 33, *geom, *args)


def _zs(seed, d, b=2):
    g = torch.Generator().manual_seed(seed)
    return {"z_nerf": torch.randn(b, 256, generator=g).to(d), "z_inr": torch.randn(b, 512, generator=g).to(d)}


KW = dict(img_size=8, fov=FOV, ray_start=T0, ray_end=T1, num_steps=6, h_stddev=0.3, v_stddev=0.155, sample_dist="gaussian")


def _level_of(G, zs):
    """a level that cuts the volume the camera looks at: the median density of a coarse lattice"""
    return float(np.float32(G.density_grid(zs, 9, cube_length=0.2).median().item()))


def test_generator_surface(x3):
    """r8, S = 6, b = 2: shapes and dtypes; the camera, the RNG state and pitch_yaw of the matching forward() / geometry(); points,
    sigma and depth as the kernel wrote them for that camera; unit normals on the surface, exact zeros on the background; psi < 1;
    only the NeRF mapping network runs; shade_surface"""
    from cips3d_amd.evaluation import shade_surface
    ops = x3
    d = dev()
    b, img, S = 2, 8, 6
    n = img * img
    G = seeded_generator(13, device=d)
    G.device = d
    zs = _zs(131, d)
    level = _level_of(G, zs)
    calls, inr = [], G._map_inr
    G._map_inr = lambda z: (calls.append(1), inr(z))[1]
    try:
        torch.manual_seed(7)
        sf = G.surface(zs, level, **KW, refine=5)
        after_sf = (torch.rand(1, device=d), torch.rand(1))
    finally:
        del G._map_inr
    assert not calls
    for nm, ch, dt in (("depth", 1, torch.float32), ("mask", 1, torch.uint8), ("points", 3, torch.float32), ("sigma", 1, torch.float32),
                       ("normals", 3, torch.float32)):
        v = getattr(sf, nm)
        assert v.shape == (b, ch, img, img) and v.dtype == dt and v.grad_fn is None and not v.requires_grad, nm
        assert dt == torch.uint8 or bool(torch.isfinite(v).all()), nm
    assert sf.pitch_yaw.shape == (b, 2)
    torch.manual_seed(7)
    geo = G.geometry(zs, **KW, hierarchical_sample=False)
    torch.manual_seed(7)
    with torch.no_grad():
        _, py = G(zs, **KW, hierarchical_sample=False)
    after_fwd = (torch.rand(1, device=d), torch.rand(1))
    assert torch.equal(sf.pitch_yaw, geo.pitch_yaw) and torch.equal(sf.pitch_yaw, py)
    assert torch.equal(after_sf[0], after_fwd[0]) and torch.equal(after_sf[1], after_fwd[1])

    def rows(v):                     # (b,c,H,W) -> (b,n,c)
        return v.permute(0, 2, 3, 1).reshape(b, n, -1)
    # the same camera by hand: the draws of forward() after that seed are jitter, theta, phi
    torch.manual_seed(7)
    torch.rand((b, n, S, 1), device=d)
    theta, phi = torch.randn((b, 1), device=d), torch.randn((b, 1), device=d)
    _, origin, c2w = ops.camera_pose(theta, phi, False, 0.3, math.pi * 0.5, 0.155, math.pi * 0.5)
    xg, yg, zg = ops.pixel_grids(img, img, S, T0, T1, d)
    with torch.no_grad():
        args = G.siren._siren_args(G._map_nerf(zs["z_nerf"]))
    depth, hit, sigma, points, trace = ops.siren_surface(level, 5, (b, img, img, S, ZC), xg, yg, zg, c2w, *args, trace=True)
    assert torch.equal(rows(sf.depth).squeeze(-1), depth) and torch.equal(rows(sf.mask).squeeze(-1), hit)
    assert torch.equal(rows(sf.points), points) and torch.equal(rows(sf.sigma).squeeze(-1), sigma)
    dirs = ops.rays_fwd(xg, yg, zg, ZC, c2w, None, b, img, img, S)[2]
    assert float((points - (origin.view(b, 1, 3) + dirs * depth.unsqueeze(-1))).abs().max()) < 1e-6     # origin + dir * depth
    assert len(set(hit.flatten().tolist())) >= 2, "the level must cut the view"
    nrm, mask = rows(sf.normals), rows(sf.mask).squeeze(-1)
    assert float((nrm[mask == 1].norm(dim=-1) - 1).abs().max()) < 1e-6 if bool((mask == 1).any()) else True
    assert bool((nrm[mask == 0] == 0).all())
    assert bool(((rows(sf.sigma).squeeze(-1) - level).abs()[mask == 1] < 0.05 * sigma.abs().max()).all())    # on the surface
    assert G.surface(zs, level, **KW, normals=False).normals is None
    torch.manual_seed(9)
    sf_t = G.surface(zs, level, **KW, psi=0.5)
    assert torch.isfinite(sf_t.depth).all() and not torch.equal(sf_t.depth, sf.depth)

    # the composed search: the kernel's mask and, within the final bracket, its depth, on the rays rounding cannot decide
    cd, ch, cs, cp = ops.siren_surface_composed(level, 5, (b, img, img, S, ZC), xg, yg, zg, c2w, *args)
    amb = torch.zeros(b, n, dtype=torch.bool, device=d)
    smax = float(trace[..., 1][~torch.isnan(trace[..., 1])].abs().max())
    rep = _replay(dict(zg=zg.cpu(), level=level, b=b, n=n), trace, 5)
    for t, sig, own in rep.visited:
        amb |= (own & ~((sig - level).abs() > BAR * smax)).to(d)
    ok = ~amb
    assert int(ok.sum()) > n and torch.equal(ch[ok], hit[ok])
    assert float((cd - depth).abs()[ok].max()) <= (T1 - T0) / (S - 1) / 2 ** 5
    assert cp.shape == (b, n, 3) and cs.shape == (b, n) and ch.dtype == torch.uint8

    img3 = shade_surface(sf)
    assert img3.shape == (b, 3, img, img) and float(img3.min()) >= -1 and float(img3.max()) <= 1
    assert bool((img3.permute(0, 2, 3, 1).reshape(b, n, 3)[mask == 0] == -1).all())
    assert bool((img3.permute(0, 2, 3, 1).reshape(b, n, 3)[mask == 1] >= 2 * 0.2 - 1 - 1e-6).all())


def test_v1_generator_other_widths_and_the_exact_fp32_mode(x3, monkeypatch):
    """generator_v1 inherits the entry point; another SIREN width and CIPS_SIREN_FWD=f32 run the composed search (no kernel is
    missing silently: ops.siren_surface itself raises in that mode)"""
    from cips3d_amd.generator import NeRFNetwork
    from test_generator_v1_cpu import seeded_generator_v1
    ops = x3
    d = dev()
    G1 = seeded_generator_v1(9, device=d)
    zs = _zs(91, d)
    sf = G1.surface(zs, _level_of(G1, zs), **KW)
    assert sf.depth.shape == (2, 1, 8, 8) and sf.normals.shape == (2, 3, 8, 8) and sf.mask.dtype == torch.uint8
    assert all(bool(torch.isfinite(v).all()) for v in (sf.depth, sf.points, sf.sigma, sf.normals))

    b, img, S = 2, 8, 6
    xg, yg, zg = ops.pixel_grids(img, img, S, T0, T1, d)
    c2w = _case("ragged")["c2w"].to(d)
    geom = (b, img, img, S, ZC)
    torch.manual_seed(10)
    net = NeRFNetwork(hidden_dim=64, rgb_dim=32, style_dim=128).to(d)
    assert not net.fused
    g = torch.Generator().manual_seed(10)
    sd = _styles(torch.randn(b, 128, generator=g).to(d))
    depth, hit, sigma, points = net.surface_rays(sd, geom, xg, yg, zg, c2w, 0.0, 4)
    assert depth.shape == (b, img * img) and hit.dtype == torch.uint8 and points.shape == (b, img * img, 3)
    assert torch.isfinite(depth).all() and sigma.grad_fn is None
    assert torch.allclose(sigma, net.density(points, sd), rtol=1e-5, atol=1e-6)

    G = seeded_generator(12, device=d)
    st = _styles(torch.randn(b, 128, generator=g).to(d))
    k_depth, k_hit, _, _ = G.siren.surface_rays(st, geom, xg, yg, zg, c2w, 0.0, 4)
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "f32")
    f_depth, f_hit, f_sigma, _ = G.siren.surface_rays(st, geom, xg, yg, zg, c2w, 0.0, 4)
    assert float((f_hit == k_hit).float().mean()) > 0.95 and torch.isfinite(f_depth).all() and torch.isfinite(f_sigma).all()
    with torch.no_grad():
        args = G.siren._siren_args(st)
    with pytest.raises(RuntimeError, match="composed"):
        ops.siren_surface(0.0, 4, geom, xg, yg, zg, c2w, *args)
