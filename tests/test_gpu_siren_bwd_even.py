"""GPU: the EVEN list walk of the fused SIREN backward (cips_siren_bwd_x3_live_plan -> cips_siren_bwd_x3_live_even /
cips_siren_bwd_x3_rays_live_even -> cips_siren_bwd_x3_reduce_segments; ops.SIREN_BWD_EVEN): the workgroups of the launch
are dealt to the images by their live rounds instead of `chunks` each.  In file order the table is proven first (the rule
itself is tests/test_siren_bwd_plan_cpu.py, on the host; here the device table must be the host's), then the kernel on a
table that is the dense partition (bit-identical partials), then on skewed and ragged tables (gradients to the tolerance of
test_siren_backward, NaN in everything it must not read or write), then the switch in RayMarchFunction and a replayed graph.
With the switch on by default, the tests of tests/test_gpu_siren_bwd_live.py that go through ops (test_live_walk_equals_dense,
test_march_backward_live_switch, the replay test) run this path too; the *_live entries themselves are reached by that file's
direct-call bit-identity test and by the off arm of test_march_backward_even_switch here."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_err
from test_gpu_siren_bwd_live import TOL, P_, dev, _siren_setup, _points_or_rays, _grads, _march_setup, _run

pytestmark = pytest.mark.gpu


def _host_plan(count, P):
    from cips3d_amd import _lib
    lib = _lib.load()
    count = np.ascontiguousarray(count, dtype=np.int32)
    B = len(count)
    G = B * lib.cips_siren_bwd_x3_chunks(B, P)
    seg = np.full((G, 4), -7, dtype=np.int32)
    img = np.full((B, 2), -7, dtype=np.int32)
    assert lib.cips_siren_bwd_x3_live_plan_host(count.ctypes.data_as(C.c_void_p), B, P, seg.ctypes.data_as(C.c_void_p),
                                                img.ctypes.data_as(C.c_void_p)) == 0
    return torch.from_numpy(seg), torch.from_numpy(img)


def _device_plan(count, P):
    """count: (B) int32 on the device -> seg (G, 4), img (B, 2), pre-filled with -7"""
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    B = count.numel()
    G = B * lib.cips_siren_bwd_x3_chunks(B, P)
    seg = torch.full((G, 4), -7, dtype=torch.int32, device=dev())
    img = torch.full((B, 2), -7, dtype=torch.int32, device=dev())
    _lib.check(lib.cips_siren_bwd_x3_live_plan(P_(count), B, P, P_(seg), P_(img), ops._stream()), "cips_siren_bwd_x3_live_plan")
    return seg, img


# --------------------------------------------------------------------------------------
# a. the table
# --------------------------------------------------------------------------------------
def _count_vectors():
    rng = np.random.default_rng(3)
    P = 98304
    one = [0] * 32
    one[5] = P
    out = [([1024, 1024], 1024), ([P] * 32, P), ([24 * 128 * 19] * 32, P), (one, P), ([0] * 32, P), ([0, 0, 0], 128 * 7 + 5),
           ([128 * 7 + 5], 128 * 7 + 5), ([128 * 7 + 5] * 3, 128 * 7 + 5), ([2048, 384, 5, 0], 2048), ([5000, -3], 1024)]
    out.append(((np.clip(rng.normal(0.6, 0.22, 32), 0.05, 0.99) * P).astype(np.int64).tolist(), P))
    out.append((rng.integers(0, P + 1, 32).tolist(), P))
    out.append((rng.integers(0, 40001, 70).tolist(), 40000))          # more images than the plan's wave has lanes
    out.append((rng.integers(0, 3, 7).tolist(), 300))
    return out


def test_device_table_equals_host_table():
    got = []
    for count, P in _count_vectors():
        seg, img = _device_plan(torch.tensor(count, dtype=torch.int32, device=dev()), P)
        got.append((seg, img))
    torch.cuda.synchronize()
    for (count, P), (seg, img) in zip(_count_vectors(), got):
        seg_h, img_h = _host_plan(count, P)
        assert torch.equal(img.cpu(), img_h), (count[:8], P)
        assert torch.equal(seg.cpu(), seg_h), (count[:8], P)


# --------------------------------------------------------------------------------------
# the three launches by hand: the test owns the partial arrays and their pre-fill
# --------------------------------------------------------------------------------------
def _partials(tt, dfeat, dsigma, b, P, pts, rays, live):
    """live None: the dense call; else (idx, count): plan + EVEN call on NaN-filled partials -> sred, gpart, seg, img"""
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    sw = ops._siren_struct(tt)
    chunks = lib.cips_siren_bwd_x3_chunks(b, P)
    sred = torch.full((b * chunks, lib.cips_siren_bwd_x3_sred()), float("nan"), device=dev())
    gpart = torch.full((b * chunks, lib.cips_siren_bwd_x3_gpart()), float("nan"), device=dev())
    s = ops._stream()
    if live is None:
        if pts is not None:
            rc = lib.cips_siren_bwd_x3(C.byref(sw), P_(pts), P_(dfeat), P_(dsigma), P_(sred), P_(gpart), b, P, s)
        else:
            rc = lib.cips_siren_bwd_x3_rays(C.byref(sw), C.byref(rays), P_(dfeat), P_(dsigma), P_(sred), P_(gpart), b, s)
        _lib.check(rc, "siren backward")
        return sred, gpart, None, None
    idx, count = live
    seg, img = _device_plan(count, P)
    torch.cuda.synchronize()                         # the kernel reads its lists by this table: not launched on a wrong one
    seg_h, img_h = _host_plan(count.tolist(), P)
    assert torch.equal(seg.cpu(), seg_h) and torch.equal(img.cpu(), img_h)
    if pts is not None:
        rc = lib.cips_siren_bwd_x3_live_even(C.byref(sw), P_(pts), P_(dfeat), P_(dsigma), P_(idx), P_(count), P_(seg), P_(sred),
                                             P_(gpart), b, P, s)
    else:
        rc = lib.cips_siren_bwd_x3_rays_live_even(C.byref(sw), C.byref(rays), P_(dfeat), P_(dsigma), P_(idx), P_(count), P_(seg),
                                                  P_(sred), P_(gpart), b, s)
    _lib.check(rc, "siren backward, even")
    return sred, gpart, seg, img


def _even_grads(t, std, dfeat, dsigma, b, P, pts, rays, live):
    """plan -> kernel -> segmented reduction -> finalisation -> the 16 gradients by name, the style gradient, and the
    partial arrays with their tables"""
    from cips3d_amd import ops, _lib
    lib = _lib.load()
    tt = {k: v.detach().contiguous() for k, v in t.items()}
    sred, gpart, seg, img = _partials(tt, dfeat, dsigma, b, P, pts, rays, live)
    sr = torch.full((b, sred.shape[1]), float("nan"), device=dev())
    gp = torch.full((b, gpart.shape[1]), float("nan"), device=dev())
    _lib.check(lib.cips_siren_bwd_x3_reduce_segments(P_(sred), P_(gpart), P_(img), b, P_(sr), P_(gp), ops._stream()), "reduce")
    outs = tuple(torch.empty_like(tt[n]) for n in ops._SIREN_NAMES)
    sg = _lib.SirenGrads()
    for n, v in zip(ops._SIREN_NAMES, outs):
        setattr(sg, "d" + n, v.data_ptr())
    sw = ops._siren_struct(tt)
    _lib.check(lib.cips_siren_bwd_x3_finalize(C.byref(sw), P_(sr), P_(gp), b, 1, C.byref(sg), ops._stream()), "finalize")
    gs, = torch.autograd.grad([t[n] for n in ops._SIREN_NAMES[:6]], std, grad_outputs=list(outs[:6]), retain_graph=True)
    return dict(zip(ops._SIREN_NAMES, outs)), gs, (sred, gpart, seg, img)


def _nan_dead_rows(live, dfeat, dsigma):
    """-> (dense inputs: zeros in the dead rows), (live inputs: NaN in the dead rows)"""
    nan = torch.tensor(float("nan"), device=dev())
    dense = ((dfeat * live.unsqueeze(-1)).contiguous(), (dsigma * live).contiguous())
    lv = (torch.where(live.unsqueeze(-1), dfeat, nan).contiguous(), torch.where(live, dsigma, nan).contiguous())
    return dense, lv


def _assert_grads(got, got_s, ref, ref_s, tag):
    from cips3d_amd import ops
    worst = 0.0
    for n in ops._SIREN_NAMES:
        assert torch.isfinite(got[n]).all(), n
        e = rel_err(got[n], ref[n])
        print(f"{tag}: {n} rel err {e:.3e}")
        worst = max(worst, e)
        assert e < TOL, (n, e)
    assert torch.isfinite(got_s).all()
    e = rel_err(got_s, ref_s)
    print(f"{tag}: style rel err {e:.3e}, worst parameter {worst:.3e}")
    assert e < TOL


# --------------------------------------------------------------------------------------
# b. equal counts: the dense partition, bit for bit
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("trig", [0, 1])
@pytest.mark.parametrize("form", ["points", "rays"])
def test_even_walk_of_every_point_is_bit_identical(trig, form, monkeypatch):
    """b = 2, P = 1024, every point listed: the table is two workgroups of 512 slots per image in the dense row order, the
    same points in the same rounds, so the partials are the dense kernel's bit for bit"""
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    b, H, W, S = 2, 8, 8, 16
    P = H * W * S
    std, t, g = _siren_setup(b, 21)
    tt = {k: v.detach().contiguous() for k, v in t.items()}
    pts, rp = _points_or_rays(form, b, H, W, S, g)
    rays = rp[0] if rp else None
    dfeat = torch.randn(b, P, 32, generator=g).to(dev()); dsigma = torch.randn(b, P, generator=g).to(dev())
    idx = torch.arange(P, dtype=torch.int32, device=dev()).repeat(b, 1).contiguous()
    count = torch.full((b,), P, dtype=torch.int32, device=dev())
    sr_d, gp_d, _, _ = _partials(tt, dfeat, dsigma, b, P, pts, rays, None)
    sr_e, gp_e, seg, img = _partials(tt, dfeat, dsigma, b, P, pts, rays, (idx, count))
    torch.cuda.synchronize()
    assert seg.tolist() == [[0, 0, 512, 4], [0, 512, 1024, 4], [1, 0, 512, 4], [1, 512, 1024, 4]]
    assert torch.isfinite(sr_d).all() and torch.isfinite(gp_d).all()
    assert torch.equal(sr_e, sr_d) and torch.equal(gp_e, gp_d)


# --------------------------------------------------------------------------------------
# c. the skewed case
# --------------------------------------------------------------------------------------
def _skewed(form, seed=23):
    from cips3d_amd import ops
    b, H, W, S = 4, 8, 16, 16
    P = H * W * S
    assert P == 2048
    std, t, g = _siren_setup(b, seed)
    pts, rp = _points_or_rays(form, b, H, W, S, g)
    live = torch.zeros(b, P, dtype=torch.bool)
    live[0] = True
    live[1, torch.randperm(P, generator=g)[:3 * 128]] = True
    live[2, torch.tensor([0, 130, 131, 640, P - 1])] = True
    live = live.to(dev())
    dfeat = torch.randn(b, P, 32, generator=g).to(dev()); dsigma = torch.randn(b, P, generator=g).to(dev())
    dense, lv = _nan_dead_rows(live, dfeat, dsigma)
    lp = ops.live_points(live.to(torch.uint8).contiguous())
    return b, P, std, t, pts, rp, dense, lv, lp


@pytest.mark.parametrize("trig", [0, 1])
@pytest.mark.parametrize("form", ["points", "rays"])
def test_even_walk_of_skewed_images(form, trig, monkeypatch):
    """b = 4, P = 2048 (chunk 512, G = 16): image 0 all live, image 1 3 x 128 live points, image 2 five, image 3 none ->
    T = 2, n = [8, 2, 1, 1], 4 idle ids: image 0 runs on twice its dense share of workgroups.  Dead rows of dfeat / dsigma
    and the whole of sred / gpart are NaN beforehand: every gradient is finite and the dense call's (zeros in the dead
    rows) to TOL, image 3's FiLM gradients are exactly zero, and the idle rows are still NaN — nobody wrote or summed them."""
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    b, P, std, t, pts, rp, dense, lv, lp = _skewed(form)
    rays = rp[0] if rp else None
    ref, ref_s = _grads(t, std, dense[0], dense[1], b, P, pts, rays, None)
    got, got_s, (sred, gpart, seg, img) = _even_grads(t, std, lv[0], lv[1], b, P, pts, rays, lp)
    torch.cuda.synchronize()
    assert lp[1].tolist() == [2048, 384, 5, 0]
    assert seg.shape[0] == 16 and img[:, 1].tolist() == [8, 2, 1, 1] and int(seg[:, 3].max()) == 2
    idle = seg[:, 0] < 0
    assert idle.tolist() == [False] * 12 + [True] * 4
    _assert_grads(got, got_s, ref, ref_s, f"even walk skewed {form} trig={trig}")
    for n in ops._SIREN_NAMES[:6]:
        assert bool((got[n][3] == 0).all()), n
    assert bool((got_s[3] == 0).all())
    assert torch.isnan(sred[idle]).all() and torch.isnan(gpart[idle]).all(), "an idle row was written"
    assert torch.isfinite(sred[~idle]).all() and torch.isfinite(gpart[~idle]).all()


# --------------------------------------------------------------------------------------
# d. ragged shape
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("trig", [0, 1])
@pytest.mark.parametrize("form", ["points", "rays"])
@pytest.mark.parametrize("case", ["sparse", "empty_image"])
def test_even_walk_of_a_ragged_shape(case, form, trig, monkeypatch):
    """b = 3, P = 128 * 7 + 5 with the two masks of test_live_walk_equals_dense (G = 6): a clipped last round in every
    segment's image, an image of five points, an image of none"""
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "TRIG_MODE", trig)
    b, H, W, S = 3, 1, 53, 17
    P = H * W * S
    assert P == 128 * 7 + 5
    std, t, g = _siren_setup(b, 22)
    pts, rp = _points_or_rays(form, b, H, W, S, g)
    rays = rp[0] if rp else None
    live = torch.ones(b, P, dtype=torch.bool)
    if case == "sparse":
        live[1] = torch.rand(P, generator=g) >= 0.35
        live[2] = False
        live[2, torch.tensor([0, 130, 131, 640, P - 1])] = True
    else:
        live[0] = torch.rand(P, generator=g) >= 0.5
        live[1] = False
    live = live.to(dev())
    dfeat = torch.randn(b, P, 32, generator=g).to(dev()); dsigma = torch.randn(b, P, generator=g).to(dev())
    dense, lv = _nan_dead_rows(live, dfeat, dsigma)
    lp = ops.live_points(live.to(torch.uint8).contiguous())
    ref, ref_s = _grads(t, std, dense[0], dense[1], b, P, pts, rays, None)
    got, got_s, (sred, gpart, seg, img) = _even_grads(t, std, lv[0], lv[1], b, P, pts, rays, lp)
    torch.cuda.synchronize()
    assert seg.shape[0] == 6 and int(img[:, 1].sum()) <= 6
    _assert_grads(got, got_s, ref, ref_s, f"even walk {case} {form} trig={trig}")
    idle = seg[:, 0] < 0
    assert torch.isnan(sred[idle]).all() and torch.isnan(gpart[idle]).all()
    if case == "empty_image":
        for n in ops._SIREN_NAMES[:6]:
            assert bool((got[n][1] == 0).all()), n
        assert bool((got_s[1] == 0).all())


# --------------------------------------------------------------------------------------
# e. determinism
# --------------------------------------------------------------------------------------
def test_even_walk_is_deterministic():
    """the same inputs twice, by hand and through ops: equal bit for bit (fixed partition, fixed summation order)"""
    from cips3d_amd import ops
    b, P, std, t, pts, rp, dense, lv, lp = _skewed("rays", seed=24)
    rays = rp[0]
    a, a_s, (sr_a, gp_a, seg_a, _) = _even_grads(t, std, lv[0], lv[1], b, P, pts, rays, lp)
    c, c_s, (sr_c, gp_c, seg_c, _) = _even_grads(t, std, lv[0], lv[1], b, P, pts, rays, lp)
    assert ops.SIREN_BWD_EVEN
    o, o_s = _grads(t, std, lv[0], lv[1], b, P, pts, rays, lp)          # ops._siren_backward: the same three launches
    torch.cuda.synchronize()
    used = seg_a[:, 0] >= 0
    assert torch.equal(seg_a, seg_c)
    assert torch.equal(sr_a[used], sr_c[used]) and torch.equal(gp_a[used], gp_c[used])
    for n in ops._SIREN_NAMES:
        assert torch.equal(a[n], c[n]), n
        assert torch.equal(a[n], o[n]), n
    assert torch.equal(a_s, c_s) and torch.equal(a_s, o_s)


# --------------------------------------------------------------------------------------
# f. RayMarchFunction
# --------------------------------------------------------------------------------------
def test_march_backward_even_switch(monkeypatch):
    """RayMarchFunction forward + backward (r8, S = 16, b = 3) with ops.SIREN_BWD_EVEN on vs off (off: the *_live calls)"""
    from cips3d_amd import ops
    net, params, step = _march_setup(8, 16, 3, 0.0, 0, 13)
    monkeypatch.setattr(ops, "SIREN_BWD_LIVE", True)
    monkeypatch.setattr(ops, "SIREN_BWD_EVEN", False)
    off = _run(params, step)
    monkeypatch.setattr(ops, "SIREN_BWD_EVEN", True)
    on = _run(params, step)
    worst = 0.0
    for a, r in zip(on, off):
        assert torch.isfinite(a).all()
        worst = max(worst, rel_err(a, r))
    print(f"march backward even on vs off: worst gradient rel err {worst:.3e}")
    assert worst < TOL


def test_march_backward_even_follows_the_data_in_a_replayed_graph(monkeypatch):
    """The captured forward + backward (r8, S = 16, b = 3) replayed after the density bias moved by +1 (nearly every sample
    live), to -1 (nearly none) and back: each replay's gradients equal an eager run on the same weights bit for bit — the
    plan is a launch of the graph and reads the counts of the replay, nothing of the partition is baked in at capture time."""
    from cips3d_amd import ops, graph
    monkeypatch.setattr(ops, "SIREN_BWD_LIVE", True)
    monkeypatch.setattr(ops, "SIREN_BWD_EVEN", True)
    net, params, step = _march_setup(8, 16, 3, 0.0, 0, 12)
    captured = graph.capture(step, params=params)
    held = [p.grad for p in params]
    assert all(h is not None for h in held)
    counts, real = [], ops.live_points

    def spy(mask):                                   # eager runs only: installed after the capture
        idx, count = real(mask)
        counts.append((count, mask.numel()))
        return idx, count
    monkeypatch.setattr(ops, "live_points", spy)
    shares = []
    for delta in (1.0, -2.0, 1.0):
        with torch.no_grad():
            net.final_layer.bias.add_(delta)
        captured.replay()
        torch.cuda.synchronize()
        got = [h.clone() for h in held]
        ref = _run(params, step)
        for a, r in zip(got, ref):
            assert torch.isfinite(a).all()
            assert torch.equal(a, r)
        count, total = counts[-1]
        shares.append(count.sum().item() / total)
    print("live shares at bias +1, -1, +0:", [round(s, 3) for s in shares])
    assert shares[0] > 0.9 and shares[1] < 0.1 and shares[1] < shares[2] < shares[0]
