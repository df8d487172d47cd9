"""GPU: the view-reprojection kernels (csrc/reproject.hip) through ops.reproject against the fp64 yardstick
(tests/reproject_oracle.py), on the input sets tests/test_reproject_oracle_cpu.py holds to the 2 % cap: 2x2 on 2x2, 5x7 on 6x9
(no multiple of 4 anywhere: the scalar stores), 16^2 and 64^2 (the 16-byte stores; more than one workgroup), C = 1, 3, 4, B = 2
with a transform per image, the analytic plane / sphere scenes, a transform that puts part of the frame behind the source
camera, with and without src_depth, with non-finite, zero and negative tgt_depth pixels.

Pixels inside a decision margin (at most 2 % of a case) are left out of the value comparisons; they must still hold a mask in
{0, 1, 2} and a finite out.  Elsewhere, with eps = 2^-24:

  mask   equals the oracle's.
  uv     |error| <= uvbar = 16 eps max(1, |zc_src|) max(Ws, Hs) / 2 px: sixteen roundings on quantities of that size.
         (The kernel forms (u, v) in fp64 and rounds once: it has half an ulp of u to lose.  MI355X maximum: MEASURED below.)
  out    |error| <= 2 uvbar Lip + 8 eps max|src|.  Lip: the largest difference of two neighbours in the sampled cell (oracle).
         An error of uvbar in u and in v moves the sample by at most uvbar Lip each; the bilinear form itself is a handful of
         fp32 roundings on values no larger than max|src|.
  d_tgt_depth = sum_c dout_c (A_c U + B_c V), A_c = d out_c / du, B_c = d out_c / dv (the cell's slopes), U = du / ddepth,
         V = dv / ddepth.  |A_c|, |B_c| <= Lip.
           * A_c = (s01 - s00) + fv ((s11 - s10) - (s01 - s00)): an error of uvbar in fv changes it by at most 2 Lip uvbar, and
             its own fp32 evaluation (differences of neighbours, rounded relative to themselves, and one fma) by at most
             8 eps Lip.  The same for B_c.
           * U = (Ws-1)/2 zc_src (e_x q'_z - q'_x e_z) / q'_z^2 is a difference of two products: sixteen roundings, each relative
             to the larger of them, bound its error by 16 eps Uabs, Uabs the same expression with both terms taken absolutely
             (oracle).  The same for V.
           * the sum over the channels and the final rounding: 4 eps |d_tgt_depth|.
         bar = sum_c |dout_c| Lip [(|U| + |V|) (2 uvbar + 8 eps) + 16 eps (Uabs + Vabs)] + 4 eps |d_tgt_depth|
  d_src  every source pixel receives n contributions w_k dout_k (n counted by the oracle, four per visible target pixel whose
         cell holds it).  Each product is rounded once and the atomic adds round n - 1 times in some order, every partial sum
         bounded by S = sum |w_k dout_k|: (n + 4) eps S covers them and the rounding of the weights themselves.  An error of
         uvbar in u and in v changes a weight (1-fu)(1-fv) by at most 2 uvbar: 2 uvbar sum |dout_k| on top.
         bar = (n + 4) eps S + 2 uvbar sum |dout_k|

MEASURED on an MI355X, the largest error over its bar among the 21 input sets (every test prints its own, `pytest -s`):
  uv 0.036 (4.8e-7 px against 1.3e-5 in the fov-60 case; at 64^2 and fov 12: 1.9e-6 px, half an ulp of u, against 2.9e-4)
  out 0.027  |  d_tgt_depth 0.0012  |  d_src 0.0037  |  no pixel inside a margin was decided otherwise than by the oracle
"""
import pytest
import torch

import reproject_oracle as ro
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu
EPS = ro.EPS32
CASES = ro.cases()
_REF = {}


def _mx(t):
    return float(t.max()) if t.numel() else 0.0


def _ref(name):
    """the oracle's result for a case, computed once and shared"""
    if name not in _REF:
        _REF[name] = ro.run(CASES[name], ro.dout_for(CASES[name]))
    return _REF[name]


def _run(case, d, dout=None, src_grad=True, return_uv=True):
    from cips3d_amd import ops
    src = case.src.to(d).requires_grad_(src_grad and dout is not None)
    depth = case.tgt_depth.to(d).requires_grad_(dout is not None)
    res = ops.reproject(src, depth, case.pose.to(d), case.zc_tgt, case.zc_src,
                        src_depth=None if case.src_depth is None else case.src_depth.to(d), occ_tol=case.occ_tol, return_uv=return_uv)
    if dout is not None:
        res[0].backward(dout.to(d))
    return res, src, depth


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_the_oracle(name):
    d = dev()
    case, r = CASES[name], _ref(name)
    dout = ro.dout_for(case)
    (out, mask, uv), src, depth = _run(case, d, dout)
    out, mask, uv = out.detach().cpu().double(), mask.cpu(), uv.cpu().double()
    Hs, Ws = case.src.shape[2:]
    assert mask.dtype == torch.uint8 and mask.shape == r.mask.shape and out.shape == r.out.shape and uv.shape == r.uv.shape
    # everywhere, the margins included
    assert (mask <= 2).all() and torch.isfinite(out).all()
    assert (out[(mask != 1).expand_as(out)] == 0).all()
    assert torch.isnan(uv[(mask == 0).expand_as(uv)]).all() and torch.isfinite(uv[(mask != 0).expand_as(uv)]).all()
    if case.src_depth is None:
        assert (mask != 2).all()
    # away from the margins
    firm = ~r.near
    assert torch.equal(mask[firm], r.mask[firm])
    uvbar = ro.uv_bar(case.zc_src, Hs, Ws)
    seen = firm & (r.mask != 0)
    e_uv = _mx((uv - r.uv)[seen.expand_as(uv)].abs())
    vis = firm & (r.mask == 1)
    bar_out = (2 * uvbar * r.lip + 8 * EPS * case.src.abs().max().double()).expand_as(out)
    q_out = _mx(((out - r.out).abs() / bar_out)[vis.expand_as(out)])
    # gradients: also away from integer u, v (the cell's slopes jump there)
    g = dout.double()
    d_depth, d_src = depth.grad.cpu().double(), src.grad.cpu().double()
    assert (d_depth[mask != 1] == 0).all() and torch.isfinite(d_depth).all() and torch.isfinite(d_src).all()
    gsum = g.abs().sum(1, keepdim=True)
    bar_dd = gsum * r.lip * ((r.dudt.abs() + r.dvdt.abs()) * (2 * uvbar + 8 * EPS) + 16 * EPS * (r.dudt_abs + r.dvdt_abs)) \
        + 4 * EPS * r.d_tgt_depth.abs()
    sel = ~r.near_grad & (r.mask == 1)
    q_dd = _mx(((d_depth - r.d_tgt_depth).abs() / bar_dd.clamp_min(1e-300))[sel])
    # d_src: a pixel inside a margin that the kernel decides otherwise adds to (or is missing from) the four source pixels of its
    # cell; those source pixels, with a ring of one more around them, are left out of the comparison
    same = (mask == r.mask)
    assert (~same & ~r.near).sum() == 0
    bar_ds = (r.n + 4) * EPS * r.s_abs + 2 * uvbar * r.s_dout
    touched = torch.zeros_like(r.n, dtype=torch.bool)
    for b, _, i, j in (~same).nonzero().tolist():
        land = uv[b, :, i, j] if torch.isfinite(uv[b, :, i, j]).all() else r.uv[b, :, i, j]
        if torch.isfinite(land).all():
            u0, v0 = int(land[0]), int(land[1])
            touched[b, 0, max(v0 - 1, 0):v0 + 3, max(u0 - 1, 0):u0 + 3] = True
    keep = ~touched.expand_as(d_src)
    q_ds = _mx(((d_src - r.d_src).abs() / bar_ds.clamp_min(1e-300))[keep & (r.n.expand_as(d_src) > 0)])
    assert (d_src[keep & (r.n.expand_as(d_src) == 0)] == 0).all()
    print(f"{name}: uv error {e_uv:.3e} px = {e_uv / uvbar:.4f} of its bar {uvbar:.3e}, out {q_out:.4f} of its bar, d_tgt_depth "
          f"{q_dd:.4f}, d_src {q_ds:.4f}; {int((~same).sum())} pixels decided otherwise inside a margin")
    assert e_uv <= uvbar
    assert q_out <= 1
    assert q_dd <= 1
    assert q_ds <= 1


def test_identity_warp():
    """tgt2src = identity, src_depth = tgt_depth, occ_tol = 1e-4: the mask is 1 everywhere, the last row and column included,
    uv is the pixel's own index and out is src, within the bars"""
    d = dev()
    c = ro.random_case(11, 2, 3, 16, 16, 16, 16, True)
    c.pose = torch.eye(3, 4).repeat(2, 1, 1)
    c.src_depth, c.occ_tol = c.tgt_depth, 1e-4
    (out, mask, uv), _, _ = _run(c, d)
    assert (mask == 1).all()
    jj, ii = torch.arange(16.).view(1, 16).expand(16, 16), torch.arange(16.).view(16, 1).expand(16, 16)
    uvbar = ro.uv_bar(c.zc_src, 16, 16)
    e = max(float((uv[:, 0].cpu() - jj).abs().max()), float((uv[:, 1].cpu() - ii).abs().max()))
    r = ro.run(c)
    bar = 2 * uvbar * r.lip + 8 * EPS * c.src.abs().max().double()
    q = float(((out.cpu().double() - c.src.double()).abs() / bar).max())
    print(f"identity: uv error {e:.3e} px (bar {uvbar:.3e}), out {q:.3f} of its bar")
    assert e <= uvbar and q <= 1


def test_two_calls_give_equal_bits():
    d = dev()
    case = CASES["64_c3_depth"]
    dout = ro.dout_for(case)
    (o1, m1, u1), _, t1 = _run(case, d, dout)
    (o2, m2, u2), _, t2 = _run(case, d, dout)
    assert torch.equal(o1, o2) and torch.equal(m1, m2) and torch.equal(u1.nan_to_num(-1.), u2.nan_to_num(-1.))
    assert torch.equal(t1.grad, t2.grad)
    # without uv the other outputs are the same bits
    (o3, m3), _, _ = _run(case, d, return_uv=False)
    assert torch.equal(o1, o3) and torch.equal(m1, m3)


def test_a_misaligned_depth_takes_the_scalar_path_with_the_same_bits():
    from cips3d_amd import ops
    d = dev()
    case = CASES["16_c4_depth"]
    (o1, m1, u1), _, _ = _run(case, d)
    depth = torch.empty(case.tgt_depth.numel() + 1, device=d)[1:].view_as(case.tgt_depth)
    depth.copy_(case.tgt_depth)
    assert depth.data_ptr() % 16 == 4 and depth.is_contiguous()
    o2, m2, u2 = ops.reproject(case.src.to(d), depth, case.pose.to(d), case.zc_tgt, case.zc_src, src_depth=case.src_depth.to(d),
                               occ_tol=case.occ_tol, return_uv=True)
    assert torch.equal(o1, o2) and torch.equal(m1, m2) and torch.equal(u1.nan_to_num(-1.), u2.nan_to_num(-1.))


def test_src_without_grad_gets_none_and_nothing_is_launched_for_it(monkeypatch):
    from cips3d_amd import ops
    d = dev()
    case = CASES["16_c3"]
    dout = ro.dout_for(case)
    _, src_ref, depth_ref = _run(case, d, dout)
    real, calls = ops._lib.load(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != "cips_reproject_bwd":
                return fn

            def call(*a):
                calls.append(a)
                return fn(*a)
            return call
    monkeypatch.setattr(ops._lib, "load", lambda: Spy())
    _, src, depth = _run(case, d, dout, src_grad=False)
    assert src.grad is None and len(calls) == 1
    d_src_arg = calls[0][7]
    assert d_src_arg is None or d_src_arg.value is None          # a NULL d_src: the entry point neither zeroes nor adds
    assert torch.equal(depth.grad, depth_ref.grad)
    # and the other way round: only src
    calls.clear()
    src = case.src.to(d).requires_grad_(True)
    out, _ = ops.reproject(src, case.tgt_depth.to(d), case.pose.to(d), case.zc_tgt)
    out.backward(dout.to(d))
    assert calls[0][8] is None or calls[0][8].value is None
    r = _ref("16_c3")
    assert (src.grad.cpu().double() - r.d_src).abs().max() <= ((r.n + 4) * EPS * r.s_abs + 2 * ro.uv_bar(case.zc_src, 16, 16) * r.s_dout).max()
    assert src_ref.grad is not None
