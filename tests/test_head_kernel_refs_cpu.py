"""CPU: the references of tests/head_kernel_refs.py against each other, on the very cases tests/test_gpu_head_kernels.py
runs on the GPU.  What the GPU file takes for granted is shown here: the float32 restatement (the yardstick) agrees with
the float64 autograd truth, the bf16 hi / lo split carries a float32 to 2^-16, the in_dim = 1 gradients are degenerate the
way the absolute bound assumes, a re-split of hi + lo returns hi and lo except at exact ties, the ToRGB references are each
other's transposes, and the form codes written into the case tables are what the library's queries answer."""
import pytest
import torch

import head_kernel_refs as R

ALL_CASES = ([("fwd", c) for c in R.MODFC_FWD_CASES] + [("bwd", c) for c in R.MODFC_BWD_CASES] +
             [("cpu", c) for c in R.MODFC_CPU_EXTRA])
IDS = [f"{k}-{c.name}" for k, c in ALL_CASES]


def _layers(case):
    """distinct layers of a case (the 25-job lists repeat two shapes, each with its own seed: the first of each is enough here)"""
    seen = set()
    for (i, o), wsg in zip(case.shapes, case.inputs()):
        if (i, o) not in seen:
            seen.add((i, o))
            yield (i, o), wsg


@pytest.mark.parametrize("kind,case", ALL_CASES, ids=IDS)
def test_float32_restatement_agrees_with_float64_autograd(kind, case):
    """modfc_f32 (the closed form of modfc.hip's header, in float32) against modfc_ref64 (autograd of mod_conv_fc.py's rule).
    Bar 1e-6 = 8 x 2^-23 for each of demod (max_rel), wb, dW, ds (rel_err): every output is a chain of fewer than eight
    float32 roundings on top of sums whose rounding errors average out.  Measured: demod 4.1e-8 .. 1.4e-7, wb 2.8e-8 .. 6.4e-8,
    dW 6.5e-8 .. 2.2e-7, ds 8.5e-8 .. 2.5e-7.  The degenerate in_dim = 1 gradients: test_in_dim_1_is_degenerate."""
    for (i, o), (W, s, G) in _layers(case):
        wb, dm, dW, ds = R.modfc_ref64(W, s, G, case.eps)
        wbf, dmf, dWf, dsf = R.modfc_f32(W, s, G, case.eps)
        assert wbf.dtype == dmf.dtype == dWf.dtype == dsf.dtype == torch.float32
        e = (R.max_rel(dmf, dm), R.rel_err(wbf, wb), R.rel_err(dWf, dW), R.rel_err(dsf, ds))
        print(f"{case.name} ({i}, {o}) B {case.B}: demod {e[0]:.2e} wb {e[1]:.2e} dW {e[2]:.2e} ds {e[3]:.2e}")
        assert e[0] < 1e-6 and e[1] < 1e-6
        if not R.is_degenerate(i):
            assert e[2] < 1e-6 and e[3] < 1e-6


@pytest.mark.parametrize("kind,case", ALL_CASES, ids=IDS)
def test_split_carries_wb_to_2_pow_minus_16(kind, case):
    """hi + lo of split_ref(float32(wb64)) against wb64, element by element, relative to the element: hi keeps 8 significant
    bits and lo 8 of what is left, so 2^-17 plus the float32 rounding of wb64 itself (2^-24), which is why the measured
    7.5e-6 .. 7.7e-6 sits at 2^-17 = 7.63e-6 and sometimes just above it.  Bar 2^-16."""
    for (i, o), (W, s, G) in _layers(case):
        wb = R.modfc_ref64(W, s, G, case.eps)[0]
        hi, lo = R.split_ref(wb.float())
        assert hi.dtype == lo.dtype == torch.bfloat16
        err = float(((hi.double() + lo.double() - wb).abs() / wb.abs()).max())
        print(f"{case.name} ({i}, {o}): {err:.3e}")
        assert err <= 2.0 ** -16


def test_in_dim_1_is_degenerate():
    """in_dim = 1: wb = u / sqrt(u^2 + eps) = +-(1 - eps / (2 u^2)), whatever W and s; the true dW and ds are G eps / |u|^3 times
    (s+1) or W, ~1e-7 |G| for the |u| >= 0.25 that modfc_inputs draws.  The float32 closed form leaves the rounding of
    1 - d^2 u^2 there instead: rel_err of order 1 against that truth (measured 0.25 / 0.37 on N(0, 1) weights).  So the GPU
    tests bound |dW| and |ds| absolutely by degenerate_bound = 1e-5 max|G| max|W|: the truth is more than a factor 10 below it
    (measured: 430 times below), the float32 restatement is inside it (150 times below), and a kernel that dropped the correction term d^2 u c
    altogether would leave dW ~ G (s+1) d ~ G / |W|, five orders above it."""
    for case in (c for c in R.MODFC_FWD_CASES + R.MODFC_BWD_CASES if any(R.is_degenerate(i) for i, _ in c.shapes)):
        (W, s, G), = case.inputs()
        assert float(W.abs().min()) >= 0.5 and float((s + 1).min()) >= 0.5
        wb, dm, dW, ds = R.modfc_ref64(W, s, G)
        wbf, dmf, dWf, dsf = R.modfc_f32(W, s, G)
        assert float((wb.abs() - 1).abs().max()) < 1e-7 and float((wbf.abs() - 1).abs().max()) < 2e-7
        bound = R.degenerate_bound(W, G)
        truth, f32 = max(float(dW.abs().max()), float(ds.abs().max())), max(float(dWf.abs().max()), float(dsf.abs().max()))
        print(f"{case.name}: bound {bound:.2e}, truth {truth:.2e}, float32 {f32:.2e}, rel_err dW {R.rel_err(dWf, dW):.2f} ds {R.rel_err(dsf, ds):.2f}")
        assert truth * 10 < bound
        assert f32 < bound
        assert R.rel_err(dWf, dW) > 1e-3 or R.rel_err(dsf, ds) > 1e-3           # a relative bar has no meaning here
        m = (s + 1).unsqueeze(-1)
        dropped = (m * dmf.unsqueeze(1) * G).sum(0)                              # dW without the correction term
        assert float(dropped.abs().max()) > 1e3 * bound


def test_resplit_of_hi_plus_lo_returns_hi_and_lo_except_at_ties():
    """what the GPU file's 'the planes are the split of a float32' check rests on: v = hi + lo is exact in float32, and
    split_ref(v) is (hi, lo) again unless v lies exactly midway between two bf16 values (split_ties), where the first
    split's lo was rounded up to the half step and the re-split rounds to the even neighbour instead.  The ties are few (one
    value in ~500), and the mismatches are a subset of them."""
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(200000, generator=g), torch.randn(50000, generator=g) * 1e-4, torch.tensor([0.0, 1.0, -1.0, 0.5])])
    hi, lo = R.split_ref(x)
    v = hi.float() + lo.float()
    assert torch.equal(v.double(), hi.double() + lo.double())                  # exact
    assert float(((v - x).abs() / x.abs().clamp_min(1e-30)).max()) <= 2.0 ** -16
    h2, l2 = R.split_ref(v)
    same = (h2 == hi) & (l2 == lo)
    ties = R.split_ties(v)
    assert bool((same | ties).all())
    assert 0 < int((~same).sum()) <= int(ties.sum()) < x.numel() // 200
    assert torch.equal(h2.float() + l2.float(), v)                              # either way the value is kept


def test_torgb_references_are_each_others_transposes():
    """the three float64 ToRGB references against autograd of the forward one, with add, gate and slope"""
    g = torch.Generator().manual_seed(9)
    M, K = 37, 12
    x = torch.randn(M, K, generator=g, dtype=torch.float64)
    w = torch.randn(3, K, generator=g, dtype=torch.float64).requires_grad_(True)
    b = torch.randn(3, generator=g, dtype=torch.float64).requires_grad_(True)
    drgb = torch.randn(M, 3, generator=g, dtype=torch.float64)
    mask = torch.randn(M, K, generator=g)
    add = torch.randn(M, K, generator=g, dtype=torch.float64)
    pre = (x * 1.0).requires_grad_(True)                      # the layer below: x = leaky_relu(pre), gate = pre > 0
    rgb0 = torch.randn(M, 3, generator=g, dtype=torch.float64)
    act = torch.nn.functional.leaky_relu(pre, R.SLOPE)
    rgb = R.torgb_fwd_ref(act, w, b, rgb0)
    assert torch.equal(R.torgb_fwd_ref(act, w), act @ w.t())
    ((rgb * drgb).sum() + (act * add).sum()).backward()
    dT, db = R.torgb_bwd_w_ref(act.detach(), drgb)
    assert R.max_rel(dT, w.grad) < 1e-14 and R.max_rel(db, b.grad) < 1e-14
    un, out = R.torgb_bwd_x_ref(drgb, w.detach(), add, pre.detach(), R.SLOPE)
    assert R.max_rel(un, drgb @ w.detach() + add) < 1e-14 and R.max_rel(out, pre.grad) < 1e-14
    un2, out2 = R.torgb_bwd_x_ref(drgb, w.detach())
    assert torch.equal(un2, out2)
    f32 = R.torgb_fwd_ref(act.detach(), w.detach(), b.detach(), rgb0, dtype=torch.float32)
    assert f32.dtype == torch.float32 and R.rel_err(f32, rgb) < 1e-6


def test_case_tables_state_the_forms_the_queries_answer():
    """the codes in the tables were worked out by hand; the library's queries (host only) give the same, call by call"""
    from cips3d_amd import build, ops
    build.build(verbose=False)
    for cases, query in ((R.MODFC_FWD_CASES + R.MODFC_CPU_EXTRA, ops.modfc_prep_x3_batch_form), (R.MODFC_BWD_CASES, ops.modfc_prep_bwd_batch_form)):
        for case in cases:
            chunks = [case.shapes[c0:c0 + R.MAXJOBS] for c0 in range(0, len(case.shapes), R.MAXJOBS)]
            assert tuple(query(ch, case.B) for ch in chunks) == R.forms_of(case), case
