"""The exact-integer GEMM yardstick (tests/gemm_exact.py) checked without a GPU:

  * the fp32 emulation — k-tiles in any order, one fp32 addition per term — equals the fp64 integer reference bit for bit, in
    both arithmetic modes: the accumulation order cannot matter;
  * the conditions the reference must satisfy (sum |terms| < 2^24 everywhere incl. the ToRGB sums, distinct rows / columns /
    batches, the forbidden term visible at more than half of the outputs, 5 m accumulators under the production slope) hold
    for EVERY shape, flavour and slope of the GPU case list;
  * seven deliberately wrong evaluations are reported by the comparison function the GPU test uses."""
import pytest
import torch

import gemm_exact as gx

DEV = torch.device("cpu")
CUS = 256          # the MI355X's; the GPU test sizes its "more tiles than CUs" batches from the device


def _expected(A, B, single, e=None, slope=0.25, act=0):
    acc, mag, other = gx.accumulators(A, B, single)
    return acc, mag, other, gx.epilogue(acc, mag, e or {}, slope, act=act, addp_gain=round(1 / slope))


@pytest.mark.parametrize("single", [False, True], ids=["bf16x3", "bf16"])
@pytest.mark.parametrize("M,N,K,batch", [(37, 40, 160, 2), (264, 136, 96, 3), (8, 32, 512, 1)])
def test_emulation_equals_the_integer_reference_in_any_order(M, N, K, batch, single):
    A, B = gx.x3_operands(M, N, K, batch, DEV)
    acc, _, _ = gx.accumulators(A, B, single)
    nk = K // gx.BK
    g = torch.Generator().manual_seed(K + M)
    orders = [list(range(nk)), list(range(nk - 1, -1, -1))] + [torch.randperm(nk, generator=g).tolist() for _ in range(3)]
    for order in orders:
        got = gx.emulate(A, B, order, gx.TERMS1 if single else gx.TERMS3)
        gx.same(got, acc.float(), f"emulation, k-tile order {order}")
    # the term order inside a tile does not matter either
    if not single:
        gx.same(gx.emulate(A, B, orders[2], gx.TERMS3[::-1]), acc.float(), "emulation, passes reversed")


def test_padding_is_nan_and_shared_weight_is_one_matrix():
    A, B = gx.x3_operands(37, 40, 96, 3, DEV, lda=104, ldb=112, strideA=37 * 104 + 8, strideB=0)
    for p, n in ((A.hi, 3 * 37 * 96), (A.lo, 3 * 37 * 96), (B.hi, 40 * 96), (B.lo, 40 * 96)):
        assert int(torch.isfinite(p.flat.float()).sum()) == n and int(torch.isnan(p.flat.float()).sum()) == p.flat.numel() - n
    assert B.ih.shape == (3, 40, 96) and torch.equal(B.ih[0], B.ih[2])
    Ak, Bk = gx.x3_operands(136, 72, 64, 2, DEV, kmajor=True)           # K-major planes hold the same logical values, transposed
    An, Bn = gx.x3_operands(136, 72, 64, 2, DEV)
    assert torch.equal(Ak.ih, An.ih) and torch.equal(Bk.il, Bn.il) and Ak.hi.shape == (2, 64, 136)
    assert torch.equal(Ak.hi.view().transpose(1, 2), An.hi.view())


def test_guarded_buffer_reports_region_and_guards():
    g = gx.Guarded(2, 5, 8, 16, 5 * 16 + 16, torch.float32, DEV)
    want = torch.arange(80, dtype=torch.float32).view(2, 5, 8)
    g.untouched("fresh")
    g.view()[:] = want
    g.check(want, "written")
    g.view()[1, 4, 7] = -1.0
    with pytest.raises(AssertionError, match=r"1 of 80 differ, the first at \(batch, row, column\) \(1, 4, 7\)"):
        g.check(want, "one element")
    g.view()[1, 4, 7] = want[1, 4, 7]
    g.flat[g.offset + 5 * 16] = 0.0                                     # the row behind M of batch 0
    with pytest.raises(AssertionError, match="guard / padding elements overwritten, the first at flat offset 80"):
        g.check(want, "row past M")
    with pytest.raises(AssertionError, match="refused"):
        g.untouched("refused")
    # -0.0 is not +0.0 and a NaN equals the same NaN: bit patterns are compared
    assert gx.diff(torch.tensor([[[-0.0]]]), torch.tensor([[[0.0]]]), "zero") is not None
    assert gx.diff(torch.tensor([[[float("nan")]]]), torch.tensor([[[float("nan")]]]), "nan") is None


# ----------------------------------------------------------------------------------------------------------------------
# the conditions on the reference, for the whole GPU case list
# ----------------------------------------------------------------------------------------------------------------------
_ACC = {}


def _acc(M, N, K, batch, single):
    key = (M, N, K, batch, single)
    if key not in _ACC:
        _ACC.clear()                                  # cases arrive grouped by shape: keep one
        _ACC[key] = gx.accumulators(*gx.x3_operands(M, N, K, batch, DEV), single)
    return _ACC[key]


def _nt_groups():
    """the NT cases that run (not refused), one per (shape, mode, flavour, slope) — the kernel choice, leading dimensions and
    strides do not enter the reference — grouped by mode and flavour sweep"""
    seen, groups = set(), {}
    for c in gx.nt_cases(CUS):
        if gx.nt_route(c) in ("invalid", "unsupported"):
            continue
        key = (c["M"], c["N"], c["K"], c["batch"], c["single"], c["flavour"], c["slope"])
        if key not in seen:
            seen.add(key)
            groups.setdefault(("bf16" if c["single"] else "bf16x3") + ("-many" if c.get("many") else ""), []).append(c)
    return groups


_NT = _nt_groups()


@pytest.mark.parametrize("group", sorted(_NT))
def test_reference_conditions_hold_for_every_nt_case(group):
    for c in sorted(_NT[group], key=lambda c: (c["M"], c["N"], c["K"], c["batch"])):
        acc, mag, other = _acc(c["M"], c["N"], c["K"], c["batch"], c["single"])
        e, o, unit = gx.nt_reference(c, acc, mag, DEV)
        gx.assert_conditions(o, other, unit, gx.case_id(c), acc5=gx.nt_acc5(c))
        if "bits" in gx.NT_FLAVOURS[c["flavour"]][2]:
            assert 0.25 < float((o["act"] > 0).float().mean()) < 0.75, gx.case_id(c)
    _ACC.clear()


def test_every_refused_nt_case_is_a_documented_refusal():
    refused = [c for c in gx.nt_cases(CUS) if gx.nt_route(c) in ("invalid", "unsupported")]
    assert refused
    for c in refused:
        if gx.nt_route(c) == "invalid":
            assert c["flavour"] in gx.BIT_FLAVOURS and (c["N"] % 32 or c.get("ldp8"))
        else:
            assert c["flavour"] in gx.V3_ONLY


@pytest.mark.parametrize("single", [False, True], ids=["bf16x3", "bf16"])
def test_reference_conditions_hold_for_every_kmajor_case(single):
    seen = set()
    for c in sorted(gx.km_cases(CUS), key=lambda c: (c["M"], c["N"], c["K"], c["batch"])):
        key = (c["M"], c["N"], c["K"], c["batch"], bool(c.get("ksplit")), max(c["groups"], 1))
        if c["single"] != single or key in seen:
            continue
        seen.add(key)
        for grp in range(max(c["groups"], 1)):
            if c.get("ksplit"):          # the batches are slices of one contraction
                A, B = gx.x3_operands(c["M"], c["N"], c["K"] * c["batch"], 1, DEV)
                acc, mag, other = gx.accumulators(A, B, single)
            elif grp == 0:
                acc, mag, other = _acc(c["M"], c["N"], c["K"], c["batch"], single)
            else:                        # the other groups' operands: later batch indices of the hash
                A, B = gx.x3_operands(c["M"], c["N"], c["K"], c["batch"], DEV, b0=grp * c["batch"])
                acc, mag, other = gx.accumulators(A, B, single)
            gx.assert_conditions(dict(v=acc, mag=mag), other, 1, gx.case_id(c))
    _ACC.clear()


def test_reference_conditions_hold_for_every_f32_case():
    for c in gx.f32_cases():
        *_, o, unit = gx.f32_reference(c, DEV)
        gx.assert_conditions(o, None, unit, gx.case_id(c))
        if "C2" in o:
            gx.assert_conditions(dict(v=o["C2"], mag=o["mag"]), None, unit, gx.case_id(c))


def test_the_issue_s_measured_shape():
    """(2, 264, 512, 512) — N a whole number of ToRGB blocks: the accumulators stay four decades below 2^24, the ToRGB block sums one, and a_lo b_lo would show
    at 99.8 % of the outputs"""
    A, B = gx.x3_operands(264, 512, 512, 2, DEV)
    acc, mag, lolo = gx.accumulators(A, B, False)
    assert float(mag.max()) < 1e5 and float(acc.abs().max()) < 2e4
    assert float((lolo != 0).float().mean()) > 0.99
    assert bool((acc % 5 == 0).all())
    e = gx.epilogue_inputs(264, 512, 2, DEV, ("res_hi", "res_lo", "T", "tau", "rgb0"))
    o = gx.epilogue(acc, mag, e, 0.25, act=1)
    print("largest ToRGB block sum of |v T|:", float(o["pmag"].max()), " finished:", float(o["rmag"].max()))
    assert float(o["pmag"].max()) * 4 < gx.LIMIT and float(o["rmag"].max()) * 4 < gx.LIMIT


# ----------------------------------------------------------------------------------------------------------------------
# wrong evaluations are detected
# ----------------------------------------------------------------------------------------------------------------------
M_, N_, K_, B_ = 37, 64, 96, 2


@pytest.fixture(scope="module")
def case():
    A, B = gx.x3_operands(M_, N_, K_, B_, DEV)
    e = gx.epilogue_inputs(M_, N_, B_, DEV, ("gate", "res_hi", "res_lo"))
    return A, B, e


def _planes_of(v):
    return torch.stack(gx.split(v))


def _detected(got, want, what):
    msg = gx.diff(got, want, what)
    print(msg)
    assert msg is not None and "differ, the first at (batch, row, column)" in msg, what
    return msg


def test_wrong_lo_lo_pass_is_detected(case):
    A, B, _ = case
    want = gx.accumulators(A, B, False)[0].float()
    got = gx.emulate(A, B, range(K_ // gx.BK), (("hi", "hi"), ("hi", "lo"), ("lo", "lo")))
    _detected(got, want, "a_lo b_lo in place of a_lo b_hi")


def test_dropped_lo_passes_of_the_last_k_tile_are_detected(case):
    A, B, _ = case
    want = gx.accumulators(A, B, False)[0].float()
    last = K_ // gx.BK - 1
    got = gx.emulate(A, B, range(last + 1), lambda kt: gx.TERMS1 if kt == last else gx.TERMS3)
    _detected(got, want, "lo passes of the last k-tile dropped")


def test_one_skipped_k_index_in_the_last_row_is_detected(case):
    A, B, _ = case
    want = gx.accumulators(A, B, False)[0].float()
    A2, _ = gx.x3_operands(M_, N_, K_, B_, DEV)
    A2.ih, A2.il = A2.ih.clone(), A2.il.clone()
    A2.ih[:, M_ - 1, K_ - 1] = 0
    A2.il[:, M_ - 1, K_ - 1] = 0
    got = gx.emulate(A2, B, range(K_ // gx.BK))
    msg = _detected(got, want, "k = K - 1 skipped for the last row")
    assert f"(0, {M_ - 1}, " in msg
    assert torch.equal(got[:, :M_ - 1], want[:, :M_ - 1])


def test_two_exchanged_rows_are_detected(case):
    A, B, _ = case
    want = gx.accumulators(A, B, False)[0].float()
    got = want.clone()
    got[:, [3, 4]] = want[:, [4, 3]]
    assert "(0, 3, 0)" in _detected(got, want, "rows 3 and 4 exchanged")


def test_gate_bit_of_the_neighbouring_column_is_detected(case):
    A, B, e = case
    want = _expected(A, B, False, e)[3]["v"]
    e2 = dict(e, gate=torch.roll(e["gate"], 1, dims=2))
    got = _expected(A, B, False, e2)[3]["v"]
    _detected(_planes_of(got)[0], _planes_of(want)[0], "gate bit of column n - 1: hi plane")


def test_residual_added_before_the_gate_is_detected(case):
    A, B, e = case
    acc, mag, _, o = _expected(A, B, False, e)
    wrong = gx.epilogue(acc, mag, e, 0.25, order="res_before_gate")["v"]
    _detected(_planes_of(wrong)[1], _planes_of(o["v"])[1], "residual in front of the gate: lo plane")
    _detected(_planes_of(wrong)[0], _planes_of(o["v"])[0], "residual in front of the gate: hi plane")


def test_three_passes_where_one_is_expected_are_detected(case):
    A, B, _ = case
    want = gx.accumulators(A, B, True)[0].float()
    _detected(gx.emulate(A, B, range(K_ // gx.BK), gx.TERMS3), want, "3-pass result, single pass expected")
    gx.same(gx.emulate(A, B, range(K_ // gx.BK), gx.TERMS1), want, "single pass")
