"""GPU: the helper kernels around the INR head's GEMMs (cips3d_amd/csrc/modfc.hip), ONE KERNEL AT A TIME against a float64
restatement of the operation (tests/head_kernel_refs.py) built from seeded inputs.  The head-level tests run all of them, but
behind a whole-network bar and at shapes that are multiples of every tile; here every kernel is reached at the smallest
shapes that take each of its edges.

Kernels of modfc.hip reached, and the edge each is taken to:
  modfc_prep_kernel (cips_modfc_prep)         out_dim off the 32-column block, in_dim off / below the 8 k-groups, in_dim = 1, B = 1
  modfc_colsum_batch_kernel<false / true>     one-lane tails, in_dim below the k-groups, out_dim < 4, idle blocks of a smaller job
  modfc_planes_batch_kernel (32 x 32)         one-lane tails both ways, in_dim = 1, a job far smaller than the grid, 24 + 1 jobs
  modfc_colsum4_batch_kernel<false / true>    one 4-column lane of a tile, max_out of another job, tiny weights against eps
  modfc_planes_batch64_kernel (64 x 64)       one lane of one tile, a second tile of one lane, a ragged k-tile, out_dim > 1024
  modfc_prep_bwd_w / _s_batch_kernel          out_dim % 4 == 0 but > 1024, B = 65, a mixed batch, the single-job entry
  modfc_prep_bwd_ws_batch_kernel<2>, <4>      one lane, a chunk of one lane, a full fourth chunk, B = 1 and B = 64, 24 + 1 jobs
  modfc_colsum4_cores / _fold_cores / modfc_prep_bwd_ws_cores_kernel   empty and uneven row segments (in_dim 1, 2, 3, 5), a second
                                              and a fifth trip of the chunk loop (idle lanes re-reading column 0), B = 64
  torgb_fwd_kernel<false>, <true>             K = 4 (one lane), K off 256, one row, the grid cap of 65 536 rows (second trip)
  torgb_fwd_x3_k512_kernel                    3 and 17 rows (fewer than / off the four in flight), the cap of 131 072 rows
  torgb_bwd_w_partial_kernel<false>           row-interleave groups 256, 28, 25, 16, 10 and 2 (idle threads at K = 36, 40, 100), a
                                              chunk of one row; torgb_bwd_w_reduce_kernel with 34 chunks (more than its 32 groups)
  torgb_bwd_w_partial_x3_k512_kernel, torgb_bwd_w_partial_cores_kernel, torgb_bwd_w_reduce_cores_kernel
                                              M = 1, 2, 127, 129, 8321: odd rows, a one-row chunk, an odd chunk count, 66 chunks; 2 and 8 taps
  torgb_bwd_x_kernel                          add / mask / copy in all eight combinations, the cap of 16 777 216 elements
  torgb_bwd_x_x3_kernel                       one lane per row (K = 8), the cap of 33 554 432 elements
  torgb_finish_kernel                         one row, three blocks, the cap of 1 048 576 rows, NaN in the padding float
Every output is carved out of one allocation filled with a sentinel (NaN as float32, 0x7fc1 as bf16), with at least 4 KiB of
it on both sides of every tensor (Arena): every element must come back written and every band untouched, bit for bit.
Which kernels a batch of layers reaches is asserted through ops.modfc_prep_x3_batch_form / ops.modfc_prep_bwd_batch_form,
the functions the entry points themselves switch on.

Bars.  Each output's error against float64 is held to K x the error the float32 restatement of the same formula shows on the
same inputs (head_kernel_refs.yardstick: never below 2^-24), and to the bar the older tests use for the quantity (LEGACY).
K per output kind is the smallest power of two that is at least twice the worst ratio measured on the MI355X:
    kind        measured on   worst kernel error / yardstick, where                                     K
    demod       26 outputs    1.44  (40, 3) B 3, scalar sums (yardstick at its 2^-24 floor)             4
    wb (fp32)    8            0.92  (64, 96) B 1                                                        2
    planes      42            1.00  (8, 4) B 1: both are the split's own 2^-17                          2
    planes_el   38            2.09  (1, 8) B 2: wb = +-1, one float32 ulp against the 2^-24 floor       8
    dW          71            1.92  (4, 8) B 2, job 19 of 25, fused pass                                4
    ds          71            2.01  (8, 4) B 2, job 14 of 25, fused pass                                8
    torgb      170            2.00  dT of the co-resident form at M = 129, 8 taps (2.003 before rounding) 8
    dbias      106            5.45  cips_torgb_bwd_w at (300, 100): one thread adds a chunk's 128 rows   16
                                    in order, torch's float32 sum is pairwise; the next largest is 1.25
    dx          28            0.70  (77, 40) add + mask                                                 2
  (planes: rel_err of hi + lo; planes_el: the largest element-wise relative error.)  No ratio is above 16.  in_dim = 1 gradients:
  |dW| 1.1e-7, |ds| 2.8e-7 against the absolute bound 3.6e-5, both forms.
Found by this file: both plane kernels took the split's remainder from the UNROUNDED product (hipcc contracted v - hi, v = W (s+1) d,
into one fma), so the planes were the split of no float32: check (d) of test_modfc_prep_x3_batch_every_form failed on 2 .. 373
elements of ten cases and on every element at in_dim = 1 (Wb = +-1: all of lo was bits below v's last place).  modfc.hip's
split_f32 now subtracts uncontracted; lo moves by one unit — the split's own resolution, at most 2^-16 of the value — in ~0.25 % of the elements.
Not covered: torgb_bwd_w_partial_kernel<true> (split planes, K != 512) beyond test_torgb_x3_forward_and_weight_gradient's
(777, 256) and (130, 64) — it shares its code with the <false> instantiation reached here at every group size; the ToRGB
forward folded into the GEMM epilogue (gemm_bf16x3_v3.hip), which only meets this file in cips_torgb_finish."""
import ctypes
import math

import pytest
import torch

import head_kernel_refs as R
from conftest import pack_bitplane

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 801
BF, F32 = torch.bfloat16, torch.float32
K_BAR = {"demod": 4, "wb": 2, "planes": 2, "planes_el": 8, "dW": 4, "ds": 8, "torgb": 8, "dbias": 16, "dx": 2}
LEGACY = {"demod": 1e-5, "wb": 1e-5, "planes": 2e-5, "planes_el": 2e-5, "dW": 1e-4, "ds": 1e-4, "torgb": 1e-5, "dbias": 2e-6, "dx": 1e-6}
CORES_VS_BATCH = 2e-6            # test_modfc_prep_batch_forward_backward's bar between the two summation orders

# the case tables reach every form code of both queries (head_kernel_refs asserts the same where the tables stand)
assert {f for c in R.MODFC_FWD_CASES for f in R.forms_of(c)} == {0, 1, 3}
assert {f for c in R.MODFC_BWD_CASES for f in R.forms_of(c)} == {0, 2, 4}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def lib_ops():
    from cips3d_amd import _lib, ops
    return _lib.load(), ops


def rel(a, b):
    """rel_err on the device of the reference"""
    a, b = a.detach().to(b.device).double(), b.detach().double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def mrel(a, b):
    a, b = a.detach().to(b.device).double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def elrel(a, b):
    """largest element-wise relative error"""
    a, b = a.detach().to(b.device).double(), b.detach().double()
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


def hold(kind, label, err, err_f32):
    """err <= K x yardstick(float32 restatement's error), and below the older tests' bar for the quantity"""
    y = R.yardstick(err_f32)
    print(f"RATIO {kind:9s} {label}: err {err:.3e} yardstick {y:.3e} ratio {err / y:.2f}")
    assert err <= K_BAR[kind] * y and err < LEGACY[kind], (kind, label, err, y)


class Arena:
    """Tensors carved out of ONE allocation filled with the sentinel word 0x7fc17fc1 — NaN as a float32, 0x7fc1 twice as bf16 —
    with a band of at least 4 KiB of it in front of, between and behind them; every tensor starts on a 16-byte boundary and
    every band is a multiple of 16 bytes long up to the tensor's own end.  check(): every element of every tensor was written
    (no sentinel left; `scratch` tensors excepted) and every band still holds the sentinel, bit for bit."""
    GUARD = 4096
    SENT32, SENT16 = 0x7fc17fc1, 0x7fc1

    def __init__(self, d, specs):
        self.spans, off = [], self.GUARD
        for spec in specs:
            shape, dtype = spec[0], spec[1]
            nb = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
            self.spans.append((off, nb, shape, dtype, len(spec) > 2 and spec[2] == "scratch"))
            off += (nb + 15) // 16 * 16 + self.GUARD
        self.raw = torch.full((off // 4,), self.SENT32, dtype=torch.int32, device=d).view(torch.uint8)
        self.t = [self.raw[o:o + nb].view(dtype).view(shape) for o, nb, shape, dtype, _ in self.spans]

    def check(self):
        end = 0
        for (o, nb, shape, dtype, scratch), t in zip(self.spans, self.t):
            assert not bool((self.raw[end:o].view(torch.int16) != self.SENT16).any()), f"band in front of {shape} written"
            end = o + nb
            if scratch:
                continue
            if dtype == F32:
                assert not bool(torch.isnan(t).any()), f"{shape}: elements left unwritten"
            else:
                assert not bool((t.view(torch.int16) == self.SENT16).any()), f"{shape}: elements left unwritten"
        assert not bool((self.raw[end:].view(torch.int16) != self.SENT16).any()), "band behind the last tensor written"


def chunks_of(seq):
    return [seq[c0:c0 + R.MAXJOBS] for c0 in range(0, len(seq), R.MAXJOBS)]


def value(hi, lo):
    return hi.double() + lo.double()


def assert_is_a_split(hi, lo, what):
    """the planes are the split of a float32: v = hi + lo (exact in float32) splits into hi and lo again, except where v is an
    exact tie between two bf16 values (head_kernel_refs.split_ties; test_resplit_of_hi_plus_lo_... on the CPU)"""
    v = hi.float() + lo.float()
    h2, l2 = R.split_ref(v)
    ok = ((h2 == hi) & (l2 == lo)) | R.split_ties(v)
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} elements are not a split"


# --------------------------------------------------------------------------------------
# modulate / demodulate prep, forward
# --------------------------------------------------------------------------------------
def run_prep_x3(shapes, B, devs, eps, d, single=False):
    """the split-plane prep called directly, one call per MAXJOBS jobs (single: cips_modfc_prep_x3 once per job) into an Arena
    -> per job (demod, wb_hi, wb_lo, wbt_hi, wbt_lo)"""
    from cips3d_amd import _lib
    lib, ops = lib_ops()
    outs, arenas, j0 = [], [], 0
    for chunk in chunks_of(shapes):
        A = Arena(d, [sp for (i, o) in chunk for sp in (((B, o), F32), ((B, i, o), BF), ((B, i, o), BF), ((B, o, i), BF), ((B, o, i), BF))])
        jobs = (_lib.ModfcPrepJob * len(chunk))()
        for n, (j, (i, o)) in enumerate(zip(jobs, chunk)):
            W, s = devs[j0 + n][:2]
            dm, wh, wl, th, tl = A.t[5 * n:5 * n + 5]
            j.weight, j.s, j.demod = ops._p(W), ops._p(s), ops._p(dm)
            j.wb_hi, j.wb_lo, j.wbt_hi, j.wbt_lo = ops._p(wh), ops._p(wl), ops._p(th), ops._p(tl)
            j.in_dim, j.out_dim = i, o
            if single:
                assert lib.cips_modfc_prep_x3(ops._p(W), ops._p(s), ops._p(wh), ops._p(wl), ops._p(th), ops._p(tl), ops._p(dm), B, i, o,
                                              eps, ops._stream()) == 0
            outs.append((dm, wh, wl, th, tl))
        if not single:
            assert lib.cips_modfc_prep_x3_batch(jobs, len(chunk), B, eps, ops._stream()) == 0
        arenas.append(A)
        j0 += len(chunk)
    torch.cuda.synchronize()
    for A in arenas:
        A.check()
    return outs


@pytest.mark.parametrize("case", R.MODFC_FWD_CASES, ids=repr)
def test_modfc_prep_x3_batch_every_form(case):
    """demod, the wb planes and the wbt planes of cips_modfc_prep_x3_batch: (a) the case reaches the kernels it is meant for;
    (b) demod (max_rel) and the planes' value hi + lo (rel_err and element by element) against float64, each within K x what the
    float32 restatement — for the planes: put through split_ref — shows on the same inputs; (c) the transposed planes are the
    row-major planes transposed, bit for bit; (d) the planes are the split of a float32; (e) the ops wrapper (which cuts the
    list into calls of MAXJOBS) returns the same bits; (f) where every call takes the scalar kernels (form 0), the single-job
    entry returns the same bits."""
    lib, ops = lib_ops()
    d = dev()
    forms = tuple(ops.modfc_prep_x3_batch_form(ch, case.B) for ch in chunks_of(case.shapes))
    assert forms == R.forms_of(case)                                                                           # (a)
    ins = case.inputs()
    devs = [(W.to(d), s.to(d)) for W, s, _ in ins]
    outs = run_prep_x3(case.shapes, case.B, devs, case.eps, d)
    wrapped = ops.modfc_prep_x3_batch(devs, eps=case.eps)
    for n, ((i, o), (W, s, G), (dm, wh, wl, th, tl), (wbP, wbtP, dmW)) in enumerate(zip(case.shapes, ins, outs, wrapped)):
        if n >= 2 and n < len(ins) - 1:
            continue                      # the 24 / 25-job lists: the first two and the last job against float64, all of them in (e)
        label = f"{case.name}[{n}] ({i}, {o}) B {case.B}"
        wb64, dm64 = R.modfc_ref64(W, s, G, case.eps)[:2]
        wbf, dmf = R.modfc_f32(W, s, G, case.eps)[:2]
        hold("demod", label, mrel(dm.cpu(), dm64), mrel(dmf, dm64))                                            # (b)
        yv = value(*R.split_ref(wbf))
        for hi, lo, ref, what in ((wh, wl, wb64, "wb"), (th, tl, wb64.transpose(1, 2), "wbt")):
            v = value(hi.cpu(), lo.cpu())
            assert v.shape == ref.shape
            yref = yv if what == "wb" else yv.transpose(1, 2)
            hold("planes", f"{label} {what}", rel(v, ref), rel(yref, ref))
            hold("planes_el", f"{label} {what}", elrel(v, ref), elrel(yref, ref))
        assert torch.equal(th, wh.transpose(1, 2)) and torch.equal(tl, wl.transpose(1, 2)), label              # (c)
        assert_is_a_split(wh.cpu(), wl.cpu(), label)                                                           # (d)
    for (dm, wh, wl, th, tl), (wbP, wbtP, dmW) in zip(outs, wrapped):                                          # (e)
        assert torch.equal(dm, dmW) and torch.equal(wh, wbP.hi) and torch.equal(wl, wbP.lo)
        assert torch.equal(th, wbtP.hi) and torch.equal(tl, wbtP.lo)
    if set(forms) == {0}:                                                                                      # (f)
        for a, b in zip(outs, run_prep_x3(case.shapes, case.B, devs, case.eps, d, single=True)):
            assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_modfc_prep_eps_is_where_the_rule_puts_it():
    """tiny weights: sum u^2 ~ 8e-7, so eps = 1e-6 more than halves demod and a dropped, doubled or misplaced eps moves it by
    tens of percent; the two tiny_w cases above hold the kernel to float64 at either eps, this shows the premise"""
    a, b = (c for c in R.MODFC_FWD_CASES if c.name in ("tiny_w", "tiny_w_eps"))
    (W, s, G), = a.inputs()
    d0, d1 = R.modfc_ref64(W, s, G, a.eps)[1], R.modfc_ref64(W, s, G, b.eps)[1]
    assert a.eps == 1e-8 and b.eps == 1e-6 and float((d1 / d0).max()) < 0.8


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("i,o", [(64, 96), (33, 40), (5, 100), (1, 8)])
def test_modfc_prep_fp32_entry(i, o, B):
    """cips_modfc_prep: demod, wb and wbt in float32 against float64; wbt is wb transposed, bit for bit"""
    lib, ops = lib_ops()
    d = dev()
    W, s, G = R.modfc_inputs(i, o, B, 8000 + 17 * i + o + B)
    A = Arena(d, [((B, i, o), F32), ((B, o, i), F32), ((B, o), F32)])
    wb, wbt, dm = A.t
    Wd, sd = W.to(d), s.to(d)
    assert lib.cips_modfc_prep(ops._p(Wd), ops._p(sd), ops._p(wb), ops._p(wbt), ops._p(dm), B, i, o, R.EPS, ops._stream()) == 0
    torch.cuda.synchronize()
    A.check()
    wb64, dm64 = R.modfc_ref64(W, s, G)[:2]
    wbf, dmf = R.modfc_f32(W, s, G)[:2]
    label = f"fp32 ({i}, {o}) B {B}"
    hold("demod", label, mrel(dm.cpu(), dm64), mrel(dmf, dm64))
    hold("wb", label, rel(wb.cpu(), wb64), rel(wbf, wb64))
    assert torch.equal(wbt, wb.transpose(1, 2))


# --------------------------------------------------------------------------------------
# modulate / demodulate prep, backward
# --------------------------------------------------------------------------------------
def run_prep_bwd(shapes, B, devs, d, mode):
    """mode 'batch' | 'cores' | 'single': the backward called directly into an Arena -> per job (dW, ds); cbuf is scratch"""
    from cips3d_amd import _lib
    lib, ops = lib_ops()
    parts = lib.cips_cores_colsum_parts() if mode == "cores" else 1
    outs, arenas, j0 = [], [], 0
    for chunk in chunks_of(shapes):
        A = Arena(d, [sp for (i, o) in chunk for sp in (((parts, B, o), F32, "scratch"), ((i, o), F32), ((B, i), F32))])
        jobs = (_lib.ModfcBwdJob * len(chunk))()
        for n, (j, (i, o)) in enumerate(zip(jobs, chunk)):
            W, s, dm, G = devs[j0 + n]
            cbuf, dW, ds = A.t[3 * n:3 * n + 3]
            j.weight, j.s, j.demod, j.gwb = ops._p(W), ops._p(s), ops._p(dm), ops._p(G)
            j.cbuf, j.dweight, j.ds = ops._p(cbuf), ops._p(dW), ops._p(ds)
            j.in_dim, j.out_dim = i, o
            if mode == "single":
                assert lib.cips_modfc_prep_bwd(ops._p(W), ops._p(s), ops._p(dm), ops._p(G), ops._p(cbuf), ops._p(dW), ops._p(ds), B, i, o,
                                               ops._stream()) == 0
            outs.append((dW, ds))
        if mode != "single":
            fn = lib.cips_modfc_prep_bwd_batch_cores if mode == "cores" else lib.cips_modfc_prep_bwd_batch
            assert fn(jobs, len(chunk), B, ops._stream()) == 0
        arenas.append(A)
        j0 += len(chunk)
    torch.cuda.synchronize()
    for A in arenas:
        A.check()
    return outs


def same_bits(xs, ys):
    return all(torch.equal(a, b) for x, y in zip(xs, ys) for a, b in zip(x, y))


@pytest.mark.parametrize("case", R.MODFC_BWD_CASES, ids=repr)
def test_modfc_prep_bwd_every_form(case):
    """dW and ds of cips_modfc_prep_bwd_batch (scalar three-pass, fused with 2 and with 4 chunks) and of the co-resident entry:
    (a) the form; (b) rel_err against float64 within K x the float32 restatement's — in_dim = 1: |dW|, |ds| below the absolute
    bound of head_kernel_refs.degenerate_bound; (c) the ops wrapper returns the same bits; (d) where the co-resident entry
    applies (B <= 64, every out_dim % 4 == 0): it against float64, against the batch entry at 2e-6, and twice bit for bit;
    where it does not: it answers hipErrorNotSupported and the wrapper's cores=True falls back to the batch entry; (e) form 0:
    the single-job entry returns the batch entry's bits.  demod comes from the float64 reference rounded to float32, not
    from the forward kernel: an error there cannot cancel here."""
    from cips3d_amd import _lib
    lib, ops = lib_ops()
    d = dev()
    forms = tuple(ops.modfc_prep_bwd_batch_form(ch, case.B) for ch in chunks_of(case.shapes))
    assert forms == R.forms_of(case)                                                                           # (a)
    ins = case.inputs()
    refs = [R.modfc_ref64(W, s, G, case.eps) for W, s, G in ins]
    devs = [(W.to(d), s.to(d), r[1].float().to(d), G.to(d)) for (W, s, G), r in zip(ins, refs)]

    def against_float64(outs, tag):
        for n, ((i, o), (W, s, G), r, (dW, ds)) in enumerate(zip(case.shapes, ins, refs, outs)):
            label = f"{case.name}[{n}] ({i}, {o}) B {case.B} {tag}"
            assert dW.shape == (i, o) and ds.shape == (case.B, i)
            if R.is_degenerate(i):
                bound = R.degenerate_bound(W, G)
                print(f"{label}: |dW| {float(dW.abs().max()):.2e} |ds| {float(ds.abs().max()):.2e} bound {bound:.2e}")
                assert float(dW.abs().max()) <= bound and float(ds.abs().max()) <= bound
                continue
            f = R.modfc_f32(W, s, G, case.eps)
            hold("dW", label, rel(dW.cpu(), r[2]), rel(f[2], r[2]))
            hold("ds", label, rel(ds.cpu(), r[3]), rel(f[3], r[3]))

    outs = run_prep_bwd(case.shapes, case.B, devs, d, "batch")
    against_float64(outs, "batch")                                                                             # (b)
    assert same_bits(outs, ops.modfc_prep_bwd_batch(devs))                                                     # (c)
    if case.B <= 64 and all(o % 4 == 0 for _, o in case.shapes):                                               # (d)
        co = run_prep_bwd(case.shapes, case.B, devs, d, "cores")
        against_float64(co, "cores")
        for (i, o), (dW, ds), (dWc, dsc) in zip(case.shapes, outs, co):
            if not R.is_degenerate(i):
                assert rel(dWc, dW) < CORES_VS_BATCH and rel(dsc, ds) < CORES_VS_BATCH
        assert same_bits(co, run_prep_bwd(case.shapes, case.B, devs, d, "cores"))
        assert same_bits(co, ops.modfc_prep_bwd_batch(devs, cores=True))
    else:
        jobs = (_lib.ModfcBwdJob * len(case.shapes))()
        for j, (i, o) in zip(jobs, case.shapes):
            j.in_dim, j.out_dim = i, o               # refused before any pointer is read
        assert lib.cips_modfc_prep_bwd_batch_cores(jobs, len(case.shapes), case.B, None) == UNSUPPORTED
        assert same_bits(outs, ops.modfc_prep_bwd_batch(devs, cores=True))
    if set(forms) == {0}:                                                                                      # (e)
        assert same_bits(outs, run_prep_bwd(case.shapes, case.B, devs, d, "single"))


# --------------------------------------------------------------------------------------
# ToRGB, fp32 entries
# --------------------------------------------------------------------------------------
def torgb_inputs(M, K, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *sh: torch.randn(*sh, generator=g, device=device)
    x, w, bias, rgb0, drgb, add, mask = rn(M, K), rn(3, K), rn(3), rn(M, 3), rn(M, 3), rn(M, K), rn(M, K)
    mask = torch.where(mask < 0, mask - 0.1, mask + 0.1)             # |mask| >= 0.1: the gate is unambiguous
    return x, w, bias, rgb0, drgb, add, mask


# the last: 65 543 rows against the 16 384 x 4 waves of the capped grid -> a second grid-stride trip (1 MB of input)
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M,K", [(1, 4), (5, 36), (130, 40), (777, 256), (1000, 512), (65536 + 7, 4)])
def test_torgb_fwd_fp32(M, K, accumulate, with_bias):
    lib, ops = lib_ops()
    d = dev()
    x, w, bias, rgb0 = torgb_inputs(M, K, 100 * M + K)[:4]
    b = bias if with_bias else None
    A = Arena(d, [((M, 3), F32)])
    rgb, = A.t
    if accumulate:
        rgb.copy_(rgb0)
    xd, wd, bd = x.to(d), w.to(d), (bias.to(d) if with_bias else None)
    assert lib.cips_torgb_fwd(ops._p(xd), ops._p(wd), ops._p(bd), ops._p(rgb), M, K,
                              int(accumulate), ops._stream()) == 0
    torch.cuda.synchronize()
    A.check()
    r0 = rgb0 if accumulate else None
    ref = R.torgb_fwd_ref(x, w, b, r0)
    hold("torgb", f"fwd ({M}, {K}) acc {accumulate} bias {with_bias}", rel(rgb.cpu(), ref), rel(R.torgb_fwd_ref(x, w, b, r0, dtype=F32), ref))


# row-interleave groups 256 / (K / 4) = 256, 28, 25, 10, 16, 2; (129, 36): a chunk of one row; 4225 rows: 34 chunks for the
# reduction's 32 groups
@pytest.mark.parametrize("M,K", [(1, 4), (129, 36), (130, 40), (300, 100), (4096 + 129, 64), (1000, 512)])
def test_torgb_bwd_w_fp32(M, K):
    lib, ops = lib_ops()
    d = dev()
    x, _, _, _, drgb = torgb_inputs(M, K, 100 * M + K + 1)[:5]
    chunks = lib.cips_torgb_bwd_partials(M)
    assert chunks == -(-M // 128)
    xd, gd = x.to(d), drgb.to(d)
    got = []
    for _ in range(2):
        A = Arena(d, [((chunks, 4, K), F32, "scratch"), ((3, K), F32), ((3,), F32)])
        part, dw, db = A.t
        assert lib.cips_torgb_bwd_w(ops._p(xd), ops._p(gd), ops._p(part), ops._p(dw), ops._p(db), M, K, ops._stream()) == 0
        torch.cuda.synchronize()
        A.check()
        got.append((dw, db))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])           # fixed combine order
    dT, dbias = R.torgb_bwd_w_ref(x, drgb)
    fT, fb = R.torgb_bwd_w_ref(x, drgb, dtype=F32)
    hold("torgb", f"bwd_w ({M}, {K}) dT", rel(got[0][0].cpu(), dT), rel(fT, dT))
    hold("dbias", f"bwd_w ({M}, {K}) dbias", rel(got[0][1].cpu(), dbias), rel(fb, dbias))


def test_torgb_bwd_w_fp32_refuses_what_it_cannot_tile():
    lib, ops = lib_ops()
    buf = torch.zeros(4096, device=dev())
    for K in (516, 6):                   # above the 512 columns of a pass; no multiple of 4
        assert lib.cips_torgb_bwd_w(ops._p(buf), ops._p(buf), ops._p(buf), ops._p(buf), ops._p(buf), 1, K, ops._stream()) == INVALID
    torch.cuda.synchronize()
    assert not bool(buf.any())


def run_torgb_bwd_x(M, K, drgb, w, add, mask, copy, d):
    lib, ops = lib_ops()
    A = Arena(d, [((M, K), F32)] * (2 if copy else 1))
    out, un = A.t[0], (A.t[1] if copy else None)
    assert lib.cips_torgb_bwd_x(ops._p(drgb), ops._p(w), ops._p(add), ops._p(mask), R.SLOPE, ops._p(un), ops._p(out), M, K, ops._stream()) == 0
    torch.cuda.synchronize()
    A.check()
    return un, out


@pytest.mark.parametrize("with_add,with_mask,copy", [(a, m, c) for a in (False, True) for m in (False, True) for c in (False, True)])
@pytest.mark.parametrize("M,K", [(77, 40), (1000, 64)])
def test_torgb_bwd_x_fp32(M, K, with_add, with_mask, copy):
    """dx = drgb T (+ add), the copy before the gate, the gate (mask > 0 ? 1 : slope): every operand present and absent"""
    d = dev()
    _, w, _, _, drgb, add, mask = torgb_inputs(M, K, 100 * M + K + 2)
    a, m = (add if with_add else None), (mask if with_mask else None)
    un, out = run_torgb_bwd_x(M, K, drgb.to(d), w.to(d), a.to(d) if with_add else None, m.to(d) if with_mask else None, copy, d)
    run, rout = R.torgb_bwd_x_ref(drgb, w, a, m)
    fun, fout = R.torgb_bwd_x_ref(drgb, w, a, m, dtype=F32)
    label = f"bwd_x ({M}, {K}) add {with_add} mask {with_mask}"
    hold("dx", label + " out", rel(out.cpu(), rout), rel(fout, rout))
    if copy:
        hold("dx", label + " copy", rel(un.cpu(), run), rel(fun, run))


def test_torgb_bwd_x_fp32_second_grid_stride_trip():
    """(32 768 + 3) x 512 = 16 778 752 elements against the 16 384 x 256 x 4 = 16 777 216 of the capped grid: the last 384
    float4s are written on a second trip (67 MB per tensor; inputs and float64 reference on the device)"""
    d = dev()
    M, K = 32768 + 3, 512
    _, w, _, _, drgb, add, mask = torgb_inputs(M, K, 77, device=d)
    un, out = run_torgb_bwd_x(M, K, drgb, w, add, mask, True, d)
    run, rout = R.torgb_bwd_x_ref(drgb, w, add, mask)
    fun, fout = R.torgb_bwd_x_ref(drgb, w, add, mask, dtype=F32)
    hold("dx", f"bwd_x ({M}, {K}) out", rel(out, rout), rel(fout, rout))
    hold("dx", f"bwd_x ({M}, {K}) copy", rel(un, run), rel(fun, run))
    hold("dx", f"bwd_x ({M}, {K}) second trip", rel(out.view(-1)[-1536:], rout.view(-1)[-1536:]), rel(fout.view(-1)[-1536:], rout.view(-1)[-1536:]))


# --------------------------------------------------------------------------------------
# ToRGB, split-plane entries (additions to test_torgb_x3_forward_and_weight_gradient and test_torgb_bwd_x_split_planes)
# --------------------------------------------------------------------------------------
def device_planes(M, K, g, d):
    """seeded on the device: (hi, lo) of a random float32 (M, K) and the planes' own value in float64"""
    hi, lo = R.split_ref(torch.randn(M, K, generator=g, device=d))
    return hi, lo, value(hi, lo)


# (65 543, 8): second trip of the generic form; (131 077, 512): second trip of the K = 512 form (8192 blocks x 16 rows);
# (3, 512), (17, 512): fewer rows than the four a wave keeps in flight, and a ragged last group
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M,K", [(65536 + 7, 8), (131072 + 5, 512), (3, 512), (17, 512)])
def test_torgb_fwd_x3_row_edges(M, K, accumulate):
    """the reference input is the planes' own value hi + lo, in float64 on the device: the bar measures the kernel's sums"""
    lib, ops = lib_ops()
    d = dev()
    g = torch.Generator(device=d).manual_seed(M + K)
    hi, lo, xv = device_planes(M, K, g, d)
    w, bias, rgb0 = (torch.randn(*sh, generator=g, device=d) for sh in ((3, K), (3,), (M, 3)))
    A = Arena(d, [((M, 3), F32)])
    rgb, = A.t
    if accumulate:
        rgb.copy_(rgb0)
    assert lib.cips_torgb_fwd_x3(ops._p(hi), ops._p(lo), ops._p(w), ops._p(bias), ops._p(rgb), M, K, int(accumulate), ops._stream()) == 0
    torch.cuda.synchronize()
    A.check()
    r0 = rgb0 if accumulate else None
    ref = R.torgb_fwd_ref(xv, w, bias, r0)
    f32 = R.torgb_fwd_ref(xv.float(), w, bias, r0, dtype=F32)
    hold("torgb", f"fwd_x3 ({M}, {K}) acc {accumulate}", rel(rgb, ref), rel(f32, ref))
    tail = slice(M - 8, M)                                   # the rows of the second trip / the ragged last group
    hold("torgb", f"fwd_x3 ({M}, {K}) acc {accumulate} last rows", rel(rgb[tail], ref[tail]), rel(f32[tail], ref[tail]))


# odd row counts for the co-resident kernel's two rows in flight, a one-row chunk (129), an odd chunk count for its two chunks
# per block (1, 2 -> 1; 129 -> 2; 8321 -> 66 chunks, more than the 64 lanes of its reduction)
@pytest.mark.parametrize("M", [1, 2, 127, 129, 8192 + 129])
def test_torgb_bwd_w_x3_k512_row_edges(M):
    """cips_torgb_bwd_w_x3 (one tap), _batch and _batch_cores with 2 and 8 taps at K = 512: every tap against float64 of the
    planes' own value; the batch entry's taps equal the single entry's bit for bit; the co-resident form within 2e-6 of them
    and bit-identical twice"""
    lib, ops = lib_ops()
    d = dev()
    K = 512
    g = torch.Generator(device=d).manual_seed(M)
    taps = [device_planes(M, K, g, d) for _ in range(8)]
    drgb = torch.randn(M, 3, generator=g, device=d)
    chunks = lib.cips_torgb_bwd_partials(M)

    def run(n, entry):
        A = Arena(d, [((n, chunks, 4, K), F32, "scratch"), ((n, 3, K), F32), ((n, 3), F32)])
        part, dw, db = A.t
        if entry == "single":
            rc = lib.cips_torgb_bwd_w_x3(ops._p(taps[0][0]), ops._p(taps[0][1]), ops._p(drgb), ops._p(part), ops._p(dw), ops._p(db), M, K, ops._stream())
        else:
            his = (ctypes.c_void_p * n)(*[t[0].data_ptr() for t in taps[:n]])
            los = (ctypes.c_void_p * n)(*[t[1].data_ptr() for t in taps[:n]])
            fn = lib.cips_torgb_bwd_w_x3_batch_cores if entry == "cores" else lib.cips_torgb_bwd_w_x3_batch
            rc = fn(his, los, n, ops._p(drgb), ops._p(part), ops._p(dw), ops._p(db), M, K, ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        A.check()
        return dw, db

    refs = [R.torgb_bwd_w_ref(t[2], drgb) for t in taps]
    f32s = [R.torgb_bwd_w_ref(t[2].float(), drgb, dtype=F32) for t in taps]
    dw1, db1 = run(1, "single")
    for n in (2, 8):
        dwb, dbb = run(n, "batch")
        dwc, dbc = run(n, "cores")
        dwc2, dbc2 = run(n, "cores")
        assert torch.equal(dwb[0], dw1[0]) and torch.equal(dbb[0], db1[0])
        assert torch.equal(dwc, dwc2) and torch.equal(dbc, dbc2)
        assert rel(dwc, dwb) < CORES_VS_BATCH and rel(dbc, dbb) < CORES_VS_BATCH
        for i in range(n):
            for tag, dw, db in (("batch", dwb, dbb), ("cores", dwc, dbc)):
                hold("torgb", f"bwd_w_x3 M {M} {tag} {n} taps [{i}] dT", rel(dw[i], refs[i][0]), rel(f32s[i][0], refs[i][0]))
                hold("dbias", f"bwd_w_x3 M {M} {tag} {n} taps [{i}] dbias", rel(db[i], refs[i][1]), rel(f32s[i][1], refs[i][1]))
    # the ops wrapper: the batched launch from two taps on, the same bits
    res = ops.torgb_bwd_w_x3_batch([ops.Planes(t[0], t[1]) for t in taps[:2]], drgb)
    assert torch.equal(res[0][0], dw1[0]) and torch.equal(res[0][1], db1[0])


# (65 539, 512): 33 555 968 elements against the 16 384 x 256 x 8 = 33 554 432 of the capped grid: a second trip; (5, 8): one
# lane per row
@pytest.mark.parametrize("M,K", [(5, 8), (65536 + 3, 512)])
def test_torgb_bwd_x_x3_row_edges(M, K):
    """gated planes and the float32 copy before the gate: the copy against float64 (the exact-fp32 bar), the planes' value
    against the gated float64 within K x the float32 restatement put through split_ref; the planes are a split"""
    lib, ops = lib_ops()
    d = dev()
    g = torch.Generator(device=d).manual_seed(M + K)
    drgb, w = torch.randn(M, 3, generator=g, device=d), torch.randn(3, K, generator=g, device=d)
    gate = torch.randn(M, K, generator=g, device=d) > 0
    A = Arena(d, [((M, K), F32), ((M, K), BF), ((M, K), BF)])
    cu, ph, pl = A.t
    bits = pack_bitplane(gate)
    assert lib.cips_torgb_bwd_x_x3(ops._p(drgb), ops._p(w), ops._p(bits), R.SLOPE, ops._p(cu), ops._p(ph), ops._p(pl), M, K,
                                   ops._stream()) == 0
    torch.cuda.synchronize()
    A.check()
    m = gate.float() * 2 - 1
    run, rout = R.torgb_bwd_x_ref(drgb, w, None, m)
    fun, fout = R.torgb_bwd_x_ref(drgb, w, None, m, dtype=F32)
    hold("dx", f"bwd_x_x3 ({M}, {K}) copy", rel(cu, run), rel(fun, run))
    v, yv = value(ph, pl), value(*R.split_ref(fout))
    hold("planes", f"bwd_x_x3 ({M}, {K})", rel(v, rout), rel(yv, rout))
    tail = slice(max(M * K - 1536, 0), M * K)                # what the second trip writes: the last 192 lanes of 8 columns
    hold("planes", f"bwd_x_x3 ({M}, {K}) last elements", rel(v.view(-1)[tail], rout.view(-1)[tail]), rel(yv.view(-1)[tail], rout.view(-1)[tail]))
    assert_is_a_split(ph, pl, f"bwd_x_x3 ({M}, {K})")


# (1 048 581, 2): five rows past the 4096 x 256 threads of the capped grid
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("M,nblocks", [(1, 1), (300, 3), (1048576 + 5, 2)])
def test_torgb_finish(M, nblocks, accumulate, with_bias):
    """rgb (+)= sum over column blocks of the GEMM epilogue's partials + bias; the fourth float of every partial is padding (NaN
    here) and must not reach the output"""
    lib, ops = lib_ops()
    d = dev()
    g = torch.Generator(device=d).manual_seed(M + nblocks)
    part = torch.randn(nblocks, M, 4, generator=g, device=d)
    part[..., 3] = float("nan")
    bias, rgb0 = torch.randn(3, generator=g, device=d), torch.randn(M, 3, generator=g, device=d)
    b = bias if with_bias else None
    A = Arena(d, [((M, 3), F32)])
    rgb, = A.t
    if accumulate:
        rgb.copy_(rgb0)
    assert lib.cips_torgb_finish(ops._p(part), nblocks, ops._p(b), ops._p(rgb), M, int(accumulate), ops._stream()) == 0
    torch.cuda.synchronize()
    A.check()

    def ref(dtype):
        y = part[..., :3].to(dtype).sum(0)
        y = y + bias.to(dtype) if with_bias else y
        return rgb0.to(dtype) + y if accumulate else y
    hold("torgb", f"finish ({M}, {nblocks}) acc {accumulate} bias {with_bias}", rel(rgb, ref(torch.float64)), rel(ref(F32), ref(torch.float64)))
    hold("torgb", f"finish ({M}, {nblocks}) last rows", rel(rgb[-5:], ref(torch.float64)[-5:]), rel(ref(F32)[-5:], ref(torch.float64)[-5:]))


def test_torgb_finish_refuses_a_misaligned_partial_pointer():
    lib, ops = lib_ops()
    d = dev()
    part, rgb = torch.zeros(2, 8, 4, device=d), torch.full((8, 3), 7.0, device=d)
    assert lib.cips_torgb_finish(ctypes.c_void_p(part.data_ptr() + 4), 1, None, ops._p(rgb), 8, 0, ops._stream()) == INVALID
    assert lib.cips_torgb_finish(ops._p(part), 0, None, ops._p(rgb), 8, 0, ops._stream()) == INVALID
    torch.cuda.synchronize()
    assert bool((rgb == 7.0).all())
