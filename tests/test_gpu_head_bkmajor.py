"""The head's backward on ONE orientation of the weight planes: the dX GEMMs read the forward's wbt planes (B, out, in) as a
k-major B operand (descriptor field b_kmajor, 256x256-tile v3 kernel), and the prep writes no wb planes for those layers.

GEMM: for every flavour the k-major kernel has — "dx" (gate bits in, planes out), "dx+addp+rgb" (+ planes addend, rank-3 ToRGB
term), "c" (plain fp32 C) — the same values once as B [N][K] (b_kmajor = 0) and once as B [K][ldb] (b_kmajor = 1): same MFMA
order, so the outputs must be EQUAL, bit for bit; one case is also held to the exact integer reference of gemm_exact.py in
both orientations.  Refusals: b_kmajor = 1 on anything the v3 kernel does not run returns hipErrorNotSupported (801), the
query says 0 and nothing is written.  Prep: jobs without wb planes leave wbt / demod (and the other jobs' wb) as they are
with both orientations.  Head: rgb and every gradient equal between ops.HEAD_DX_BKMAJOR True and False, and with True no
512-wide layer is given wb planes."""
import ctypes

import pytest
import torch

import gemm_exact as gx

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = 801, 1
SLOPE = 0.2
FLAVOURS = ["dx", "dx+addp+rgb", "c"]
# (M, N, K, batch, B layout): dense [K][N]; "pad": rows of N + 8; "shared": one B for the batch (strideB = 0)
SHAPES = {
    "two-ktiles": (256, 256, 64, 1, "dense"),            # smallest accepted: prologue and drain only
    "steady": (256, 512, 128, 2, "dense"),               # one steady iteration, two column tiles
    "head": (512, 512, 512, 3, "dense"),                 # the head's K, odd batch
    "tiles>cus": (256, 512, 64, 160, "dense"),           # 320 tiles: a workgroup's second tile streams in under its first epilogue
    "head-pad": (512, 512, 512, 3, "pad"),
    "head-shared": (512, 512, 512, 3, "shared"),
}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _planes(x):
    from cips3d_amd import ops
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return ops.Planes(hi.contiguous(), lo.contiguous())


class _Kernel:
    """ops.X3_KERNEL = k inside the block (2: the 256x256-tile kernels at every shape)"""

    def __init__(self, k):
        self.k = k

    def __enter__(self):
        from cips3d_amd import ops
        self.old, ops.X3_KERNEL = ops.X3_KERNEL, self.k

    def __exit__(self, *a):
        from cips3d_amd import ops
        ops.X3_KERNEL = self.old


_CASES = {}


def _case(name):
    """inputs of one shape, made once and shared by the three flavours and both orientations (never modified)"""
    if name not in _CASES:
        from cips3d_amd import ops
        M, N, K, batch, layout = SHAPES[name]
        d = dev()
        g = torch.Generator(device=d).manual_seed(17 * M + N + K + batch)
        rn = lambda *s: torch.randn(*s, device=d, generator=g)
        nb = 1 if layout == "shared" else batch
        W = rn(nb, N, K) * 0.05
        Wn = _planes(W)
        ldb = N + 8 if layout == "pad" else N
        Wk = ops.Planes(torch.full((nb, K, ldb), float("nan"), device=d, dtype=torch.bfloat16),
                        torch.full((nb, K, ldb), float("nan"), device=d, dtype=torch.bfloat16))
        Wk.hi[:, :, :N] = Wn.hi.transpose(1, 2)
        Wk.lo[:, :, :N] = Wn.lo.transpose(1, 2)
        ag = rn(batch, M, N) > 0
        _CASES[name] = dict(A=_planes(rn(batch, M, K)), Wn=Wn, Wk=Wk, ldb=ldb, sB_n=0 if nb == 1 else N * K, sB_k=0 if nb == 1 else K * ldb,
                            gate=gx.pack_bits(rn(batch, M, N) > 0), agate=gx.pack_bits(ag),
                            addp=_planes(rn(batch, M, N) * torch.where(ag, 1.0, SLOPE)), rg=rn(batch * M, 3), rw=rn(3, N))
    return _CASES[name]


def _run(flavour, c, M, N, K, batch, kmajor):
    """one launch -> the tensors it wrote"""
    from cips3d_amd import ops
    d = dev()
    P = ops.Planes(torch.full((batch, M, N), float("nan"), device=d, dtype=torch.bfloat16),
                   torch.full((batch, M, N), float("nan"), device=d, dtype=torch.bfloat16))
    Bm, ldb, sB = (c["Wk"], c["ldb"], c["sB_k"]) if kmajor else (c["Wn"], K, c["sB_n"])
    G = lambda **kw: ops.gemm_x3(c["A"], Bm, M, N, K, K, ldb, batch, M * K, sB, b_kmajor=1 if kmajor else 0, **kw)
    with _Kernel(2):
        if flavour == "dx":
            G(P=P, mask=c["gate"], gate_bits=1)
            out = (P.hi, P.lo)
        elif flavour == "dx+addp+rgb":
            G(P=P, addp=(c["addp"], c["agate"]), rgb_g=c["rg"], rgb_w=c["rw"], mask=c["gate"], gate_bits=1)
            out = (P.hi, P.lo)
        else:
            Cm = torch.full((batch, M, N), float("nan"), device=d)
            G(C=Cm)
            out = (Cm,)
        torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kmajor_b_equals_nt_b(shape, flavour):
    M, N, K, batch, _ = SHAPES[shape]
    c = _case(shape)
    want = _run(flavour, c, M, N, K, batch, kmajor=False)
    got = _run(flavour, c, M, N, K, batch, kmajor=True)
    for w in want:
        assert torch.isfinite(w.float()).all()
    for i, (g_, w) in enumerate(zip(got, want)):
        gx.same(g_, w, f"{flavour} {shape}: output {i}, B [K][ldb] against B [N][K]")


@pytest.mark.parametrize("kmajor", [0, 1])
def test_exact_integer_reference(kmajor):
    """gate flavour at (256, 512, 128, 2) on the integer operands of gemm_exact.py: the planes must equal the reference in
    both orientations (b_kmajor = 0: the kernel as it was)"""
    from cips3d_amd import ops
    M, N, K, batch = 256, 512, 128, 2
    d = dev()
    A, Bn = gx.x3_operands(M, N, K, batch, d)
    Bk = gx.Operand(batch, N, K, N, K * N, gx.B_SPAN, gx.B_SCALE, 13, d, kmajor=True)
    assert torch.equal(Bk.ih, Bn.ih) and torch.equal(Bk.il, Bn.il)
    acc, mag, lolo = gx.accumulators(A, Bn, False)
    case = dict(M=M, N=N, K=K, batch=batch, flavour="gate", slope=SLOPE, kernel=2, single=False)
    e, o, unit = gx.nt_reference(case, acc, mag, d)
    gx.assert_conditions(o, lolo, unit, "gate, slope 0.2", acc5=gx.nt_acc5(case))
    hi, lo = gx.split(o["v"])
    Ph = gx.Guarded(batch, M, N, N, M * N, gx.BF, d)
    Pl = gx.Guarded(batch, M, N, N, M * N, gx.BF, d)
    Bop = Bk if kmajor else Bn
    with _Kernel(2):
        ops.gemm_x3(ops.Planes(A.hi.data(), A.lo.data()), ops.Planes(Bop.hi.data(), Bop.lo.data()), M, N, K, K, N if kmajor else K,
                    batch, M * K, N * K, P=ops.Planes(Ph.data(), Pl.data()), mask=gx.pack_bits(e["gate"]), gate_bits=1, b_kmajor=kmajor)
        torch.cuda.synchronize()
    Ph.check(hi, "hi plane")
    Pl.check(lo, "lo plane")


def _refusal_desc(M, N, K, kernel, b_kmajor=1):
    """a gate-flavour descriptor on sentinel-filled outputs -> (descriptor, the output buffers, what keeps the inputs alive)"""
    from cips3d_amd import ops
    d = dev()
    batch = 2
    A = _planes(torch.ones(batch, M, K, device=d))
    W = _planes(torch.ones(batch, K, N, device=d))
    gate = torch.zeros(batch, M, N // 8, device=d, dtype=torch.uint8)
    Ph = gx.Guarded(batch, M, N, N, M * N, gx.BF, d)
    Pl = gx.Guarded(batch, M, N, N, M * N, gx.BF, d)
    desc = ops._x3_desc(A, W, M, N, K, K, N, batch, M * K, K * N, P=ops.Planes(Ph.data(), Pl.data()), mask=gate, gate_bits=1,
                        b_kmajor=b_kmajor)
    desc.kernel = kernel
    return desc, (Ph, Pl), (A, W, gate)


@pytest.mark.parametrize("M,N,K,kernel,ask", [(128, 256, 64, 2, True), (256, 128, 64, 2, True), (256, 256, 64, 1, True),
                                              (256, 256, 64, 3, True), (256, 256, 32, 2, False)])
def test_kmajor_refused_where_the_v3_kernel_does_not_run(M, N, K, kernel, ask):
    """a shape the v3 kernel declines, another kernel forced, K % 64 != 0: 801 from the entry point, nothing written; the
    query says 0 (not asked at K = 32, where its rule is that of the 128-wide shapes)"""
    from cips3d_amd import _lib, ops
    lib = _lib.load()
    desc, outs, keep = _refusal_desc(M, N, K, kernel)
    if ask:
        assert lib.cips_gemm_bf16x3_takes_bkmajor(ctypes.byref(desc)) == 0
    assert lib.cips_gemm_bf16x3(ctypes.byref(desc), ops._stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    for o in outs:
        o.untouched(f"M{M} N{N} K{K} kernel {kernel}")


def test_kmajor_refused_by_the_other_entry_points_and_taken_by_the_query():
    from cips3d_amd import _lib, ops
    lib = _lib.load()
    desc, outs, keep = _refusal_desc(256, 256, 128, 2)
    assert lib.cips_gemm_bf16x3_takes_bkmajor(ctypes.byref(desc)) == 1
    assert lib.cips_gemm_bf16(ctypes.byref(desc), ops._stream()) == UNSUPPORTED           # the single-pass family has no such form
    desc.b_kmajor = 0
    assert lib.cips_gemm_bf16x3_takes_bkmajor(ctypes.byref(desc)) == 0                   # nothing to take
    desc.b_kmajor = 1
    desc.act = 1                                                                           # a forward epilogue: not instantiated
    assert lib.cips_gemm_bf16x3_takes_bkmajor(ctypes.byref(desc)) == 0
    assert lib.cips_gemm_bf16x3(ctypes.byref(desc), ops._stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    for o in outs:
        o.untouched("refused entry points")


# ----------------------------------------------------------------------------------------------------------------------
# prep: jobs without wb planes
# ----------------------------------------------------------------------------------------------------------------------
PREP_SHAPES = [(32, 512), (512, 512), (512, 512), (32, 512)]
PREP_WANT = [True, False, True, False]


def _prep_layers(B):
    d = dev()
    g = torch.Generator(device=d).manual_seed(5 + B)
    return [(torch.randn(i, o, device=d, generator=g), torch.randn(B, i, device=d, generator=g) * 0.3) for i, o in PREP_SHAPES]


def _eq_planes(a, b):
    return torch.equal(a.hi, b.hi) and torch.equal(a.lo, b.lo)


@pytest.mark.parametrize("B", [1, 3])
def test_prep_batch_without_wb(B):
    from cips3d_amd import ops
    layers = _prep_layers(B)
    assert ops.modfc_prep_x3_batch_form(PREP_SHAPES, B) == 3                   # the 64 x 64-tile kernel
    full = ops.modfc_prep_x3_batch(layers)
    part = ops.modfc_prep_x3_batch(layers, want_wb=PREP_WANT)
    torch.cuda.synchronize()
    for (wb, wbt, dm), (wb2, wbt2, dm2), want in zip(full, part, PREP_WANT):
        assert _eq_planes(wbt, wbt2) and torch.equal(dm, dm2)
        assert (wb2 is not None) == want and (wb2 is None or _eq_planes(wb, wb2))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", [(32, 512), (512, 512)])
def test_prep_single_job_without_wb(shape, B):
    """the single-job entry: the scalar kernels"""
    from cips3d_amd import ops
    W, s = [(W, s) for (W, s) in _prep_layers(B) if tuple(W.shape) == shape][0]
    wb, wbt, dm = ops.modfc_prep_x3(W, s)
    none, wbt2, dm2 = ops.modfc_prep_x3(W, s, want_wb=False)
    torch.cuda.synchronize()
    assert none is None and _eq_planes(wbt, wbt2) and torch.equal(dm, dm2)
    assert torch.equal(wb.hi, wbt.hi.transpose(1, 2)) and torch.equal(wb.lo, wbt.lo.transpose(1, 2))   # one orientation holds both


def test_prep_refuses_half_a_pair():
    from cips3d_amd import _lib, ops
    from cips3d_amd.ops import _p
    lib = _lib.load()
    B = 2
    W, s = _prep_layers(B)[1]
    wb, wbt, dm = ops._modfc_prep_x3_out(W, B)
    st = ops._stream()
    for hi, lo in ((_p(wb.hi), None), (None, _p(wb.lo))):
        assert lib.cips_modfc_prep_x3(_p(W), _p(s), hi, lo, _p(wbt.hi), _p(wbt.lo), _p(dm), B, 512, 512, 1e-8, st) == INVALID
        jobs = (_lib.ModfcPrepJob * 1)()
        j = jobs[0]
        j.weight, j.s, j.demod, j.wb_hi, j.wb_lo, j.wbt_hi, j.wbt_lo = _p(W), _p(s), _p(dm), hi, lo, _p(wbt.hi), _p(wbt.lo)
        j.in_dim, j.out_dim = 512, 512
        assert lib.cips_modfc_prep_x3_batch(jobs, 1, B, 1e-8, st) == INVALID
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# head, end to end
# ----------------------------------------------------------------------------------------------------------------------
def _head_params(B, width, in0, nblocks):
    d = dev()
    g = torch.Generator(device=d).manual_seed(23)
    rn = lambda *s: torch.randn(*s, device=d, generator=g)
    params = []
    cin = in0
    for k in range(nblocks):
        params += [rn(cin, width) / cin ** 0.5, rn(B, cin) * 0.3, rn(width, width) / width ** 0.5, rn(B, width) * 0.3]
        cin = width
    for k in range(3, nblocks):
        params += [rn(3, width) / width ** 0.5, rn(3) * 0.1]
    return params


def _run_head(bkmajor, grad, monkeypatch):
    """-> (rgb, gradients or None, [(W shape, wb planes allocated?)] as the forward's prep call returned them)"""
    from cips3d_amd import ops
    B, n, in0, width, nblocks = 3, 256, 32, 512, 5
    d = dev()
    x0 = torch.randn(B, n, in0, device=d, generator=torch.Generator(device=d).manual_seed(29))
    params = _head_params(B, width, in0, nblocks)
    up = torch.randn(B, n, 3, device=d, generator=torch.Generator(device=d).manual_seed(31))
    seen = []
    real = getattr(ops.modfc_prep_x3_batch, "real", ops.modfc_prep_x3_batch)      # not the recorder of an earlier run

    def recording(layers, *a, **kw):
        out = real(layers, *a, **kw)
        seen.extend((tuple(W.shape), wb is not None) for (W, _), (wb, _, _) in zip(layers, out))
        return out
    recording.real = real
    monkeypatch.setattr(ops, "modfc_prep_x3_batch", recording)
    monkeypatch.setattr(ops, "HEAD_DX_BKMAJOR", bkmajor)
    monkeypatch.setattr(ops, "INR_MODE", "bf16x3")
    with _Kernel(2):                                     # the 256x256-tile kernels at this small batch
        if grad:
            leaves = [x0.requires_grad_(True)] + [p.requires_grad_(True) for p in params]
            rgb = ops.inr_head(nblocks, *leaves)
            (rgb * up).sum().backward()
            grads = [t.grad.clone() for t in leaves]
        else:
            with torch.no_grad():
                rgb = ops.inr_head(nblocks, x0, *params)
            grads = None
        torch.cuda.synchronize()
    return rgb.detach().clone(), grads, seen


@pytest.mark.parametrize("grad", [True, False])
def test_head_equal_on_both_sides_of_the_constant(grad, monkeypatch):
    rgb1, g1, seen1 = _run_head(True, grad, monkeypatch)
    rgb0, g0, seen0 = _run_head(False, grad, monkeypatch)
    assert torch.isfinite(rgb0).all() and float(rgb0.abs().max()) > 0
    assert torch.equal(rgb1, rgb0)
    if grad:
        assert len(g1) == len(g0) == 1 + 4 * 5 + 2 * 2
        for i, (a, b) in enumerate(zip(g1, g0)):
            assert torch.isfinite(b).all() and float(b.abs().max()) > 0, i
            assert torch.equal(a, b), f"gradient {i} differs"
    # what the forward allocated: no wb planes for the 512-wide layers, both orientations on the other side
    assert len(seen1) == len(seen0) == 10
    assert all(has == (shape != (512, 512)) for shape, has in seen1), seen1
    assert all(has for _, has in seen0), seen0
