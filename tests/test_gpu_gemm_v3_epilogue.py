"""The epilogue of gemm_bf16x3_v3_kernel (8 rows x 64 columns per step, whole 128-byte lines per 8 lanes), through
ops.gemm_x3 / ops.gemm_x3_torgb, in the five flavours bench.py's gemm_roofline times:

    fwd            <0,0,0>        LeakyReLU, gate bits out, planes out
    fwd+torgb      <0,0,0,RGBF>   ... + ToRGB partials
    fwd+res+torgb  <0,0,1,RGBF>   ... + residual planes
    dx             <0,1,0>        gate bits in, planes out
    dx+addp+rgb    <1,1,0,ADDP>   + planes addend (un-gated on the fly) + rank-3 ToRGB term, gate bits in

Shapes: N = 512, K = 512 and K = 64 (two k-tiles: the whole contraction streams in under the previous tile's epilogue);
(a) B = 2, M = 512: 8 tiles, one per workgroup; (b) B = 8, M = 4608: 288 tiles on at most 256 workgroups, so some
workgroups run a second tile behind their first epilogue.

test_against_fp64: random inputs, every flavour's planes against a float64 evaluation of the same epilogue.  Tolerances are
those of tests/test_gpu_kernels.py: rel_err < 3e-5 for the planes (test_gemm_bf16x3_wide, all flavours, and
test_gemm_bf16x3_planes_addend), rel_err < 2e-5 for the ToRGB sums against the written planes times the ToRGB weights
(test_gemm_bf16x3_fused_torgb).  Gate bits equal pre-activation >= 0 wherever |pre-activation| > 3e-5 x its rms.

test_layout: inputs that are functions of (b, row, column) built so that every step of the epilogue is exact (or one
correctly rounded fp32 operation that torch repeats), every output element differs from every other one, and signs / gate
bits follow no symmetric pattern: hi plane, lo plane and gate bytes must be equal to the expectation at every address, bit
for bit; the ToRGB partials within the rounding of their 128-term fp32 sums."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 512
SLOPE = 0.2
SHAPES = {"a": (2, 512), "b": (8, 4608)}
FLAVOURS = ["fwd", "fwd+torgb", "fwd+res+torgb", "dx", "dx+addp+rgb"]
TOL_PLANES = 3e-5          # tests/test_gpu_kernels.py::test_gemm_bf16x3_wide / test_gemm_bf16x3_planes_addend
TOL_TORGB = 2e-5           # tests/test_gpu_kernels.py::test_gemm_bf16x3_fused_torgb


def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _planes(x):
    from cips3d_amd import ops
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return ops.Planes(hi.contiguous(), lo.contiguous())


def _pack_bits(b):
    """bool (..., N) -> uint8 (..., N/8), bit c&7 of byte c>>3"""
    w = (1 << torch.arange(8, device=b.device)).to(torch.int32)
    return (b.reshape(*b.shape[:-1], -1, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def _unpack_bits(u, n):
    return ((u.to(torch.int32).unsqueeze(-1) >> torch.arange(8, device=u.device)) & 1).reshape(*u.shape[:-1], n).bool()


def _rel_err(a, b):        # conftest.rel_err, on the device
    a = a.double(); b = b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _run(flavour, c, B, M, K):
    """one launch of `flavour` on the inputs c -> (planes, gate bits or None, ToRGB partials or None)"""
    from cips3d_amd import ops
    d = c["A"].hi.device
    P = ops.Planes(torch.full((B, M, N), float("nan"), device=d, dtype=torch.bfloat16),
                   torch.full((B, M, N), float("nan"), device=d, dtype=torch.bfloat16))
    bits = torch.full((B, M, N // 8), 0xA5, device=d, dtype=torch.uint8)
    part = torch.full((N // 128, B * M, 4), float("nan"), device=d)
    G = lambda **kw: ops.gemm_x3(c["A"], c["W"], M, N, K, K, K, B, M * K, N * K, P=P, **kw)
    old, ops.X3_KERNEL = ops.X3_KERNEL, 2          # the 256x256-tile kernels at every shape, as tests/test_gpu_kernels.py forces them
    try:
        if flavour == "fwd":
            G(act=1, mask_out=bits, gate_bits=2); part = None
        elif flavour == "fwd+torgb":
            G(act=1, mask_out=bits, gate_bits=2, torgb=(c["T"], part))
        elif flavour == "fwd+res+torgb":
            G(act=1, res=c["res"], mask_out=bits, gate_bits=2, torgb=(c["T"], part))
        elif flavour == "dx":
            G(mask=c["gate"], gate_bits=1); bits = part = None
        else:
            G(addp=(c["addp"], c["agate"]), rgb_g=c["rg"], rgb_w=c["rw"], mask=c["gate"], gate_bits=1); bits = part = None
        torch.cuda.synchronize()
    finally:
        ops.X3_KERNEL = old
    return P, bits, part


# ----------------------------------------------------------------------------------------------------------------------
# against fp64
# ----------------------------------------------------------------------------------------------------------------------
_CASES = {}


def _random_case(shape, K):
    """inputs of one (shape, K) and the float64 product, made once and shared by the five flavours (never modified)"""
    key = (shape, K)
    if key not in _CASES:
        B, M = SHAPES[shape]
        d = dev()
        g = torch.Generator(device=d).manual_seed(1000 * K + M)
        rn = lambda *s: torch.randn(*s, device=d, generator=g)
        A = rn(B, M, K); W = rn(B, N, K) * 0.05
        res = rn(B, M, N)
        D = rn(B, M, N); ag = rn(B, M, N) > 0                    # the previous layer's un-gated gradient and its gate
        gate = rn(B, M, N) > 0
        c = dict(A=_planes(A), W=_planes(W), res=_planes(res), addp=_planes(D * torch.where(ag, 1.0, SLOPE)),
                 agate=_pack_bits(ag), gate=_pack_bits(gate), rg=rn(B * M, 3), rw=rn(3, N), T=rn(3, N), tau=rn(3),
                 acc64=torch.bmm(A.double(), W.double().transpose(1, 2)), res64=res.double(), D64=D.double(), gate_b=gate)
        _CASES[key] = c
    return _CASES[key]


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("K", [512, 64])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_against_fp64(shape, K, flavour):
    from cips3d_amd import ops
    B, M = SHAPES[shape]
    c = _random_case(shape, K)
    P, bits, part = _run(flavour, c, B, M, K)
    acc = c["acc64"]
    if flavour.startswith("fwd"):
        pre = acc
        want = torch.where(pre > 0, pre, SLOPE * pre)
        if "res" in flavour:
            want = want + c["res64"]
    elif flavour == "dx":
        want = acc * torch.where(c["gate_b"], 1.0, SLOPE)
    else:
        want = (acc + c["D64"] + (c["rg"].double() @ c["rw"].double()).view(B, M, N)) * torch.where(c["gate_b"], 1.0, SLOPE)
    got = P.hi.double() + P.lo.double()
    assert torch.isfinite(got).all()
    e = _rel_err(got, want)
    print(f"v3 epilogue {flavour} shape {shape} K={K}: planes rel err vs fp64 {e:.3e}")
    assert e < TOL_PLANES
    if bits is not None:
        sure = pre.abs() > TOL_PLANES * pre.pow(2).mean().sqrt()
        assert bool((_unpack_bits(bits, N) == (pre >= 0))[sure].all())
    if part is not None:
        # the sums as the step forms them (ops.gemm_x3_torgb: partials + finishing launch), against the written planes
        rgb0 = torch.zeros(B * M, 3, device=P.hi.device)
        P2 = ops.Planes.empty(B, M, N, device=P.hi.device)
        b2 = torch.zeros(B, M, N // 8, device=P.hi.device, dtype=torch.uint8)
        old, ops.X3_KERNEL = ops.X3_KERNEL, 2
        try:
            ops.gemm_x3_torgb(c["A"], c["W"], M, N, K, K, K, B, M * K, N * K, P2, c["T"], c["tau"], rgb0, False, act=1,
                              res=c["res"] if "res" in flavour else None, mask_out=b2, gate_bits=2)
            torch.cuda.synchronize()
        finally:
            ops.X3_KERNEL = old
        assert torch.equal(P2.hi, P.hi) and torch.equal(P2.lo, P.lo) and torch.equal(b2, bits)
        want_rgb = got.view(B * M, N) @ c["T"].double().t() + c["tau"].double()
        e = _rel_err(rgb0, want_rgb)
        print(f"v3 epilogue {flavour} shape {shape} K={K}: ToRGB rel err {e:.3e}")
        assert e < TOL_TORGB
        assert _rel_err(part[:, :, :3].sum(0) + c["tau"], want_rgb) < TOL_TORGB


# ----------------------------------------------------------------------------------------------------------------------
# layout
# ----------------------------------------------------------------------------------------------------------------------
def _hash_bit(R, n, salt):
    """a bit per (global row, column) without symmetry in either index"""
    h = (R * 40503 + n * 2654435761 + salt * 97 + (R * n) * 31) & 0xFFFFFFFF
    return ((h ^ (h >> 7) ^ (h >> 13)) & 1).bool()


def _layout_case(K):
    """Shape (a).  With R = b M + m the global row (1 024 rows), r = R & 63, g = n >> 4 the 16-column group:
        acc[R][n] = s(R, g) t(n) 16^(R>>6) (32768 + 512 r + n),     s, t = +-1 from hashes
    as a sum over the two contraction indices 2 g, 2 g + 1 (all other operand entries are zero):
        A[R][2g] = s 16^(R>>6) 512 (64 + r)     W[n][2g] = t(n)          (7 and 1 significant bits)
        A[R][2g+1] = s 16^(R>>6)                W[n][2g+1] = t(n) n      (1 and 9: hi + lo planes hold 16)
    Every product and the sum are exact in fp32 (16 significant bits), the value is a different one at every (b, row,
    column): the binade gives R >> 6, the 16-bit integer r and n.  A value times the slope lands two binades lower, and
    the row blocks are four binades apart, so gated and un-gated values never meet either.  The other inputs (residual,
    addend, ToRGB term) are 6-bit integers times 2^-10 of the row's power of 16: exactly held by their planes, they move
    a value by less than half the distance to the next one (also after the slope), and every epilogue step stays one
    correctly rounded fp32 operation that torch repeats."""
    B, M = SHAPES["a"]
    d = dev()
    R = torch.arange(B * M, device=d, dtype=torch.int64).view(B * M, 1)
    n = torch.arange(N, device=d, dtype=torch.int64).view(1, N)
    scale = torch.ldexp(torch.ones(B * M, 1), (4 * (R.cpu() >> 6)).int()).to(d)         # (rows, 1): 16^(R>>6), exactly
    small = scale * 2.0 ** -10
    gidx = torch.arange(N // 16, device=d, dtype=torch.int64).view(1, N // 16)
    s = torch.where(_hash_bit(R, gidx, 1), 1.0, -1.0)                           # (rows, 32)
    t = torch.where(_hash_bit(torch.zeros_like(n), n, 2), 1.0, -1.0)            # (1, N)
    A = torch.zeros(B * M, K, device=d); W = torch.zeros(N, K, device=d)
    A[:, 0:64:2] = s * scale * 512.0 * (64 + (R & 63)).float()
    A[:, 1:64:2] = s * scale
    cols = torch.arange(N, device=d)
    W[cols, 2 * (cols >> 4)] = t[0]
    W[cols, 2 * (cols >> 4) + 1] = t[0] * cols.float()
    acc = s.repeat_interleave(16, dim=1) * t * scale * (32768 + 512 * (R & 63) + n).float()
    iv = lambda salt, bits: (((R * 131 + n * 17 + salt) * 2654435761 >> 9) & ((1 << bits) - 1)).float()
    sg = lambda salt: torch.where(_hash_bit(R, n, salt), 1.0, -1.0)
    res = sg(3) * small * iv(3, 6)
    abit = _hash_bit(R, n, 4)
    addp = sg(5) * small * iv(5, 6)                                             # x 5 (gain) where the bit is clear: exact
    gate = _hash_bit(R, n, 6)
    rg = small * (((R * 7) % 5) - 2 + torch.arange(3, device=d).view(1, 3)).float()      # (rows, 3) small integers x binade
    rw = (((n * 3 + torch.arange(3, device=d).view(3, 1) * 5) % 7) - 3).float()          # (3, N) small integers
    T = (((n * 5 + torch.arange(3, device=d).view(3, 1) * 3) % 9) - 4).float()
    v = lambda x: x.view(B, M, N)
    c = dict(A=_planes(A.view(B, M, K)), W=_planes(W.unsqueeze(0).expand(B, N, K).contiguous()), res=_planes(v(res)),
             addp=_planes(v(addp)), agate=_pack_bits(v(abit)), gate=_pack_bits(v(gate)), rg=rg.contiguous(), rw=rw.contiguous(),
             T=T.contiguous())
    for k in ("A", "W", "res", "addp"):                                         # the planes hold the values exactly
        assert torch.equal(c[k].hi.float() + c[k].lo.float(), {"A": A.view(B, M, K), "W": W.unsqueeze(0).expand(B, N, K),
                                                               "res": v(res), "addp": v(addp)}[k])
    c.update(acc=v(acc), res_f=v(res), addp_f=v(addp), abit=v(abit), gate_b=v(gate))
    return c


_LAYOUT = {}


def _same(got, want, what):
    bad = (got != want).nonzero()
    assert bad.shape[0] == 0, f"{what}: {bad.shape[0]} of {want.numel()} differ, the first at (b, row, column / byte) {bad[0].tolist()}"


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("K", [512, 64])
def test_layout(K, flavour):
    B, M = SHAPES["a"]
    if K not in _LAYOUT:
        _LAYOUT[K] = _layout_case(K)
    c = _LAYOUT[K]
    slope = torch.tensor(SLOPE, dtype=torch.float32, device=c["acc"].device)      # the descriptor's fp32 slope
    acc = c["acc"]
    want_bits = None
    # the epilogue in its own order (+add, +rgb term, gate, act, +res), one fp32 operation per step
    if flavour.startswith("fwd"):
        want_bits = acc > 0
        y = torch.where(acc > 0, acc, acc * slope)
        if "res" in flavour:
            y = y + c["res_f"]
    elif flavour == "dx":
        y = torch.where(c["gate_b"], acc, acc * slope)
    else:
        y = acc + torch.where(c["abit"], c["addp_f"], c["addp_f"] * 5.0)
        for ch in (2, 1, 0):                                                      # products exact: fused or not, one rounding
            y = y + (c["rg"][:, ch].view(B, M, 1) * c["rw"][ch].view(1, 1, N))
        y = torch.where(c["gate_b"], y, y * slope)
    assert torch.unique(y).numel() == y.numel(), "the expectation must differ at every address"
    if flavour in ("fwd", "dx"):
        assert (y != 0).all()
    hi = y.bfloat16()
    lo = (y - hi.float()).bfloat16()
    P, bits, part = _run(flavour, c, B, M, K)
    _same(P.hi.view(torch.int16), hi.view(torch.int16), "hi plane")
    _same(P.lo.view(torch.int16), lo.view(torch.int16), "lo plane")
    if want_bits is not None:
        wb = _pack_bits(want_bits)
        for bit in range(8):
            _same((bits >> bit) & 1, (wb >> bit) & 1, f"gate bit {bit}")
        assert 0.25 < want_bits.float().mean() < 0.75
    if part is not None:
        # partial (block of 128 columns, row): sum of y T over the block's columns; its fp32 evaluation, 128 fused
        # multiply-adds and three additions in whatever order, stays within 128 x 2^-24 x sum |y T| of the exact sum
        yT = y.double().view(B * M, N // 128, 128, 1) * c["T"].double().t().view(1, N // 128, 128, 3)
        want = yT.sum(2).permute(1, 0, 2)                                         # (blocks, rows, 3)
        bound = 128 * 2.0 ** -24 * yT.abs().sum(2).permute(1, 0, 2)
        assert bool(((part[:, :, :3].double() - want).abs() <= bound).all()), "ToRGB partials"
        assert bool((part[:, :, 3] == 0).all())
        assert bool((want.abs() > 4 * bound).float().mean() > 0.9)                # the check can tell a partial from its neighbours
