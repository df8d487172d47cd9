"""Exact-integer yardstick for the split-bf16 and fp32 GEMM kernels (tests/test_gemm_exact_cpu.py checks it without a GPU,
tests/test_gpu_gemm_exact.py holds every kernel to it bit for bit).

The four operand planes of a split-bf16 GEMM are independent inputs of the kernel: `lo` need not be the residual of `hi`.
Here all four are small integers — A planes in [-7, 7], B planes in 5 * [-3, 3], hi and lo drawn independently — so every
product and every partial sum of  a_hi b_hi + a_hi b_lo + a_lo b_hi  is an integer far below 2^24, and ANY fp32
accumulation, in any order and with any internal alignment of 24 bits or more, returns the exact sum.  A dropped or
duplicated k element, a lo fragment paired with the wrong hi fragment, a stale LDS stage, a fourth pass or a missing one is
a different integer almost everywhere (lo is as large as hi), so the kernel's output must EQUAL the integer reference at
every element, and the comparison needs no tolerance.

Values are pure functions of (batch, row, k) / (batch, column, k) / (batch, row, column) through an integer hash in which no
index plays a symmetric role.  Operands and auxiliary inputs live in flat buffers addressed with a leading dimension and a
batch stride (strideB = 0: one weight shared by all images), every padding element is NaN; outputs live in `Guarded`
buffers: guard rows in front and behind, padded leading dimension, everything pre-filled with a sentinel (NaN, 0xA5 bytes).

The epilogue reference is integer arithmetic held in fp64, in the order include/cips3d_hip.h documents:
    +add (or the un-gated planes addend), +rgb term, store C_unmasked, gate, act, store mask_out, +res, outputs, ToRGB sums.
The one non-integer step is the multiplication by the slope, evaluated as the kernels evaluate it: ONE fp32 multiplication
by the descriptor's fp32 slope.  With slope = 0.25 (addp_gain = 4) it is exact, every later step stays exact whether or not
the compiler contracts it into an fma.  With the production slope 0.2 it is one correctly rounded fp32 operation that torch
repeats; it is used only where no addition follows it (every flavour without `res`) — in the flavours without an addend
every accumulator is 5 m and fl(5 m * 0.2f) = m (assert_conditions checks it on the reference).

Nothing in this file looks at a kernel's output except `diff` / `same` / `Guarded.check`, the comparison itself."""
import torch

A_SPAN, B_SPAN, B_SCALE = 7, 3, 5          # A planes in [-7, 7], B planes in 5 * [-3, 3]
F32_SPAN = 63                              # cips_gemm_f32 operands, `add` / `res` / planes-addend planes
RGB_SPAN, TORGB_SPAN = 3, 4                # rgb_g / rgb_w, ToRGB weights
TAU = (3, -5, 7)                           # ToRGB bias
LIMIT = float(1 << 24)
BK = 32                                    # k-tile of the emulation (the 3-pass kernels' tile)
_M32 = 0xFFFFFFFF
BF = torch.bfloat16


# ----------------------------------------------------------------------------------------------------------------------
# integer hash
# ----------------------------------------------------------------------------------------------------------------------
def _mix(b, i, k, salt):
    """32 well-mixed bits per (b, i, k): different odd multipliers per index and two cross terms, then two xorshift-multiply
    rounds.  int64 tensors; every intermediate stays below 2^63."""
    h = (b * 0x9E3779B1 + i * 0x85EBCA77 + k * 0xC2B2AE3D + salt * 0x27D4EB2F + (i * k) * 0x165667B1
         + (b * i) * 40503 + (b * k) * 3 * 40507) & _M32
    h = ((h ^ (h >> 15)) * 0x2C1B3C6D) & _M32
    h = ((h ^ (h >> 12)) * 0x297A2D39) & _M32
    return h ^ (h >> 15)


def _idx(n, pos, device):
    s = [1, 1, 1]
    s[pos] = n
    return torch.arange(n, device=device, dtype=torch.int64).view(s)


def hash_int(batch, rows, cols, salt, span, device):
    """int64 (batch, rows, cols) in [-span, span]"""
    h = _mix(_idx(batch, 0, device), _idx(rows, 1, device), _idx(cols, 2, device), salt)
    return (h >> 7) % (2 * span + 1) - span


def hash_bit(batch, rows, cols, salt, device):
    """bool (batch, rows, cols)"""
    return ((_mix(_idx(batch, 0, device), _idx(rows, 1, device), _idx(cols, 2, device), salt) >> 9) & 1).bool()


# ----------------------------------------------------------------------------------------------------------------------
# strided buffers
# ----------------------------------------------------------------------------------------------------------------------
def _sentinel(dtype):
    return 0xA5 if dtype == torch.uint8 else float("nan")


def _bits(t):
    """the bit pattern of every element, as integers"""
    return t if t.dtype == torch.uint8 else t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Strided:
    """(batch, rows, cols) in a flat buffer: element (b, r, c) at offset + b * stride + r * ld + c.  Everything else — `guard`
    elements in front and behind, the ld - cols padding of every row, the gaps between batches — holds the sentinel (NaN;
    0xA5 for bytes).  stride = 0: one matrix shared by all batches."""

    def __init__(self, batch, rows, cols, ld, stride, dtype, device, guard=0, values=None):
        nb = 1 if stride == 0 else batch
        assert ld >= cols and (nb == 1 or stride >= rows * ld)
        self.shape, self.ld, self.stride, self.offset = (nb, rows, cols), ld, stride, guard
        self.flat = torch.full((guard + (nb - 1) * stride + rows * ld + guard,), _sentinel(dtype), dtype=dtype, device=device)
        if values is not None:
            self.view()[:] = values.to(dtype)

    def view(self, flat=None):
        return (self.flat if flat is None else flat).as_strided(self.shape, (self.stride, self.ld, 1), self.offset)

    def data(self):
        """the tensor whose data_ptr() the kernel gets"""
        return self.flat[self.offset:]


class Guarded(Strided):
    """an OUTPUT buffer: guard rows in front and behind (at least two rows, a multiple of 64 elements so that the kernel's
    pointer keeps its alignment), sentinel everywhere"""

    def __init__(self, batch, rows, cols, ld, stride, dtype, device):
        super().__init__(batch, rows, cols, ld, stride, dtype, device, guard=(2 * ld + 63) // 64 * 64)

    def check(self, want, what):
        """the written region equals `want` bit for bit (first differing (batch, row, column) and the count otherwise), and
        every guard and padding element still holds the sentinel"""
        want = want.to(self.flat.dtype)
        same(self.view(), want, what)
        exp = torch.full_like(self.flat, _sentinel(self.flat.dtype))
        self.view(exp)[:] = want
        bad = (_bits(self.flat) != _bits(exp)).nonzero()
        assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} guard / padding elements overwritten, the first at flat offset "
                                   f"{int(bad[0]) - self.offset} from the output pointer (ld {self.ld}, batch stride {self.stride})")

    def untouched(self, what):
        s = torch.full_like(self.flat, _sentinel(self.flat.dtype))
        n = int((_bits(self.flat) != _bits(s)).sum())
        assert n == 0, f"{what}: {n} elements written by a call that was refused"


def diff(got, want, what):
    """None when `got` equals `want` bit for bit, else a message naming the first differing index and the count"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = (_bits(got) != _bits(want)).nonzero()
    if bad.shape[0] == 0:
        return None
    i = tuple(bad[0].tolist())
    return (f"{what}: {bad.shape[0]} of {want.numel()} differ, the first at (batch, row, column) {i}: "
            f"got {got[i].item()!r}, want {want[i].item()!r}")


def same(got, want, what):
    msg = diff(got, want, what)
    assert msg is None, msg


# ----------------------------------------------------------------------------------------------------------------------
# operands
# ----------------------------------------------------------------------------------------------------------------------
class Operand:
    """one split-bf16 operand: ih / il int64 (batch, R, K) — the logical values, functions of (batch, row, k) — and the hi /
    lo plane buffers that hold them ([R][ld] rows, or [K][ld] with kmajor)"""

    def __init__(self, batch, R, K, ld, stride, span, scale, salt, device, kmajor=False, b0=0):
        nb = 1 if stride == 0 else batch
        ih = scale * hash_int(b0 + nb, R, K, salt, span, device)[b0:]
        il = scale * hash_int(b0 + nb, R, K, salt + 1, span, device)[b0:]          # drawn independently of hi
        st = (lambda t: t.transpose(1, 2)) if kmajor else (lambda t: t)
        rows, cols = (K, R) if kmajor else (R, K)
        self.hi = Strided(batch, rows, cols, ld, stride, BF, device, values=st(ih))
        self.lo = Strided(batch, rows, cols, ld, stride, BF, device, values=st(il))
        for p, v in ((self.hi, ih), (self.lo, il)):                      # every plane value is exactly a bf16
            assert torch.equal(p.view().to(torch.int64), st(v))
        self.ih, self.il = ih.expand(batch, R, K), il.expand(batch, R, K)
        self.ld, self.stride = ld, stride


def x3_operands(M, N, K, batch, device, lda=None, ldb=None, strideA=None, strideB=None, kmajor=False, b0=0):
    """A (batch, M, K) in [-7, 7] and B (batch, N, K) in 5 * [-3, 3] as Operands.  NT: planes [M][lda], [N][ldb]; kmajor: planes
    [K][lda], [K][ldb].  Defaults: dense.  strideB = 0: one B for all batches.  b0: the hash's batch index of the first batch
    (other operands for the other groups of a grouped launch)."""
    lda = lda or (M if kmajor else K)
    ldb = ldb or (N if kmajor else K)
    strideA = (K if kmajor else M) * lda if strideA is None else strideA
    strideB = (K if kmajor else N) * ldb if strideB is None else strideB
    return (Operand(batch, M, K, lda, strideA, A_SPAN, 1, 11, device, kmajor, b0),
            Operand(batch, N, K, ldb, strideB, B_SPAN, B_SCALE, 13, device, kmajor, b0))


def f32_operands(M, N, K, batch, device):
    """cips_gemm_f32: integers in [-63, 63], logical A (batch, M, K) and B (batch, N, K) as int64"""
    return hash_int(batch, M, K, 15, F32_SPAN, device), hash_int(batch, N, K, 16, F32_SPAN, device)


# ----------------------------------------------------------------------------------------------------------------------
# reference
# ----------------------------------------------------------------------------------------------------------------------
TERMS3 = (("hi", "hi"), ("hi", "lo"), ("lo", "hi"))
TERMS1 = (("hi", "hi"),)


def _plane(op, which):
    return op.ih if which == "hi" else op.il


def accumulators(A, B, single):
    """fp64 torch.bmm of the integer terms -> (acc, sum of |terms|, what the mode must NOT add: a_lo b_lo for three passes,
    a_hi b_lo + a_lo b_hi for the single pass)"""
    acc = mag = None
    for ta, tb in (TERMS1 if single else TERMS3):
        a, b = _plane(A, ta).double(), _plane(B, tb).double().transpose(1, 2)
        t, m = torch.bmm(a, b), torch.bmm(a.abs(), b.abs())
        acc, mag = (t, m) if acc is None else (acc + t, mag + m)
    bt = lambda p: p.double().transpose(1, 2)
    if single:
        return acc, mag, torch.bmm(A.ih.double(), bt(B.il)) + torch.bmm(A.il.double(), bt(B.ih))
    return acc, mag, torch.bmm(A.il.double(), bt(B.il))


def f32_accumulators(a, b):
    a, b = a.double(), b.double().transpose(1, 2)
    return torch.bmm(a, b), torch.bmm(a.abs(), b.abs())


def epilogue_inputs(M, N, batch, device, names):
    """the integer inputs of the epilogue, by name (functions of (batch, row, column)):
    add, res_hi / res_lo, addp_hi / addp_lo (planes of the GATED addend) in [-63, 63]; gate, addp_gate: hash bits;
    maskv: the values of a bf16 gate plane in [-3, 3] (gate = value > 0: zeros and negatives are closed gates);
    rgb_g (batch * M, 3), rgb_w (3, N) in [-3, 3]; T (3, N) in [-4, 4], tau (3), rgb0 (batch * M, 3) in [-63, 63]"""
    e = {}
    spans = dict(add=(21, F32_SPAN), res_hi=(22, F32_SPAN), res_lo=(23, F32_SPAN), addp_hi=(24, F32_SPAN), addp_lo=(25, F32_SPAN),
                 maskv=(28, 3))
    for n in names:
        if n in spans:
            e[n] = hash_int(batch, M, N, *spans[n], device)
        elif n in ("gate", "addp_gate"):
            e[n] = hash_bit(batch, M, N, 26 if n == "gate" else 27, device)
        elif n == "rgb_g":
            e[n] = hash_int(1, batch * M, 3, 29, RGB_SPAN, device)[0]
        elif n == "rgb_w":
            e[n] = hash_int(1, 3, N, 30, RGB_SPAN, device)[0]
        elif n == "T":
            e[n] = hash_int(1, 3, N, 31, TORGB_SPAN, device)[0]
        elif n == "tau":
            e[n] = torch.tensor(TAU, dtype=torch.int64, device=device)
        elif n == "rgb0":
            e[n] = hash_int(1, batch * M, 3, 32, F32_SPAN, device)[0]
        else:
            raise KeyError(n)
    if "maskv" in e:
        e["gate"] = e["maskv"] > 0
    for n in ("gate", "addp_gate"):                 # gates are neither mostly open nor mostly closed
        if n in e:
            assert 0.25 < float(e[n].float().mean()) < 0.75, n
    return e


def times_slope(v, slope):
    """v * slope as the kernels form it: one fp32 multiplication by the descriptor's fp32 slope (exact for 0.25)"""
    assert torch.equal(v.float().double(), v), "the value in front of the slope must be an fp32 number"
    return (v.float() * torch.tensor(slope, dtype=torch.float32, device=v.device)).double()


def epilogue(acc, mag, e, slope, act=0, gain=1.0, addp_gain=None, order="documented"):
    """the epilogue on fp64 accumulators, in the order cips3d_hip.h documents -> dict:
      CU (the value stored as C_unmasked), pre (what the activation sees), act (the value right after it: the bf16 mask_out
      plane, bits = act > 0), v (the final value: C, the planes, the ToRGB sums' input), mag (sum of |terms| behind v),
      part (N/128, batch*M, 4) and rgb_acc / rgb_new (batch*M, 3): the ToRGB partials and the finished sums (accumulate /
      not), pmag: the sums of |v T| per partial, rmag: of everything behind a finished sum.
    gain: cips_gemm_f32's act 2 (after the activation, or folded into the mask factor).
    order = "res_before_gate": a deliberately wrong epilogue for the yardstick's own test."""
    o = {}
    v = acc
    if "add" in e:
        v, mag = v + e["add"], mag + e["add"].abs()
    if "addp_hi" in e:
        p = (e["addp_hi"] + e["addp_lo"]).double()
        v, mag = v + torch.where(e["addp_gate"], p, p * addp_gain), mag + p.abs() * addp_gain
    if "rgb_g" in e:
        B, M, N = acc.shape
        v = v + (e["rgb_g"].double() @ e["rgb_w"].double()).view(B, M, N)
        mag = mag + (e["rgb_g"].double().abs() @ e["rgb_w"].double().abs()).view(B, M, N)
    res = (e["res_hi"] + e["res_lo"]).double() if "res_hi" in e else None
    if order == "res_before_gate":
        v, res = v + res, None
    o["CU"] = v
    if "gate" in e:
        if gain != 1.0:          # cips_gemm_f32: v *= (mask > 0 ? 1 : slope) * gain, the factor formed first
            f32g = torch.tensor(gain, dtype=torch.float32, device=v.device)
            fac = torch.where(e["gate"], f32g, torch.tensor(slope, dtype=torch.float32, device=v.device) * f32g)
            v, mag = (v.float() * fac).double(), mag * gain
        else:
            v = torch.where(e["gate"], v, times_slope(v, slope))
    if act:
        o["pre"] = v
        v = torch.where(v > 0, v, times_slope(v, slope))
        if gain != 1.0:
            v, mag = (v.float() * torch.tensor(gain, dtype=torch.float32, device=v.device)).double(), mag * gain
    o["act"] = v
    if res is not None:
        v, mag = v + res, mag + res.abs()
    o["v"], o["mag"] = v, mag
    if "T" in e:
        B, M, N = acc.shape
        T = e["T"].double().t().reshape(1, N // 128, 128, 3)
        yT = v.reshape(B * M, N // 128, 128, 1) * T
        part = yT.sum(2).permute(1, 0, 2)                                     # (blocks, rows, 3)
        o["pmag"] = yT.abs().sum(2)
        o["part"] = torch.cat([part, torch.zeros_like(part[..., :1])], -1)    # the fourth float is 0
        o["rgb_new"] = e["tau"].double() + part.sum(0)
        o["rgb_acc"] = o["rgb_new"] + e["rgb0"].double()
        o["rmag"] = o["pmag"].sum(1) + e["tau"].abs().double() + e["rgb0"].abs().double()
    return o


def split(v):
    """expected planes of an fp64 value that is an fp32 number: round to nearest even, like split2 in the library"""
    f = v.float()
    assert torch.equal(f.double(), v)
    hi = f.bfloat16()
    return hi, (f - hi.float()).bfloat16()


def pack_bits(b):
    """bool (..., N) -> uint8 (..., N/8), bit c & 7 of byte c >> 3"""
    w = (1 << torch.arange(8, device=b.device)).to(torch.int32)
    return (b.reshape(*b.shape[:-1], -1, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def _all_distinct(keys):
    s = keys.sort(dim=-1).values
    return bool((s[..., 1:] != s[..., :-1]).all())


def assert_conditions(o, lolo, unit, what, acc5=False):
    """What the REFERENCE must satisfy for the comparison to mean something (no kernel output takes part):
      * every value is a multiple of `unit` (1, or 1/4 behind the quarter slope) and sum |terms| / unit < 2^24 at every
        output — and for every 128-column ToRGB partial and every finished rgb sum — so that every fp32 evaluation is exact;
      * no two rows and no two columns of one batch of the expected output are equal, and no two batches are (compared
        through 64-bit linear hashes of the integer rows: different hashes prove different rows);
      * adding the term the kernels must not compute, a_lo b_lo, changes more than half of the accumulators (every later
        step of the epilogue is one-to-one, so it changes the outputs where it changes the accumulator);
      * acc5 (slope 0.2, no addend): every accumulator in front of the slope is 5 m and fl(5 m * 0.2f) = m."""
    v = o["v"]
    assert float(o["mag"].max()) / unit < LIMIT, (what, float(o["mag"].max()))
    q = v / unit
    if unit != 1 or acc5:
        assert torch.equal(q, q.round()), what
    if "part" in o:
        assert float(o["pmag"].max()) / unit < LIMIT and float(o["rmag"].max()) / unit < LIMIT, what
    if acc5:
        pre = o["pre"] if "pre" in o else o["CU"]
        m = pre / 5
        assert torch.equal(m, m.round()) and float(m.abs().max()) < 2 ** 21, what
        assert torch.equal(times_slope(pre, 0.2), m), what
    # distinct rows / columns / batches (v is an fp32 number: its bit pattern is an exact integer key)
    k = v.float().view(torch.int32).to(torch.int64)
    B, M, N = k.shape
    g = torch.Generator().manual_seed(7)
    wn = torch.randint(-2 ** 62, 2 ** 62, (N,), generator=g).to(k.device)
    wm = torch.randint(-2 ** 62, 2 ** 62, (M,), generator=g).to(k.device)
    rows, cols = (k * wn).sum(2), (k * wm.view(1, M, 1)).sum(1)          # int64 arithmetic wraps: still a function of the row
    assert M == 1 or _all_distinct(rows), (what, "two equal rows")
    assert N == 1 or _all_distinct(cols), (what, "two equal columns")
    assert B == 1 or _all_distinct((rows * wm).sum(1)), (what, "two equal batches")
    if lolo is not None:
        assert float((lolo != 0).float().mean()) > 0.5, (what, "a_lo b_lo would go unnoticed")


# ----------------------------------------------------------------------------------------------------------------------
# emulation
# ----------------------------------------------------------------------------------------------------------------------
def emulate(A, B, order, terms=TERMS3):
    """plain fp32 torch evaluation: the k-tiles (32 deep) visited in `order`, one fp32 addition per term and tile.
    terms: the (A plane, B plane) pairs, or a function k-tile -> pairs."""
    acc = torch.zeros(A.ih.shape[0], A.ih.shape[1], B.ih.shape[1], dtype=torch.float32, device=A.ih.device)
    for kt in order:
        ks = slice(kt * BK, (kt + 1) * BK)
        for ta, tb in (terms(kt) if callable(terms) else terms):
            acc = acc + torch.bmm(_plane(A, ta)[:, :, ks].float(), _plane(B, tb)[:, :, ks].float().transpose(1, 2))
    return acc


# ----------------------------------------------------------------------------------------------------------------------
# the GPU case list (tests/test_gpu_gemm_exact.py runs it; tests/test_gemm_exact_cpu.py checks the conditions on all of it)
# ----------------------------------------------------------------------------------------------------------------------
# NT epilogue flavours: the eleven of tests/test_gpu_gemm_bf16.py, C and P together, the transposed planes (ldt a multiple of 8:
# 16-byte stores; ldt a multiple of 4 only: element stores), the bf16 gate planes (gate_bits = 0).
# name -> (epilogue inputs, act, outputs)
NT_FLAVOURS = {
    "fwd": ((), 1, ("P", "bits")),
    "fwd_res": (("res_hi", "res_lo"), 1, ("P", "bits")),
    "fwd_torgb": (("T", "tau", "rgb0"), 1, ("P", "bits", "torgb")),
    "fwd_res_torgb": (("res_hi", "res_lo", "T", "tau", "rgb0"), 1, ("P", "bits", "torgb")),
    "gate": (("gate",), 0, ("P",)),
    "gate_res": (("gate", "res_hi", "res_lo"), 0, ("P",)),
    "add": (("add", "gate"), 0, ("P", "CU")),
    "add_rgb": (("add", "gate", "rgb_g", "rgb_w"), 0, ("P", "CU")),
    "addp": (("addp_hi", "addp_lo", "addp_gate", "gate"), 0, ("P",)),
    "addp_rgb": (("addp_hi", "addp_lo", "addp_gate", "gate", "rgb_g", "rgb_w"), 0, ("P",)),
    "c32": ((), 0, ("C",)),
    "c_p": ((), 0, ("C", "P")),
    "t8": ((), 0, ("P", "T")),
    "t4": ((), 0, ("T",)),
    "fwd16": ((), 1, ("P", "act16")),
    "gate16": (("maskv",), 0, ("P",)),
    "gate16_res": (("maskv", "res_hi", "res_lo"), 0, ("P",)),
}
BIT_FLAVOURS = ("fwd", "fwd_res", "fwd_torgb", "fwd_res_torgb", "gate", "gate_res", "add", "add_rgb", "addp", "addp_rgb")
V3_ONLY = ("fwd_torgb", "fwd_res_torgb", "addp", "addp_rgb")


def slopes_of(flavour):
    """0.25 everywhere; the production 0.2 where the slope is used and no addition follows the gate (no `res`)"""
    names, act, _ = NT_FLAVOURS[flavour]
    uses = act or "gate" in names or "maskv" in names
    return (0.25, 0.2) if uses and "res_hi" not in names else (0.25,)


def nt_route(c):
    """Where gemm_nt (gemm_bf16x3.hip) sends the case, by its documented rule: "v3", "wide", "256x128", or the refusal
    "invalid" (hipErrorInvalidValue: bit planes with N % 32) / "unsupported" (hipErrorNotSupported: ToRGB partials or the
    planes addend on a shape or kernel choice the v3 kernel does not take)."""
    M, N, K, kernel, single, f = c["M"], c["N"], c["K"], c["kernel"], c["single"], c["flavour"]
    names, _, outs = NT_FLAVOURS[f]
    bits = f in BIT_FLAVOURS
    if bits and (N % 32 or c.get("ldp8")):          # ldp8: the test pads ldp to N + 8 instead of a multiple of 32
        return "invalid"
    has_add = "add" in names or "addp_hi" in names
    has_mask = "gate" in names or "maskv" in names
    has_res = "res_hi" in names
    combo = not (has_add and not has_mask) and not (has_res and (has_add or has_mask))
    if kernel == 2 and M % 256 == 0 and N % 256 == 0 and K % (128 if single else 64) == 0 and "T" not in outs and combo \
            and (bits or not (has_mask or "act16" in outs)):
        return "v3"
    if f in V3_ONLY:
        return "unsupported"
    if kernel >= 2 and not single and "T" not in outs and N % 8 == 0 and combo:
        return "wide"
    return "256x128"


def nt_reference(c, acc, mag, device):
    """-> (epilogue inputs, expected outputs, unit) of an NT case from its accumulators"""
    names, act, _ = NT_FLAVOURS[c["flavour"]]
    e = epilogue_inputs(c["M"], c["N"], c["batch"], device, names)
    slope = c["slope"]
    o = epilogue(acc, mag, e, slope, act=act, addp_gain=round(1 / slope))
    uses = act or "gate" in e
    return e, o, (0.25 if uses and slope == 0.25 else 1)


def nt_acc5(c):
    """slope 0.2 without an addend: every accumulator in front of the slope is 5 m (assert_conditions)"""
    names, act, _ = NT_FLAVOURS[c["flavour"]]
    return c["slope"] == 0.2 and not any(n in names for n in ("add", "addp_hi", "rgb_g"))


def f32_reference(c, device):
    """cips_gemm_f32: -> (A, B int64 logical operands, epilogue inputs, expected dict, unit).  Epilogue of gemm_f32.hip:
    acc * alpha + bias, + bias_m, + add, + rgb term, store C_unmasked, * (mask > 0 ? 1 : slope) * gain, act (* gain), C,
    C2 = C + resid.  alpha = 0.5, slope = 0.25 and gain = 2 keep every step exact (unit 1/8)."""
    M, N, K, batch, epi = c["M"], c["N"], c["K"], c["batch"], c["epi"]
    a, b = f32_operands(M, N, K, batch, device)
    acc, mag = f32_accumulators(a, b)
    acc, mag = acc * c["alpha"], mag * c["alpha"]
    e, x = {}, {}
    if "bias" in epi and "bias_m" not in epi:
        x["bias"] = hash_int(1, 1, N, 33, F32_SPAN, device)[0, 0]
        acc, mag = acc + x["bias"], mag + x["bias"].abs()
    if "bias_m" in epi:
        x["bias_m"] = hash_int(1, 1, M, 34, F32_SPAN, device)[0, 0]
        acc, mag = acc + x["bias_m"].view(1, M, 1), mag + x["bias_m"].abs().view(1, M, 1)
    if "resid" in epi:
        x["resid"] = hash_int(batch, M, N, 35, F32_SPAN, device)
    if "add" in epi:
        e = epilogue_inputs(M, N, batch, device, ("add", "rgb_g", "rgb_w", "maskv"))
    # act 2 scales by act_gain behind the activation AND inside the mask factor: "add_rgb_mask_gain" has both
    act = 1 if ("act1" in epi or "resid" in epi) else 2 if ("act2" in epi or "gain" in epi) else 0
    gain = 2.0 if act == 2 else 1.0
    x["act"], x["gain"] = act, gain
    o = epilogue(acc, mag, e, 0.25, act=act, gain=gain)
    if "resid" in x:
        o["C2"], o["mag"] = o["v"] + x["resid"], o["mag"] + x["resid"].abs()
    return a, b, e, x, o, 0.125


def nt_cases(cus):
    """-> list of dicts (kernel, M, N, K, batch, flavour, slope, single, + lda / ldb / strideA / strideB, many, ldp8).
    The ragged shapes of the k sweeps have N % 32 != 0, where the entry refuses gate bit planes; the flavour sweeps therefore
    add (300, 160) for the 256x128 kernel and (264, 288) for the wide one: ragged in both directions, 2 x 2 tiles, N % 32 == 0."""
    c = []

    def add(kernel, M, N, K, batch, flavour, single, slope=0.25, **kw):
        c.append(dict(kernel=kernel, M=M, N=N, K=K, batch=batch, flavour=flavour, slope=slope, single=single, **kw))

    for single in (False, True):
        # 256x128 kernel: 3-stage ring of 32-deep k-tiles — fewer k-tiles than the ring, exactly the ring, a wrapped ring
        for (M, N) in ((256, 128), (264, 136), (37, 40), (300, 200), (8, 32)):
            for K in (32, 64, 96, 128, 160):
                add(1, M, N, K, 2, "c_p", single)
        add(1, 264, 136, 512, 2, "c_p", single)
        add(1, 256, 128, 64, cus + 1, "c_p", single, many=True)                       # a second tile per workgroup
        add(1, 264, 136, 32, 3, "c_p", single, strideB=0)                             # one weight for all images
        add(1, 37, 40, 96, 2, "c_p", single, lda=104, ldb=112, strideA=37 * 104 + 8, strideB=40 * 112 + 16)
        for (M, N) in ((300, 160), (8, 32)):                                          # N % 32 == 0: the bit planes are taken
            for f in NT_FLAVOURS:
                for s in slopes_of(f):
                    add(1, M, N, 96, 2, f, single, s)
        for f in ("c32", "t8", "t4", "fwd16", "gate16", "gate16_res"):               # ragged N: no bit planes
            add(1, 300, 200, 96, 2, f, single)
        add(1, 300, 200, 96, 2, "fwd16", single, 0.2)
        add(1, 300, 200, 96, 2, "gate16", single, 0.2)
        add(1, 300, 160, 96, 2, "fwd", single, ldp8=True)                             # bit planes with ldp % 32 != 0: refused
        add(2, 256, 256, 128, 2, "gate", single, ldp8=True)
        # v3 kernel (interior shapes; 64-deep k-tiles in the single-pass form)
        ks = (128, 256, 384) if single else (64, 128, 192)
        for (M, N) in ((256, 256), (512, 768)):
            for K in ks:
                add(2, M, N, K, 2, "c_p", single)
        add(2, 256, 256, 512, 2, "c_p", single)
        add(2, 256, 256, ks[0], cus + 1, "c_p", single, many=True)
        for f in NT_FLAVOURS:
            for s in slopes_of(f):
                add(2, 256, 256, ks[0], 2, f, single, s)
        add(2, 512, 768, ks[1], 2, "fwd_res_torgb", single)
        add(2, 512, 768, ks[1], 2, "addp_rgb", single)
        add(2, 512, 768, ks[1], 2, "addp_rgb", single, 0.2)
        add(2, 264, 256, ks[0], 2, "c_p", single)             # refused by v3: falls through to the wide / the 256x128 kernel
        add(2, 264, 256, ks[0], 2, "fwd", single)
    # wide kernel (3-pass only: the single-pass family has no such kernel and never runs it)
    for (M, N) in ((256, 256), (520, 264), (300, 96), (1024, 768)):
        for K in (32, 64, 96, 128):
            add(3, M, N, K, 2, "c_p", False)
    add(3, 520, 264, 512, 2, "c_p", False)
    add(3, 256, 256, 64, cus + 1, "c_p", False, many=True)
    for (M, N) in ((300, 96), (264, 288)):
        for f in NT_FLAVOURS:
            for s in slopes_of(f):
                add(3, M, N, 96, 2, f, False, s)
    for f in ("c32", "fwd16", "gate16"):
        add(3, 520, 264, 96, 2, f, False)
    add(3, 520, 264, 96, 2, "c_p", True)                      # cips_gemm_bf16 with kernel = 3: the 256x128 kernel, never three passes
    add(3, 256, 256, 128, 2, "fwd", True)
    add(3, 264, 288, 96, 2, "add", False, ldp8=True)
    return list({case_id(x): x for x in c}.values())          # a flavour sweep repeats the c_p case of the k sweep at its shape


def km_cases(cus):
    """K-major: dicts (kernel, M, N, K, batch, single, groups (0: cips_gemm_*_km, else the grouped entry), many, ksplit)"""
    c = []

    def add(kernel, M, N, K, batch, single, groups=0, **kw):
        c.append(dict(kernel=kernel, M=M, N=N, K=K, batch=batch, single=single, groups=groups, **kw))

    for single in (False, True):
        for M in (64, 128, 136, 200, 520):                    # <= 128: the 128-row form (2-stage ring), else the 256-row form
            for N in (72, 128, 264):
                for K in (32, 64, 96, 128):
                    add(1, M, N, K, 2, single)
        add(1, 128, 72, 512, 2, single)
        add(1, 200, 264, 512, 2, single)
        add(1, 64, 72, 64, 2 * cus + 1, single, many=True)    # two workgroups per CU
        add(1, 136, 72, 64, cus + 1, single, many=True)
        add(1, 200, 264, 64, 4, single, ksplit=True)          # the batch as a K split
        # 256x256 tiles
        ks = (128, 192) if single else (32, 64, 96, 128)
        for (M, N) in ((256, 256), (264, 520)):
            for K in ks:
                add(2, M, N, K, 2, single)
                add(2, M, N, K, 2, single, groups=2)
        add(2, 264, 520, 512, 2, single)
        for gcount in (1, 4):
            add(2, 264, 520, ks[-1], 1, single, groups=gcount)
        if not single:
            add(2, 256, 256, 32, 2, single, groups=4)         # the one-k-tile kernel, grouped
        add(2, 256, 256, ks[0] if single else 64, cus + 1, single, many=True)
        add(2, 256, 256, ks[0] if single else 32, (cus + 3) // 2, single, groups=2, many=True)
    return c


F32_SHAPES = ((128, 128, 32), (200, 36, 64), (132, 260, 12), (100, 512, 100), (64, 512, 148))
F32_EPILOGUES = ("plain", "bias_act1", "bias_m_act2", "resid_c2", "add_rgb_mask", "add_rgb_mask_gain")


def f32_cases():
    c = []
    for (M, N, K) in F32_SHAPES:
        for a_k in (False, True):
            for b_n in (False, True):
                for alpha in (1.0, 0.5):
                    c.append(dict(M=M, N=N, K=K, batch=2, a_k=a_k, b_n=b_n, alpha=alpha, epi="plain"))
    for (M, N, K) in ((200, 36, 64), (132, 260, 12)):
        for epi in F32_EPILOGUES[1:]:
            c.append(dict(M=M, N=N, K=K, batch=2, a_k=False, b_n=M == 132, alpha=0.5 if epi == "bias_act1" else 1.0, epi=epi))
    return c


def case_id(c):
    parts = []
    for k, v in c.items():
        if k == "batch" and c.get("many"):
            v = "tiles>CUs"
        if k == "single":
            k, v = "mode", ("bf16" if v else "bf16x3")
        if isinstance(v, bool):
            if v:
                parts.append(k)
        elif v is not None:
            parts.append(f"{k}{v}" if k in ("M", "N", "K", "kernel", "groups") else str(v) if k in ("flavour", "mode", "epi") else f"{k}:{v}")
    return "-".join(parts)
