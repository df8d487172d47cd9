"""References for the helper kernels around the INR head's GEMMs (cips3d_amd/csrc/modfc.hip), built on the CPU from seeded
inputs, and the case tables that tests/test_head_kernel_refs_cpu.py (CPU) and tests/test_gpu_head_kernels.py (GPU) share.

Two restatements of every operation:
  * float64, the truth: torch autograd of the rule of exp/comm/models/mod_conv_fc.py:470-489 for the modulate / demodulate
    prep, plain matrix products for ToRGB;
  * float32, the yardstick: the closed form the header of modfc.hip states (c, du, dW, ds), op by op in float32, and the same
    matrix products in float32.  Its own error against the float64 truth on a test's inputs is what a correct float32 kernel
    can be expected to show on them; the GPU tests hold every kernel to a small multiple of it (yardstick())."""
import torch

EPS = 1e-8                       # SinStyleMod's eps (mod_conv_fc.py:470-489), the default of every prep entry
SLOPE = 0.2                      # LeakyReLU slope of the head (ops.LRELU_SLOPE)
F32_ROUND = 2.0 ** -24           # half an ulp of float32: the error of ONE correctly rounded float32 result


# --------------------------------------------------------------------------------------
# modulate / demodulate prep
# --------------------------------------------------------------------------------------
def modfc_inputs(in_dim, out_dim, B, seed, wscale=1.0):
    """W (in, out) ~ N(0, wscale^2), s (B, in) ~ N(0, 0.25), G = dL/dWb (B, in, out) ~ N(0, 1), float32.  in_dim = 1 (see
    is_degenerate): |W| >= 0.5 wscale and s >= -0.5, because there the true gradients are eps G / (|W|^3 (s+1)^2), which an
    entry of W near zero makes as large as one pleases"""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(in_dim, out_dim, generator=g)
    s = torch.randn(B, in_dim, generator=g) * 0.5
    G = torch.randn(B, in_dim, out_dim, generator=g)
    if is_degenerate(in_dim):
        W = torch.where(W < 0, W - 0.5, W + 0.5)
        s = s.clamp_min(-0.5)
    return W * wscale, s, G


def modfc_ref64(W, s, G, eps=EPS):
    """float64 autograd of Wb = W (s+1) rsqrt(sum_in (W (s+1))^2 + eps) -> wb (B, in, out), demod (B, out), dW (in, out), ds (B, in)
    for the upstream gradient G = dL/dWb"""
    Wd = W.double().requires_grad_(True)
    sd = s.double().requires_grad_(True)
    u = Wd.unsqueeze(0) * (sd.unsqueeze(-1) + 1)
    demod = torch.rsqrt(u.pow(2).sum(1) + eps)
    wb = u * demod.unsqueeze(1)
    (wb * G.double()).sum().backward()
    return wb.detach(), demod.detach(), Wd.grad, sd.grad


def modfc_f32(W, s, G, eps=EPS):
    """the closed form of modfc.hip's header, op by op in float32:  u = W (s+1), d = rsqrt(sum_k u^2 + eps), Wb = u d,
    c_n = sum_k G_kn u_kn, du = d (G - d^2 u c), dW_kn = sum_b (s_bk+1) du_bkn, ds_bk = sum_n W_kn du_bkn"""
    W, s, G = W.float(), s.float(), G.float()
    m = (s + 1).unsqueeze(-1)                                   # (B, in, 1)
    u = W.unsqueeze(0) * m                                      # (B, in, out)
    d = torch.rsqrt((u * u).sum(1) + torch.tensor(eps, dtype=torch.float32))          # (B, out)
    wb = u * d.unsqueeze(1)
    c = (G * u).sum(1)                                          # (B, out)
    dd = d.unsqueeze(1)
    du = dd * (G - dd * dd * u * c.unsqueeze(1))
    dW = (m * du).sum(0)
    ds = (W.unsqueeze(0) * du).sum(2)
    return wb, d, dW, ds


def split_ref(v):
    """float32 -> (hi, lo) bf16: hi = bf16(v) (round to nearest even), lo = bf16(v - hi): the kernels' operand split"""
    v = v.float()
    hi = v.bfloat16()
    lo = (v - hi.float()).bfloat16()
    return hi, lo


def split_ties(v):
    """where a float32 lies exactly midway between two neighbouring bf16 values (low half of the word 0x8000).  split_ref of
    hi + lo returns (hi, lo) again everywhere else; at a tie it cannot tell which neighbour the first split came from: a v0
    just below the midpoint splits into hi = the lower neighbour, lo = bf16(v0 - hi) ROUNDED UP to the half step, and hi + lo
    is the midpoint itself, which rounds to the even neighbour"""
    return (v.float().contiguous().view(torch.int32) & 0xFFFF) == 0x8000


# --------------------------------------------------------------------------------------
# ToRGB: rgb (M, 3) (+)= x (M, K) T^T (3, K) + bias
# --------------------------------------------------------------------------------------
def torgb_fwd_ref(x, w, bias=None, rgb0=None, dtype=torch.float64):
    y = x.to(dtype) @ w.to(dtype).t()
    if bias is not None:
        y = y + bias.to(dtype)
    return y if rgb0 is None else rgb0.to(dtype) + y


def torgb_bwd_w_ref(x, drgb, dtype=torch.float64):
    """dT (3, K) = drgb^T x, dbias (3) = sum_m drgb"""
    return drgb.to(dtype).t() @ x.to(dtype), drgb.to(dtype).sum(0)


def torgb_bwd_x_ref(drgb, w, add=None, mask=None, slope=SLOPE, dtype=torch.float64):
    """(the sum before the gate, the gated sum): dx = drgb T (+ add), times (mask > 0 ? 1 : slope) where a mask is given"""
    un = drgb.to(dtype) @ w.to(dtype)
    if add is not None:
        un = un + add.to(dtype)
    out = un if mask is None else un * torch.where(mask > 0, torch.ones((), dtype=dtype), torch.full((), slope, dtype=dtype))
    return un, out


# --------------------------------------------------------------------------------------
# error measures and the yardstick
# --------------------------------------------------------------------------------------
def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def max_rel(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def yardstick(err_f32):
    """the float32 restatement's own error, but never below 2^-24: on a handful of outputs the restatement can happen to round
    every one of them correctly (error far below the format's resolution, or 0), and no float32 kernel with another order of
    operations can be held to a multiple of that"""
    return max(err_f32, F32_ROUND)


# --------------------------------------------------------------------------------------
# case tables of the prep kernels.  Form codes (include/cips3d_hip.h), worked out by hand from the rule:
#   forward   bit 0 (1): every out_dim % 4 == 0;  bit 1 (2): and every in_dim % 8 == 0
#   backward  0 unless every out_dim % 4 == 0 and B <= 64 and max out_dim <= 1024;  2: max out_dim <= 512;  4: <= 1024
# --------------------------------------------------------------------------------------
class ModfcCase:
    def __init__(self, name, shapes, B, form, wscale=1.0, eps=EPS, edge=""):
        self.name, self.shapes, self.B, self.form, self.wscale, self.eps, self.edge = name, shapes, B, form, wscale, eps, edge

    def inputs(self):
        """[(W, s, G)] per job, seeded by the job's position and shape"""
        return [modfc_inputs(i, o, self.B, 7000 + 131 * j + 17 * i + o + self.B, self.wscale)
                for j, (i, o) in enumerate(self.shapes)]

    def __repr__(self):
        return self.name


ALTERNATING = [(8, 4), (4, 8)]
JOBS25 = [ALTERNATING[j % 2] for j in range(25)]
MAXJOBS = 24                     # cips_modfc_max_jobs(): the wrappers cut longer lists into calls of at most this many jobs

MODFC_FWD_CASES = [
    ModfcCase("one_lane", [(8, 4)], 1, 3, edge="16-byte sums + 64x64 tiles; one lane of one tile; B = 1"),
    ModfcCase("tile_tail", [(64, 68)], 2, 3, edge="the second 64-column tile holds one 4-column lane"),
    ModfcCase("ragged_k_wide", [(72, 1028)], 2, 3, edge="ragged second k-tile; out_dim above 1024"),
    ModfcCase("sums16_tiles32", [(36, 520), (8, 4)], 3, 1, edge="in_dim % 8 != 0: 16-byte sums, 32x32 tiles; second job far smaller than the grid"),
    ModfcCase("maxima_apart", [(8, 132), (136, 4)], 2, 3, edge="max_in and max_out from different jobs: both jobs leave blocks idle"),
    ModfcCase("scalar_33", [(33, 33)], 2, 0, edge="scalar forms; one-lane tails of the 32-column blocks and 32x32 tiles"),
    ModfcCase("in_1", [(1, 8)], 2, 1, edge="in_dim = 1 (out_dim % 4 == 0: 16-byte sums, 32x32 tiles); fewer rows than k-groups"),
    ModfcCase("scalar_small", [(5, 30), (40, 3)], 3, 0, edge="scalar forms; in_dim below the 8 k-groups; out_dim below 4"),
    ModfcCase("jobs_25", JOBS25, 2, (1, 3), edge="24 + 1 jobs: the wrapper's second call holds one job"),
    ModfcCase("jobs_24", JOBS25[:24], 2, (1,), edge="exactly MAXJOBS jobs: one call"),
    ModfcCase("tiny_w", [(64, 96)], 3, 3, wscale=1e-4, edge="sum u^2 ~ 8e-7 against eps 1e-8"),
    ModfcCase("tiny_w_eps", [(64, 96)], 3, 3, wscale=1e-4, eps=1e-6, edge="... against eps 1e-6: demod moves by tens of percent"),
]
MODFC_BWD_CASES = [
    ModfcCase("one_lane", [(5, 4)], 1, 2, edge="one lane; in_dim no multiple of the 4 waves of a block; B = 1"),
    ModfcCase("chunk_tail", [(12, 260)], 3, 2, edge="the second 256-column chunk holds one lane"),
    ModfcCase("four_chunks", [(8, 516), (8, 1024)], 2, 4, edge="third chunk with one lane; full fourth chunk"),
    ModfcCase("wide_scalar", [(8, 1028)], 2, 0, edge="every out_dim % 4 == 0 but the largest above 1024: scalar"),
    ModfcCase("B_64", [(16, 64)], 64, 2, edge="last B of the fused form: lane 63 keeps image 63"),
    ModfcCase("B_65", [(16, 64)], 65, 0, edge="first B of the scalar form; the co-resident entry refuses"),
    ModfcCase("in_1", [(1, 8)], 2, 2, edge="co-resident column sums: three empty row segments; degenerate gradients"),
    ModfcCase("in_2", [(2, 8)], 2, 2, edge="two empty row segments"),
    ModfcCase("in_3", [(3, 8)], 2, 2, edge="one empty row segment"),
    ModfcCase("in_5", [(5, 8)], 2, 2, edge="uneven row segments 1, 1, 1, 2"),
    ModfcCase("mixed", [(64, 96), (40, 30)], 3, 0, edge="one out_dim % 4 != 0 moves both jobs to the scalar form"),
    ModfcCase("jobs_25", JOBS25, 2, (2, 2), edge="24 + 1 jobs: the wrapper's second call holds one job"),
]
# the extra shapes the issue's measurements name (CPU only: the restatement's error on ordinary and large layers)
MODFC_CPU_EXTRA = [
    ModfcCase("ordinary", [(64, 96)], 3, 3),
    ModfcCase("head_width", [(512, 1024)], 8, 3),
    ModfcCase("many_images", [(3, 4)], 64, 1),
    ModfcCase("odd_wide", [(33, 1028)], 5, 1),
    ModfcCase("tiny_w5", [(64, 96)], 3, 3, wscale=1e-5),
]


def forms_of(case):
    """the form code of every call the wrapper makes for this case (one per chunk of MAXJOBS jobs)"""
    return case.form if isinstance(case.form, tuple) else (case.form,)


# the tables reach every code of both queries
assert {f for c in MODFC_FWD_CASES for f in forms_of(c)} == {0, 1, 3}          # 2 alone cannot occur: bit 1 implies bit 0
assert {f for c in MODFC_BWD_CASES for f in forms_of(c)} == {0, 2, 4}


def is_degenerate(in_dim):
    """in_dim = 1: wb = +-(1 + O(eps)) whatever W and s, so the true dW and ds are cancellations of order eps.  A float32
    evaluation of du = d (G - d^2 u c) leaves its rounding there instead (relative error of order 1 against a truth of order
    eps), so these gradients are bounded ABSOLUTELY: degenerate_bound()"""
    return in_dim == 1


def degenerate_bound(W, G):
    return 1e-5 * float(G.abs().max()) * float(W.abs().max())
