"""GPU: every split-bf16 GEMM kernel (gemm_bf16x3.hip, gemm_bf16x3_wide.hip, gemm_bf16x3_v3.hip, gemm_bf16x3_km_wide.hip), in
both arithmetic modes (cips_gemm_bf16x3*: three passes, cips_gemm_bf16*: the hi planes only), and cips_gemm_f32, against the
exact integer reference of tests/gemm_exact.py: operand planes of small independent integers make every fp32 partial sum
exact, so each output element — fp32 C, hi / lo planes, transposed planes, gate bytes, C_unmasked, ToRGB partials and the
finished rgb — must EQUAL the reference bit for bit, and every guard row and padding element around the outputs (pre-filled
with NaN / 0xA5, leading dimensions larger than N) must still hold its sentinel.  No tolerance anywhere.

The descriptors are filled here from ops._x3_desc and handed to the library entry directly; the kernel is forced through the
descriptor field `kernel`, slope = 0.25 and addp_gain = 4 (every epilogue step exact), plus the production slope 0.2 (gain 5)
in the flavours in which no addition follows the gate.  gemm_exact.nt_route restates the dispatch rule of gemm_nt
(gemm_bf16x3.hip) and names the kernel each case is sent to in the test id (`->v3`, `->wide`, `->256x128`) or the refusal the
entry documents (`->unsupported`: hipErrorNotSupported 801 for ToRGB partials / the planes addend outside v3;
`->invalid`: hipErrorInvalidValue for bit planes with N % 32 != 0 or, `ldp8`, ldp % 32 != 0); refused calls must leave every output untouched.
Transposed planes T are never refused by the public entry: with kernel = 2 / 3 the 256x256-tile kernels decline them and
gemm_nt falls through to the 256x128 kernel, which the `t8` / `t4` cases exercise.

Which shape reaches which path, and why it is the smallest that does (batch 2 unless stated: two batch strides):

NT 256x128 kernel (kernel = 1; automatic for everything that does not fill the chip with 256x256 tiles)
  K = 32, 64 | 96 | 128, 160   fewer k-tiles than the 3-stage ring (1, 2: the prologue issues fewer than DIST tiles, every wait
                               is vmcnt(0) or the last-tile form) | exactly the ring | a wrapped ring (stage reuse, 4 and 5 tiles)
  (256, 128)                   one full tile: no clamped row, every store the 16-byte form
  (264, 136)                   one row / column group past the tile in both directions: a second, nearly empty tile each way
  (37, 40)                     below a wave's 64x64 sub-tile, M odd: clamped DMA rows, element-wise ragged stores
  (300, 200)                   two tiles each way with a ragged last one that several waves share
  (8, 32)                      fewer rows than one DMA row group, one MFMA column block
  batch = CUs + 1, K = 64      one tile more than workgroups: workgroup 0 runs a second tile behind its first epilogue
  strideB = 0, K = 32          one weight for all images (production: ops.py, the shared first-layer weight)
  lda, ldb, strideA, strideB padded   NaN between rows and batches of the operands
  flavours at (300, 160) / (8, 32): N % 32 == 0 so that the bit planes are accepted; at (300, 200): the bf16 gate planes,
  T and C where the bit planes are refused with hipErrorInvalidValue
NT wide kernel (kernel = 3, three passes only; the single-pass family has no such kernel: with kernel = 3 it runs the 256x128 one)
  K = 32 | 64, 96, 128         one k-tile (no DMA under the MFMAs) | 2-stage ring: both stages, first reuse, second reuse
  (256, 256) | (520, 264)      one full tile | 3 x 2 tiles, last row of tiles 8 rows, last column of tiles 8 columns
  (300, 96) | (1024, 768)      N below half a tile (the wn = 1 waves store nothing) | 4 x 3 interior tiles
  batch = CUs + 1, K = 64      a second tile per workgroup: its first k-tile streams into stage 0 under the first epilogue
  flavours at (300, 96), (264, 288); gate_res, T and the v3-only flavours fall through / are refused as nt_route says
NT v3 kernel (kernel = 2; interior shapes: M, N % 256 == 0, K % 64 == 0, single pass K % 128 == 0)
  K = 64, 128, 192 (single pass 128, 256, 384)   two k-tiles (the whole contraction streams in under the previous epilogue), 4, 6
  (256, 256) | (512, 768)      one tile | 2 x 3 tiles
  batch = CUs + 1              a second tile per workgroup
  (264, 256)                   refused by v3: falls through to the wide kernel (three passes) / the 256x128 kernel (single pass)
  all flavours at (256, 256) incl. ToRGB partials + cips_torgb_finish and the planes addend; the two widest at (512, 768)
One K = 512 case per kernel: the head's contraction length.
K-major, cips_gemm_*_km with kernel = 1
  M = 64, 128 | 136, 200, 520  the 128-row form (4 waves, 2-stage ring; half a tile, a full one) | the 256-row form (8 waves,
                               3-stage ring: 8 rows past half a tile, ragged, two full tiles + 8 rows)
  N = 72, 128, 264             ragged below a tile, one tile, two tiles + 8 columns;  K = 32 .. 128: as for the NT ring
  batch = 2 CUs + 1 / CUs + 1  a second tile per workgroup (the 128-row form runs two workgroups per CU)
  batch as a K split           four batches that are slices of one 256-long contraction, summed as ops._head_wgrad sums them
K-major 256x256 tiles (kernel = 2 and cips_gemm_*_km_grouped)
  (256, 256), (264, 520); K = 32: the one-k-tile kernel, K = 64, 96, 128: the v3 form (2, 3, 4 k-tiles); single pass
  K = 128, 192 (64-deep k-tiles, two or more: K = 64 is refused with 801); groups 1, 2, 4 with different operands, 5 refused
cips_gemm_f32: the four layouts at five shapes (full tile, ragged, K not a multiple of the 32-deep k-tile: 12, 100, 148),
  alpha 1 and 0.5, integer bias / bias_m, act 1 and act 2 (gain 2), resid + C2, add + rgb + C_unmasked + mask, padded ldc."""
import ctypes

import pytest
import torch

import gemm_exact as gx

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 801          # hipErrorInvalidValue, hipErrorNotSupported
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
NT_CASES = [dict(c, route=gx.nt_route(c)) for c in gx.nt_cases(CUS)]
KM_CASES = gx.km_cases(CUS)
F32_CASES = gx.f32_cases()


def dev():
    return torch.device("cuda:0")


def _id(c):
    r = c.get("route")
    return gx.case_id({k: v for k, v in c.items() if k != "route"}) + (f"->{r}" if r else "")


_OPS = {}


def _operands(key, make):
    """operands and accumulators of the last shape, shared by its flavours (never modified)"""
    if key not in _OPS:
        _OPS.clear()
        _OPS[key] = make()
    return _OPS[key]


def _entry(single, suffix=""):
    from cips3d_amd import _lib
    return getattr(_lib.load(), ("cips_gemm_bf16" if single else "cips_gemm_bf16x3") + suffix)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ----------------------------------------------------------------------------------------------------------------------
# NT
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", NT_CASES, ids=_id)
def test_nt(c):
    from cips3d_amd import _lib, ops
    d = dev()
    M, N, K, batch, single, route = c["M"], c["N"], c["K"], c["batch"], c["single"], c["route"]
    names, act, outs = gx.NT_FLAVOURS[c["flavour"]]
    okey = ("nt", M, N, K, batch, c.get("lda"), c.get("ldb"), c.get("strideA"), c.get("strideB"), single)

    def make():
        A, B = gx.x3_operands(M, N, K, batch, d, c.get("lda"), c.get("ldb"), c.get("strideA"), c.get("strideB"))
        return (A, B) + gx.accumulators(A, B, single)
    A, B, acc, mag, other = _operands(okey, make)
    runs = route not in ("invalid", "unsupported")
    if runs:
        e, o, unit = gx.nt_reference(c, acc, mag, d)
        gx.assert_conditions(o, other, unit, _id(c), acc5=gx.nt_acc5(c))
    else:
        e = gx.epilogue_inputs(M, N, batch, d, names)

    # auxiliary inputs and outputs share the padded leading dimension and batch stride (ldc / strideC, ldp / strideP)
    ld = N + 8 if c.get("ldp8") else (N + 31) // 32 * 32 + 32
    stride = M * ld + (0 if c.get("ldp8") else 64)
    g = (2 * ld + 63) // 64 * 64
    inp = lambda v, dt: gx.Strided(batch, M, N, ld, stride, dt, d, guard=g, values=v)
    bits_in = lambda b: gx.Strided(batch, M, N // 8, ld // 8, stride // 8, torch.uint8, d, guard=g, values=gx.pack_bits(b))
    out = lambda dt: gx.Guarded(batch, M, N, ld, stride, dt, d)
    planes = lambda hi, lo: ops.Planes(hi.data(), lo.data())
    keep, kw, gate_bits = [], {}, 0          # keep: the input buffers stay alive until the launch has run
    if "add" in e:
        keep.append(inp(e["add"], torch.float32)); kw["add"] = keep[-1].data()
    if "res_hi" in e:
        keep += [inp(e["res_hi"], gx.BF), inp(e["res_lo"], gx.BF)]; kw["res"] = planes(*keep[-2:])
    if "maskv" in e:
        keep.append(inp(e["maskv"], gx.BF)); kw["mask"] = keep[-1].data()
    elif "gate" in e:
        keep.append(bits_in(e["gate"])); kw["mask"] = keep[-1].data(); gate_bits |= 1
    if "addp_hi" in e:
        keep += [inp(e["addp_hi"], gx.BF), inp(e["addp_lo"], gx.BF), bits_in(e["addp_gate"])]
        kw["addp"] = (planes(*keep[-3:-1]), keep[-1].data())
    if "rgb_g" in e:
        keep += [e["rgb_g"].float().contiguous(), e["rgb_w"].float().contiguous()]; kw["rgb_g"], kw["rgb_w"] = keep[-2:]
    G = {}
    if "P" in outs:
        G["P_hi"], G["P_lo"] = out(gx.BF), out(gx.BF); kw["P"] = planes(G["P_hi"], G["P_lo"])
    if "C" in outs:
        G["C"] = out(torch.float32)
    if "CU" in outs:
        G["CU"] = out(torch.float32); kw["C_unmasked"] = G["CU"].data()
    if "bits" in outs:
        G["bits"] = gx.Guarded(batch, M, N // 8, ld // 8, stride // 8, torch.uint8, d); kw["mask_out"] = G["bits"].data(); gate_bits |= 2
    if "act16" in outs:
        G["act16"] = out(gx.BF); kw["mask_out"] = G["act16"].data()
    ldt = strideT = 0
    if "T" in outs:
        # t8: 16-byte stores of 8 rows; t4: ldt a multiple of 4 but not of 8 — element stores
        ldt = (M + 7) // 8 * 8 + 8 if c["flavour"] == "t8" else next(x for x in range(M + 1, M + 17) if x % 4 == 0 and x % 8)
        strideT = N * ldt + (8 if c["flavour"] == "t8" else 4)
        G["T_hi"], G["T_lo"] = (gx.Guarded(batch, N, M, ldt, strideT, gx.BF, d) for _ in range(2))
        kw["T"] = planes(G["T_hi"], G["T_lo"])
    nblk = max(N // 128, 1)
    if "torgb" in outs:
        keep.append(e["T"].float().contiguous())
        G["part"] = gx.Guarded(1, nblk * batch * M, 4, 4, 0, torch.float32, d)
        kw["torgb"] = (keep[-1], G["part"].data())

    desc = ops._x3_desc(planes(A.hi, A.lo), planes(B.hi, B.lo), M, N, K, A.ld, B.ld, batch, A.stride, B.stride,
                        C=G["C"].data() if "C" in G else None, act=act, gate_bits=gate_bits, ldt=ldt, strideT=strideT, **kw)
    desc.ldc = desc.ldp = ld
    desc.strideC = desc.strideP = stride
    desc.slope = c["slope"]
    if "addp_hi" in e:
        desc.addp_gain = float(round(1 / c["slope"]))
    desc.kernel = c["kernel"]
    if "torgb" in outs or "addp_hi" in e:      # the queries agree with the entry
        q = _entry(single, "_fuses_torgb" if "torgb" in outs else "_takes_addp")
        assert bool(q(ctypes.byref(desc))) == (route == "v3")
    rc = _entry(single)(ctypes.byref(desc), _stream())
    torch.cuda.synchronize()
    tag = _id(c)
    if not runs:
        assert rc == (INVALID if route == "invalid" else UNSUPPORTED), (tag, rc)
        for k, b in G.items():
            b.untouched(f"{tag}: {k}")
        return
    assert rc == 0, (tag, rc)
    if "P" in outs:
        hi, lo = gx.split(o["v"])
        G["P_hi"].check(hi, f"{tag}: hi plane"); G["P_lo"].check(lo, f"{tag}: lo plane")
    if "C" in outs:
        G["C"].check(o["v"].float(), f"{tag}: C")
    if "CU" in outs:
        G["CU"].check(o["CU"].float(), f"{tag}: C_unmasked")
    if "bits" in outs:
        G["bits"].check(gx.pack_bits(o["act"] > 0), f"{tag}: gate bytes")
        assert 0.25 < float((o["act"] > 0).float().mean()) < 0.75, tag
    if "act16" in outs:
        G["act16"].check(o["act"].float().bfloat16(), f"{tag}: bf16 mask_out")
    if "T" in outs:
        hi, lo = gx.split(o["v"])
        G["T_hi"].check(hi.transpose(1, 2), f"{tag}: transposed hi plane (batch, column, row)")
        G["T_lo"].check(lo.transpose(1, 2), f"{tag}: transposed lo plane (batch, column, row)")
    if "torgb" in outs:
        G["part"].check(o["part"].float().reshape(1, nblk * batch * M, 4), f"{tag}: ToRGB partials (row = block * rows + row)")
        lib = _lib.load()
        tau = e["tau"].float().contiguous()
        for accumulate, want in ((0, o["rgb_new"]), (1, o["rgb_acc"])):
            rgb = gx.Guarded(1, batch * M, 3, 3, 0, torch.float32, d)
            if accumulate:
                rgb.view()[:] = e["rgb0"].float()
            assert lib.cips_torgb_finish(ctypes.c_void_p(G["part"].data().data_ptr()), nblk, ctypes.c_void_p(tau.data_ptr()),
                                         ctypes.c_void_p(rgb.data().data_ptr()), batch * M, accumulate, _stream()) == 0
            torch.cuda.synchronize()
            rgb.check(want.float().view(1, batch * M, 3), f"{tag}: cips_torgb_finish accumulate={accumulate}")


# ----------------------------------------------------------------------------------------------------------------------
# K-major
# ----------------------------------------------------------------------------------------------------------------------
def _km_desc(ops, A, B, M, N, K, batch, C, kernel, strideA=None, strideB=None):
    from cips3d_amd._lib import GemmX3Desc
    dsc = ops._x3_operands(GemmX3Desc(), ops.Planes(A.hi.data(), A.lo.data()), ops.Planes(B.hi.data(), B.lo.data()), M, N, K,
                           A.ld, B.ld, batch, A.stride if strideA is None else strideA, B.stride if strideB is None else strideB,
                           C.data())
    dsc.ldc, dsc.strideC, dsc.kernel = C.ld, C.stride, kernel
    return dsc


def _km_out(M, N, batch):
    ldc = N + 8
    return gx.Guarded(batch, M, N, ldc, M * ldc + 8, torch.float32, dev())


@pytest.mark.parametrize("c", KM_CASES, ids=_id)
def test_kmajor(c):
    """groups = 0: cips_gemm_*_km — kernel = 1: the 128-row form for M <= 128, else the 256-row form; kernel = 2: 256x256 tiles (a
    group of one) where M, N >= 256 — groups >= 1: cips_gemm_*_km_grouped, other operands per group"""
    from cips3d_amd import ops
    from cips3d_amd._lib import GemmX3Desc
    d = dev()
    M, N, K, batch, single, groups = c["M"], c["N"], c["K"], c["batch"], c["single"], c["groups"]
    tag = _id(c)
    if c.get("ksplit"):
        A, B = gx.x3_operands(M, N, K * batch, 1, d, kmajor=True)
        C = _km_out(M, N, batch)
        dsc = _km_desc(ops, A, B, M, N, K, batch, C, c["kernel"], strideA=K * A.ld, strideB=K * B.ld)
        assert _entry(single, "_km")(ctypes.byref(dsc), _stream()) == 0
        torch.cuda.synchronize()

        class Slices:          # batch b = contraction indices [b K, (b + 1) K)
            def __init__(self, op):
                cut = lambda t: t[0].reshape(t.shape[1], batch, K).permute(1, 0, 2)
                self.ih, self.il = cut(op.ih), cut(op.il)
        acc, mag, other = gx.accumulators(Slices(A), Slices(B), single)
        gx.assert_conditions(dict(v=acc, mag=mag), other, 1, tag)
        C.check(acc.float(), f"{tag}: partial products")
        whole, wmag, wother = gx.accumulators(A, B, single)
        gx.assert_conditions(dict(v=whole, mag=wmag), wother, 1, tag)
        gx.same(C.view().sum(0, keepdim=True), whole.float(), f"{tag}: the sum of the parts")
        return
    probs = []
    for grp in range(max(groups, 1)):
        def make(grp=grp):
            A, B = gx.x3_operands(M, N, K, batch, d, kmajor=True, b0=grp * batch)
            return (A, B) + gx.accumulators(A, B, single)
        A, B, acc, mag, other = _operands(("km", M, N, K, batch, single), make) if groups <= 1 else make()
        gx.assert_conditions(dict(v=acc, mag=mag), other, 1, tag)
        probs.append((A, B, acc, _km_out(M, N, batch)))
    if groups == 0:
        dsc = _km_desc(ops, probs[0][0], probs[0][1], M, N, K, batch, probs[0][3], c["kernel"])
        rc = _entry(single, "_km")(ctypes.byref(dsc), _stream())
    else:
        descs = (GemmX3Desc * groups)()
        for i, (A, B, _, C) in enumerate(probs):
            ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(_km_desc(ops, A, B, M, N, K, batch, C, c["kernel"])), ctypes.sizeof(GemmX3Desc))
        rc = _entry(single, "_km_grouped")(descs, groups, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (tag, rc)
    for i, (_, _, acc, C) in enumerate(probs):
        C.check(acc.float(), f"{tag}: C of group {i}")


@pytest.mark.parametrize("single", [False, True], ids=["bf16x3", "bf16"])
def test_kmajor_grouped_refusals(single):
    """a fifth group, and in the single-pass form a contraction of one 64-deep k-tile: hipErrorNotSupported, nothing written"""
    from cips3d_amd import ops
    from cips3d_amd._lib import GemmX3Desc
    d = dev()
    M = N = 256
    for K, groups in ((128, 5),) + (((64, 1), (64, 2)) if single else ()):
        probs = [gx.x3_operands(M, N, K, 1, d, kmajor=True, b0=g) + (_km_out(M, N, 1),) for g in range(groups)]
        descs = (GemmX3Desc * groups)()
        for i, (A, B, C) in enumerate(probs):
            ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(_km_desc(ops, A, B, M, N, K, 1, C, 2)), ctypes.sizeof(GemmX3Desc))
        rc = _entry(single, "_km_grouped")(descs, groups, _stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED, (K, groups, rc)
        for *_, C in probs:
            C.untouched(f"K-major grouped K={K} groups={groups}")


# ----------------------------------------------------------------------------------------------------------------------
# fp32
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", F32_CASES, ids=_id)
def test_f32(c):
    from cips3d_amd import ops
    d = dev()
    M, N, K, batch, a_k, b_n = c["M"], c["N"], c["K"], c["batch"], c["a_k"], c["b_n"]
    a, b, e, x, o, unit = gx.f32_reference(c, d)
    gx.assert_conditions(o, None, unit, _id(c))
    Ad = (a.transpose(1, 2) if a_k else a).float().contiguous()           # (K, M) rows or (M, K) rows
    Bd = (b if b_n else b.transpose(1, 2)).float().contiguous()           # (N, K) rows or (K, N) rows
    ldc = N + 12
    stride = M * ldc + 4
    g = (2 * ldc + 63) // 64 * 64
    inp = lambda v: gx.Strided(batch, M, N, ldc, stride, torch.float32, d, guard=g, values=v)
    out = lambda: gx.Guarded(batch, M, N, ldc, stride, torch.float32, d)
    keep, kw, G = [], {}, {"C": out()}
    for name in ("bias", "bias_m"):
        if name in x:
            keep.append(x[name].float().contiguous()); kw[name] = keep[-1]
    if "resid" in x:
        keep.append(inp(x["resid"])); kw["resid"] = keep[-1].data()
        G["C2"] = out(); kw["C2"] = G["C2"].data()
    if "add" in e:
        keep += [inp(e["add"]), inp(e["maskv"]), e["rgb_g"].float().contiguous(), e["rgb_w"].float().contiguous()]
        G["CU"] = out()
        kw.update(add=keep[-4].data(), mask=keep[-3].data(), rgb_g=keep[-2], rgb_w=keep[-1], C_unmasked=G["CU"].data())
    ops.gemm(Ad, Bd, G["C"].data(), M, N, K, M if a_k else K, K if b_n else N, ldc, batch=batch, strideA=M * K, strideB=K * N,
             strideC=stride, a_kmajor=a_k, b_nmajor=b_n, alpha=c["alpha"], act=x["act"], slope=0.25, act_gain=x["gain"], **kw)
    torch.cuda.synchronize()
    tag = _id(c)
    G["C"].check(o["v"].float(), f"{tag}: C")
    if "C2" in G:
        G["C2"].check(o["C2"].float(), f"{tag}: C2")
    if "CU" in G:
        G["CU"].check(o["CU"].float(), f"{tag}: C_unmasked")
