"""GPU: the single-pass ("bf16") GEMM kernels — cips_gemm_bf16 (256x256-tile and 256x128 kernels), cips_gemm_bf16_km and
cips_gemm_bf16_km_grouped — against epilogue(sum_k a_hi * b_hi) computed by torch in fp64 from the SAME hi planes, for every
epilogue flavour the INR head issues.

The tolerance is derived, not measured.  The kernels' products a_hi * b_hi are exact in fp32 (8 x 8 significant bits), so only the
fp32 accumulation differs from the fp64 sum: K roundings of at most one fp32 ulp of a partial sum that never exceeds
S = sum_k |a_hi| |b_hi|, doubled for the matrix core's own rounding of its internal partial sums:
    |err| <= 4 * K * 2^-24 * S            per element, before the epilogue
(the epilogue only scales by <= 1 or adds exactly known terms), plus 2^-17 |value| where the value is read back from hi / lo
planes.  Gate bit planes must be equal except where the fp64 pre-activation is within that bound of zero.  Every case also
shows that the pass count is what it claims: the 3-pass kernel's result on the same planes differs from the single-pass one by
more than the bound somewhere (its lo terms are a random walk of ~sqrt(2K) * 2^-10 |a||b|; the bound grows like K * S, which
is why the contraction lengths here stop at the head's 512 — at K = 4096 the worst-case bound is wider than the lo terms)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
SLOPE = 0.2


def dev():
    return torch.device("cuda:0")


def _planes(x):
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return hi, lo


def _pack_bits(b):
    w = (1 << torch.arange(8, device=b.device)).to(torch.int32)
    return (b.reshape(*b.shape[:-1], -1, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


def _unpack_bits(u, N):
    return ((u.to(torch.int32).unsqueeze(-1) >> torch.arange(8, device=u.device)) & 1).reshape(*u.shape[:-1], N).bool()


def _nan_like(t):
    return torch.full_like(t, float("nan"))


FLAVOURS = ["fwd", "fwd_res", "fwd_torgb", "fwd_res_torgb", "gate", "gate_res", "add", "add_rgb", "addp", "addp_rgb", "c32"]
# fwd*: LeakyReLU, gate bit plane out, planes (+ residual planes, + ToRGB forward: fused partials where the kernel folds it in);
# gate*: gate read from a bit plane (backward through a layer; the pinned forward; + residual: the pinned skip forward);
# add*: fp32 addend + C_unmasked + gate (+ the rank-3 ToRGB term); addp*: the addend as gated planes + their gate's bit plane;
# c32: plain fp32 C (dx0)


def _make(M, N, K, batch, flavour, seed):
    d = dev()
    g = torch.Generator(device=d).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=d, generator=g)
    a = {"A": r(batch, M, K), "B": r(batch, N, K) * 0.05}
    if "res" in flavour:
        a["res"] = r(batch, M, N)
    if "torgb" in flavour:
        a["T"], a["tau"], a["rgb0"] = r(3, N), r(3), r(batch * M, 3)
    if flavour.startswith(("gate", "add")):
        a["gate"] = r(batch, M, N) > 0
    if flavour.startswith("add"):
        a["D"] = r(batch, M, N)
        a["pg"] = r(batch, M, N) > 0
    if flavour.endswith("_rgb"):
        a["rg"], a["rw"] = r(batch * M, 3), r(3, N)
    return a


def _run(ops, single, kernel, a, M, N, K, batch, flavour, nan_lo=False):
    """-> dict of outputs (fp32 tensors on the device; "bits": bool gates)"""
    d = dev()
    Ah, Al = _planes(a["A"]); Bh, Bl = _planes(a["B"])
    if nan_lo:
        Al, Bl = _nan_like(Al), _nan_like(Bl)
    Ap, Bp = ops.Planes(Ah, Al), ops.Planes(Bh, Bl)
    sh = (M, N, K, K, K, batch, M * K, N * K)
    P = ops.Planes(_nan_like(Ah.new_empty(batch, M, N)), _nan_like(Ah.new_empty(batch, M, N)))
    out = {}
    old_k, ops.X3_KERNEL = ops.X3_KERNEL, kernel
    try:
        if flavour.startswith("fwd"):
            mb = torch.zeros(batch, M, N // 8, device=d, dtype=torch.uint8)
            res = ops.Planes(*_planes(a["res"])) if "res" in flavour else None
            if "torgb" in flavour:
                rgb = a["rgb0"].clone()
                ops.gemm_x3_torgb(Ap, Bp, *sh, P, a["T"], a["tau"], rgb, True, single=single, act=1, res=res, mask_out=mb, gate_bits=2)
                out["rgb"] = rgb
            else:
                ops.gemm_x3(Ap, Bp, *sh, single=single, P=P, act=1, res=res, mask_out=mb, gate_bits=2)
            out["bits"] = _unpack_bits(mb, N)
        elif flavour.startswith("gate"):
            res = ops.Planes(*_planes(a["res"])) if "res" in flavour else None
            ops.gemm_x3(Ap, Bp, *sh, single=single, P=P, res=res, mask=_pack_bits(a["gate"]), gate_bits=1)
        elif flavour.startswith("addp"):
            gated = a["D"] * torch.where(a["pg"], 1.0, SLOPE)
            kw = dict(mask=_pack_bits(a["gate"]), gate_bits=1, rgb_g=a.get("rg"), rgb_w=a.get("rw"))
            assert ops.gemm_x3_takes_addp(Ap, Bp, *sh, single=single, P=P, addp=(ops.Planes(*_planes(gated)), _pack_bits(a["pg"])), **kw)
            ops.gemm_x3(Ap, Bp, *sh, single=single, P=P, addp=(ops.Planes(*_planes(gated)), _pack_bits(a["pg"])), **kw)
        elif flavour.startswith("add"):
            CU = torch.full((batch, M, N), float("nan"), device=d)
            ops.gemm_x3(Ap, Bp, *sh, single=single, P=P, add=a["D"], C_unmasked=CU, mask=_pack_bits(a["gate"]), gate_bits=1,
                        rgb_g=a.get("rg"), rgb_w=a.get("rw"))
            out["CU"] = CU
        else:
            C = torch.full((batch, M, N), float("nan"), device=d)
            ops.gemm_x3(Ap, Bp, *sh, single=single, C=C)
            out["C"] = C
        torch.cuda.synchronize()
    finally:
        ops.X3_KERNEL = old_k
    if flavour != "c32":
        out["P"] = P.float()
    return out


def _reference(a, M, N, K, batch, flavour):
    """fp64 from the hi planes -> (dict of expected outputs incl. "pre": the value the LeakyReLU sees, bound per element)"""
    Ah = a["A"].bfloat16().double(); Bh = a["B"].bfloat16().double()
    acc = torch.bmm(Ah, Bh.transpose(1, 2))
    bound = 4.0 * K * 2.0 ** -24 * torch.bmm(Ah.abs(), Bh.abs().transpose(1, 2))
    f64 = lambda t: torch.stack([p.double() for p in _planes(t)]).sum(0)          # what the kernel reads from split planes
    want = {}
    if flavour.startswith("fwd"):
        want["pre"] = acc
        v = torch.where(acc > 0, acc, acc * SLOPE)
        if "res" in flavour:
            v = v + f64(a["res"])
        want["P"] = v
    elif flavour.startswith("gate"):
        v = acc * torch.where(a["gate"], 1.0, SLOPE)
        if "res" in flavour:
            v = v + f64(a["res"])
        want["P"] = v
    elif flavour.startswith("add"):
        if flavour.startswith("addp"):
            s = acc + f64(a["D"] * torch.where(a["pg"], 1.0, SLOPE)) * torch.where(a["pg"], 1.0, float(torch.tensor(1.0 / SLOPE, dtype=torch.float32)))
        else:
            s = acc + a["D"].double()
            want["CU"] = s
        if flavour.endswith("_rgb"):
            s = s + (a["rg"].double() @ a["rw"].double()).view(batch, M, N)
            if "CU" in want:
                want["CU"] = s
        want["P"] = s * torch.where(a["gate"], 1.0, SLOPE)
    else:
        want["C"] = acc
    return want, bound


def _check(tag, got, want, bound, a, flavour):
    """every output within the derived bound of the fp64 value; -> the single-pass planes / C (for the cross checks)"""
    worst = {}
    for key in ("C", "CU", "P"):
        if key in want:
            # P: read back from hi / lo planes; CU: the epilogue adds an fp32 addend (and the rank-3 term) to the accumulator and
            # stores the fp32 sum — up to four more roundings of at most 2^-24 |value| each; C: the accumulator itself, no extra term
            extra = {"P": 2.0 ** -17, "CU": 2.0 ** -22, "C": 0.0}[key]
            tol = bound + extra * want[key].abs()
            err = (got[key].double() - want[key]).abs()
            assert torch.isfinite(got[key]).all(), (tag, key)
            worst[key] = float((err / tol).max())
    if "bits" in got:
        wrong = got["bits"] != (want["pre"] > 0)
        worst["gate bits off where |pre| > bound"] = int((wrong & (want["pre"].abs() > bound)).sum())
        worst["gate bits off"] = int(wrong.sum())
    print(f"{tag}: largest |err| / bound per output {worst}")
    for key in ("C", "CU", "P"):
        assert worst.get(key, 0.0) <= 1.0, (tag, key, worst)
    assert worst.get("gate bits off where |pre| > bound", 0) == 0, (tag, worst)
    if "rgb" in got:
        # ToRGB forward of the values the GEMM wrote (its own fp32 sums over N terms: the existing fused-ToRGB bar)
        wr = got["P"].double().view(-1, got["P"].shape[-1]) @ a["T"].double().t() + a["tau"].double() + a["rgb0"].double()
        e = float((got["rgb"].double() - wr).norm() / wr.norm())
        print(f"{tag}: ToRGB of the written planes rel err {e:.3e}")
        assert e < 2e-5, (tag, e)


def _main_output(o):
    return o["P"] if "P" in o else o["C"]


HEAD_SHAPES = [(4096, 512, 512, 1), (4096, 512, 512, 4), (4096, 512, 512, 32), (16384, 512, 512, 4),      # the head's layers
               (4096, 512, 32, 4), (16384, 512, 32, 1),                                                  # ... its first layer (K = 32)
               (64, 512, 512, 2), (160, 512, 512, 2), (256, 512, 512, 2)]                                # the fixtures' images


def _tiled_ok(M, N, K, flavour):
    return M % 256 == 0 and N % 256 == 0 and K % 128 == 0 and flavour != "gate_res"


@pytest.mark.parametrize("flavour", FLAVOURS)
@pytest.mark.parametrize("M,N,K,batch", HEAD_SHAPES)
def test_single_pass_nt_gemm_is_the_hi_plane_product(M, N, K, batch, flavour):
    from cips3d_amd import ops
    if flavour == "c32":
        N, K = (32, 512) if K == 512 else (K, K)          # dx0 = g1 . Wb1^T: 512 -> 32 features
    if flavour.startswith("addp") and not _tiled_ok(M, N, K, flavour):
        # only the 256 x 256-tile kernel takes the planes addend; elsewhere the head falls back to the fp32 addend ("add")
        assert not ops._addp_shape_ok(M, K, N, batch, dev(), single=True)
        return
    a = _make(M, N, K, batch, flavour, M + N + K + batch + len(flavour))
    want, bound = _reference(a, M, N, K, batch, flavour)
    tag = f"bf16 NT {M}x{N}x{K}x{batch} {flavour}"
    addp = flavour.startswith("addp")          # taken by the 256 x 256-tile kernel only: no other kernel to run or to compare with
    outs = {}
    for kernel, name in ((1, "256x128 kernel"), (0, "automatic"), (2, "256x256 kernel")):
        if (kernel == 2 and not _tiled_ok(M, N, K, flavour)) or (addp and kernel != 2):
            continue
        outs[kernel] = _run(ops, True, kernel, a, M, N, K, batch, flavour)
        _check(f"{tag} [{name}]", outs[kernel], want, bound, a, flavour)
    tol = bound + 2.0 ** -17 * _main_output(want).abs()
    if 1 in outs and 2 in outs:
        # the two kernels agree with each other to the same bound (numerics do not depend on which kernel takes a shape)
        r = float(((_main_output(outs[2]).double() - _main_output(outs[1]).double()).abs() / tol).max())
        print(f"{tag}: 256x256 vs 256x128 kernel, largest |difference| / bound {r:.4f}")
        assert r <= 1.0
    # the pass count: the 3-pass result on the same planes is further away than the bound allows
    x3 = _run(ops, False, 2 if addp else 0, a, M, N, K, batch, flavour)
    for kernel, o in outs.items():
        r = float(((_main_output(o).double() - _main_output(x3).double()).abs() / tol).max())
        print(f"{tag} kernel={kernel}: largest |single pass - 3 passes| / bound {r:.2f}")
        assert r > 1.0, (tag, kernel, r)


@pytest.mark.parametrize("kernel", [1, 2])
def test_lo_planes_are_never_read(kernel):
    """operand lo planes filled with NaN bit patterns: the results are the ones computed with the real lo planes, bit for bit"""
    from cips3d_amd import ops
    M, N, K, batch = 4096, 512, 512, 4
    for flavour in ("fwd_res_torgb", "addp_rgb" if kernel == 2 else "add_rgb"):
        a = _make(M, N, K, batch, flavour, 11)
        clean = _run(ops, True, kernel, a, M, N, K, batch, flavour)
        nan = _run(ops, True, kernel, a, M, N, K, batch, flavour, nan_lo=True)
        for k in clean:
            assert torch.isfinite(nan[k].float()).all(), (flavour, k)
            assert torch.equal(clean[k], nan[k]), (flavour, k)
        want, bound = _reference(a, M, N, K, batch, flavour)
        _check(f"bf16 NT NaN lo planes kernel={kernel} {flavour}", nan, want, bound, a, flavour)
    # K-major, single problem and grouped launch: the clean-lo result bit for bit, and the fp64 reference
    for grouped in (False, True):
        clean, refs = _km_case(ops, 512, 512, K, batch, kernel, True, grouped, 3)
        nan, _ = _km_case(ops, 512, 512, K, batch, kernel, True, grouped, 3, nan_lo=True)
        for Cc, Cn, (want, bound) in zip(clean, nan, refs):
            assert torch.isfinite(Cn).all() and torch.equal(Cc, Cn), grouped
            assert float(((Cn.double() - want).abs() / bound).max()) <= 1.0, grouped


def _km_case(ops, M, N, K, batch, kernel, single, grouped, seed, nan_lo=False):
    d = dev()
    g = torch.Generator(device=d).manual_seed(seed)
    probs, refs = [], []
    for _ in range(2 if grouped else 1):
        A = torch.randn(batch, K, M, device=d, generator=g); B = torch.randn(batch, K, N, device=d, generator=g)
        C = torch.full((batch, M, N), float("nan"), device=d)
        (Ah, Al), (Bh, Bl) = _planes(A), _planes(B)
        if nan_lo:
            Al, Bl = _nan_like(Al), _nan_like(Bl)
        probs.append((ops.Planes(Ah, Al), ops.Planes(Bh, Bl), C))
        Ah, Bh = A.bfloat16().double(), B.bfloat16().double()
        refs.append((torch.bmm(Ah.transpose(1, 2), Bh), 4.0 * K * 2.0 ** -24 * torch.bmm(Ah.abs().transpose(1, 2), Bh.abs())))
    old_k, ops.X3_KERNEL = ops.X3_KERNEL, kernel
    try:
        if grouped:
            ops.gemm_x3_km_grouped(probs, M, N, K, M, N, batch, K * M, K * N, single=single)
        else:
            ops.gemm_x3_km(*probs[0][:2], M, N, K, M, N, batch, K * M, K * N, probs[0][2], single=single)
        torch.cuda.synchronize()
    finally:
        ops.X3_KERNEL = old_k
    return [p[2] for p in probs], refs


# the head's weight gradients dWb = X^T G: 512 x 512 outputs (32 x 512 for the first layer), contraction over the pixels of one part of
# an image (512 at up to 4 images of 64^2 pixels); 160 / 64 / 256: the fixtures' images (K not a whole number of 64-deep k-tiles
# -> the 256x128 kernel; M = 32 -> the 128-row kernel)
KM_SHAPES = [(512, 512, 512, 32, True), (512, 512, 512, 8, True), (512, 512, 512, 32, False), (512, 512, 256, 4, False), (32, 512, 512, 32, False),
             (512, 512, 160, 2, True), (512, 512, 64, 2, True), (32, 512, 160, 2, False), (256, 256, 128, 3, False)]


@pytest.mark.parametrize("M,N,K,batch,grouped", KM_SHAPES)
def test_single_pass_kmajor_gemm_is_the_hi_plane_product(M, N, K, batch, grouped):
    from cips3d_amd import ops
    tag = f"bf16 K-major {M}x{N}x{K}x{batch}{' grouped' if grouped else ''}"
    outs = {}
    for kernel in (1, 2, 0):
        Cs, refs = _km_case(ops, M, N, K, batch, kernel, True, grouped, M + N + K + batch)
        for C, (want, bound) in zip(Cs, refs):
            assert torch.isfinite(C).all(), tag
            r = float(((C.double() - want).abs() / bound).max())
            print(f"{tag} kernel={kernel}: largest |err| / bound {r:.3f}")
            assert r <= 1.0, (tag, kernel, r)
        outs[kernel] = Cs
    for Ca, Cb, (want, bound) in zip(outs[1], outs[2], refs):         # 256x128 / 128x128 kernel against the 256x256-tile one
        assert float(((Ca.double() - Cb.double()).abs() / bound).max()) <= 1.0, tag
    C3, _ = _km_case(ops, M, N, K, batch, 0, False, grouped, M + N + K + batch)
    for kernel in (1, 2, 0):
        for C, Cx, (want, bound) in zip(outs[kernel], C3, refs):
            r = float(((C.double() - Cx.double()).abs() / bound).max())
            print(f"{tag} kernel={kernel}: largest |single pass - 3 passes| / bound {r:.2f}")
            assert r > 1.0, (tag, kernel, r)
