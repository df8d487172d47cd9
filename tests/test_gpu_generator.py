"""GPU: the drop-in generator (HIP path through the C-ABI) against the golden vectors minted
from the reference and against the CPU oracle, forward and backward."""
import math

import pytest
import torch

from conftest import (load_golden, load_gates, seeded_generator, check_checksums, max_rel, rel_err, G_CFG, pack_bitplane,
                      unpack_bitplane)
from oracle import cips3d_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-3
GRAD_TOL = 2e-4    # parameter gradients for fixed gates: measured <= 7.3e-5 (bf16x3), <= 1.7e-5 (f32) on MI355X; the bar is 1e-3
CASES = ["g_r16_hier", "g_r8_flat_noise", "g_r8_hier_noise", "g_r8_freeze", "g_r16_part",
         "g_r16_part_odd"]   # _part: part_grad_forward (96 of 256 pixels; _odd: 100, not a multiple of the 32-pixel GEMM granule)


@pytest.fixture(params=["f32", "bf16x3", "f32_all"])
def inr_mode(request):
    """Run under the numeric modes: exact fp32 MFMA for the head GEMMs and the SIREN forward ("f32"; the SIREN backward stays
    the fused split-bf16 kernel), the 3-pass split-operand MFMA path (default), and — round 6 — "f32_all": additionally the SIREN
    backward as the fp32 data pass with fp32-staged activations and fp32-MFMA weight-gradient GEMMs (CIPS_SIREN_BWD=staged_f32):
    no split operand anywhere in the generator."""
    from cips3d_amd import ops
    old = (ops.INR_MODE, ops.SIREN_FWD_MODE, ops.SIREN_BWD_MODE)
    ops.INR_MODE = "bf16x3" if request.param == "bf16x3" else "f32"
    ops.SIREN_FWD_MODE = "x3" if request.param == "bf16x3" else "f32"
    ops.SIREN_BWD_MODE = "staged_f32" if request.param == "f32_all" else "x3"
    yield request.param
    ops.INR_MODE, ops.SIREN_FWD_MODE, ops.SIREN_BWD_MODE = old


def _oracle64(fix, gates, keep_preact=False):
    """fp64 evaluation of the (reference-pinned) oracle with the given LeakyReLU gates pinned -> ({name: grad}, tape).
    With the gates fixed the gradient is a smooth function of the inputs, so this is a yardstick without any
    conditioning caveat (tests/test_oracle_golden.py: it agrees with the reference's own fp32 gradients to < 1e-5
    when given the reference's gates)."""
    G64 = seeded_generator(fix["seed"], freeze=fix["freeze"]).double()
    kw = fix["G_kwargs"]
    dbl = lambda dd: {k: (v.double() if torch.is_floating_point(v) else v) for k, v in dd.items()}
    tape = orc.GateTape(pin=gates)
    tape.keep_preact = keep_preact
    torch.set_default_dtype(torch.float64)
    try:
        with orc.gate_tape(tape):
            o64 = orc.generator_forward(dict(G64.named_parameters()), dbl(fix["zs"]), dbl(fix["rand"]), fix["img_size"],
                                        kw["fov"], kw["ray_start"], kw["ray_end"], kw["num_steps"], kw["h_stddev"],
                                        kw["v_stddev"], kw["hierarchical_sample"], nerf_noise=fix["nerf_noise"],
                                        return_aux_img=fix["aux"], freeze_nerf=fix["freeze"],
                                        grad_points=fix.get("grad_points"))
    finally:
        torch.set_default_dtype(torch.float32)
    tape.done()
    (o64["imgs"] * fix["G0"].double()).sum().backward()
    return {n: p.grad for n, p in G64.named_parameters()}, tape


_REF64 = {}


def _run_product(G, fix, d, pin=None, rec=None):
    from cips3d_amd import ops
    zs = {k: v.to(d) for k, v in fix["zs"].items()}
    rand = {k: v.to(d) for k, v in fix["rand"].items()}
    for p in G.parameters():
        p.grad = None
    with ops.gate_debug(pin=pin, rec=rec):
        imgs, pitch_yaw = G(zs, img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"],
                            grad_points=fix.get("grad_points"), forward_points=None, rand_override=rand, **fix["G_kwargs"])
    (imgs * fix["G0"].to(d)).sum().backward()
    torch.cuda.synchronize()
    return imgs.detach(), pitch_yaw.detach(), {n: (None if p.grad is None else p.grad.detach().cpu().double())
                                                for n, p in G.named_parameters()}


def _grad_errors(fix, grads, g64):
    """-> rows (name, err vs the fp64 yardstick over the whole tensor, err vs the reference's fp32 digest sample)"""
    rows = []
    for name, g in grads.items():
        dg = fix["grads"][name]
        if dg is None:
            assert g is None or float(g.abs().max()) == 0.0, name
            continue
        assert g is not None, name
        g = g.reshape(-1)
        t64 = g64[name].reshape(-1)
        e64 = float((g - t64).norm() / t64.norm().clamp_min(1e-300))
        ref32 = dg["sample"].double()
        eref = float((g[::dg["stride"]] - ref32).norm() / ref32.norm().clamp_min(1e-300))
        enorm = abs(float(g.norm()) - dg["norm"]) / max(dg["norm"], 1e-300)
        rows.append((name, e64, max(eref, enorm)))
    return rows


def test_grad_points_ignores_forward_points_like_the_reference():
    """generator.py:1325-1347: with grad_points < img_size**2 the reference takes part_grad_forward and never looks at
    forward_points.  Same call with and without it -> the same images and gradients, bit for bit."""
    fix = load_golden("g_r16_part")
    d = torch.device("cuda:0")
    G = seeded_generator(fix["seed"], freeze=fix["freeze"], device=d)
    zs = {k: v.to(d) for k, v in fix["zs"].items()}
    rand = {k: v.to(d) for k, v in fix["rand"].items()}
    out = []
    for fp in (None, 50):
        for p in G.parameters():
            p.grad = None
        imgs, _ = G(zs, img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"],
                    grad_points=fix["grad_points"], forward_points=fp, rand_override=rand, **fix["G_kwargs"])
        (imgs * fix["G0"].to(d)).sum().backward()
        out.append((imgs.detach().clone(), {n: p.grad.clone() for n, p in G.named_parameters() if p.grad is not None}))
    assert torch.equal(out[0][0], out[1][0])
    assert out[0][1].keys() == out[1][1].keys() and all(torch.equal(out[0][1][k], out[1][1][k]) for k in out[0][1])
    assert max_rel(out[0][0].cpu(), fix["imgs"]) < TOL


@pytest.mark.parametrize("tag", CASES)
def test_generator_matches_reference_golden(tag, inr_mode):
    """Images within 1e-3 of the reference; parameter gradients within 1e-3 of the reference for the SAME LeakyReLU
    gates, in both numeric modes, with no gate allowance:
      (A) head gates pinned to the reference's (tests/golden/gates_*.pt): every parameter gradient matches the
          reference's fp32 gradient digest and the fp64 oracle (same gates) — this holds everything upstream of the
          head (SIREN, composite, mapping networks, part-grad bookkeeping) to the bar as well;
      (B) free-running (the product decides its own gates): the gates it chose differ from the reference's only at
          pre-activations that are ambiguous at the mode's arithmetic precision (count and |pre-activation| bounded),
          and its gradients match the fp64 oracle evaluated AT THE PRODUCT'S gates."""
    fix = load_golden(tag)
    ref_gates = load_gates(tag)
    d = torch.device("cuda:0")
    G = seeded_generator(fix["seed"], freeze=fix["freeze"], device=d)
    check_checksums({k: v.cpu() for k, v in G.state_dict().items()}, fix["state_checksums"])
    if tag not in _REF64:
        _REF64[tag] = _oracle64(fix, ref_gates, keep_preact=True)
    g64_ref, tape_ref = _REF64[tag]
    total = sum(g.numel() for g in ref_gates)

    # ---- (A) pinned to the reference's gates ----
    imgs, pitch_yaw, grads = _run_product(G, fix, d, pin=[pack_bitplane(g) for g in ref_gates])
    assert imgs.shape == fix["imgs"].shape
    e = max_rel(imgs, fix["imgs"])
    assert e < TOL and max_rel(pitch_yaw, fix["pitch_yaw"]) < 1e-5
    rows_a = _grad_errors(fix, grads, g64_ref)
    wa = max(rows_a, key=lambda r: max(r[1], r[2]))
    print(f"{tag} [{inr_mode}] pinned: imgs max_rel {e:.3e}; worst gradient error {wa[1]:.3e} vs fp64 oracle, "
          f"{wa[2]:.3e} vs the reference's fp32 digest, at {wa[0]} ({len(rows_a)} parameters)")
    bad = [r for r in rows_a if max(r[1], r[2]) > GRAD_TOL]
    assert not bad, bad
    if inr_mode == "f32_all":
        # no split operand anywhere: every gradient in the fp32 class against the fp64 oracle (2e-5)
        assert wa[1] <= 2e-5, wa

    # ---- (B) free-running ----
    rec = []
    imgs, pitch_yaw, grads = _run_product(G, fix, d, rec=rec)
    e = max_rel(imgs, fix["imgs"])
    print(f"{tag} [{inr_mode}] free: imgs max_rel vs reference {e:.3e}")
    assert e < TOL and max_rel(pitch_yaw, fix["pitch_yaw"]) < 1e-5
    own = [unpack_bitplane(p.cpu()) for p in rec]
    assert [tuple(g.shape) for g in own] == [tuple(g.shape) for g in ref_gates]
    # gates that differ from the reference's: few, and only where the fp64 pre-activation is within the mode's
    # arithmetic error of zero (relative to the layer's rms pre-activation)
    amb = 2e-4 if inr_mode == "bf16x3" else 2e-5
    flips, worst_amb = 0, 0.0
    for a, b, y in zip(own, ref_gates, tape_ref.preact):
        diff = a != b
        k = int(diff.sum())
        if k:
            flips += k
            worst_amb = max(worst_amb, float(y[diff].max() / y.pow(2).mean().sqrt()))
    print(f"{tag} [{inr_mode}] free: {flips} of {total} gates differ from the reference's; largest |pre-activation| / rms "
          f"among them {worst_amb:.2e}")
    assert worst_amb < amb and flips <= 4 + total * (1e-4 if inr_mode == "bf16x3" else 1e-5)
    g64_own, _ = _oracle64(fix, own) if flips else (g64_ref, None)
    rows_b = _grad_errors(fix, grads, g64_own)
    wb = max(rows_b, key=lambda r: r[1])
    print(f"{tag} [{inr_mode}] free: worst gradient error vs the fp64 oracle at the product's gates {wb[1]:.3e} at {wb[0]}")
    bad = [r for r in rows_b if r[1] > GRAD_TOL]
    import os
    os.makedirs("gpurun_out", exist_ok=True)
    with open(f"gpurun_out/gradtable_{tag}_{inr_mode}.txt", "w") as fh:
        fh.write(f"# {flips} of {total} gates differ from the reference's (largest |preact|/rms {worst_amb:.2e})\n")
        fh.write("name  pinned:err_vs_fp64  pinned:err_vs_ref32_digest  free:err_vs_fp64_at_own_gates  free:err_vs_ref32_digest\n")
        for ra, rb in zip(rows_a, rows_b):
            fh.write(f"{ra[0]} {ra[1]:.3e} {ra[2]:.3e} {rb[1]:.3e} {rb[2]:.3e}\n")
    assert not bad, bad


@pytest.mark.parametrize("tag", ["g_r8_flat_noise", "g_r16_hier", "g_r8_hier_noise"])
def test_fused_and_unfused_march_agree_on_the_flat_golden_case(tag, monkeypatch):
    """By default the ray set-up lives inside the SIREN kernels: hierarchical_sample=False runs the fused ray-march
    (ops.RayMarchFunction: rays + SIREN + composite in one kernel), hierarchical_sample=True regenerates the coarse and
    the fine points in-kernel (ops.SirenRaysFunction, resampler with in-kernel ray directions).  CIPS_MARCH_FUSED=0
    keeps the materialised path (rays kernel, (b,n,S,3) point tensors).  Both against the reference's images, and
    against each other, forward and parameter gradients."""
    from cips3d_amd import ops
    fix = load_golden(tag)
    d = torch.device("cuda:0")
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(ops, "MARCH_FUSED", fused)
        G = seeded_generator(fix["seed"], device=d)
        imgs, _, grads = _run_product(G, fix, d, pin=[pack_bitplane(g) for g in load_gates(tag)])
        assert max_rel(imgs, fix["imgs"]) < TOL
        res[fused] = (imgs, grads)
    e = max_rel(res[True][0], res[False][0])
    worst = max(float((a - b).norm() / b.norm().clamp_min(1e-300)) for a, b in
                ((res[True][1][k], res[False][1][k]) for k in res[True][1] if res[True][1][k] is not None))
    print(f"{tag}: in-kernel rays vs materialised points: imgs {e:.2e}, worst parameter gradient {worst:.2e}")
    assert e < 1e-5 and worst < GRAD_TOL


def test_generator_rng_draw_order_matches_reference_shapes():
    """Same-device seed parity contract: the wrapper must issue the reference's draws in order."""
    d = torch.device("cuda:0")
    G = seeded_generator(0, device=d)
    calls = []
    o_rand, o_randn = torch.rand, torch.randn

    def rand(*a, **k):
        calls.append(("rand", tuple(a[0]) if isinstance(a[0], (tuple, list, torch.Size)) else a)); return o_rand(*a, **k)

    def randn(*a, **k):
        calls.append(("randn", tuple(a[0]) if isinstance(a[0], (tuple, list, torch.Size)) else a)); return o_randn(*a, **k)

    torch.rand, torch.randn = rand, randn
    try:
        zs = G.get_zs(2)
        with torch.no_grad():
            G(zs, img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=4, h_stddev=0.3, v_stddev=0.155,
              hierarchical_sample=True, sample_dist="gaussian", nerf_noise=0.)
    finally:
        torch.rand, torch.randn = o_rand, o_randn
    assert calls == [("randn", (2, 256)), ("randn", (2, 512)), ("rand", (2, 64, 4, 1)), ("randn", (2, 1)),
                     ("randn", (2, 1)), ("randn", (2, 64, 4, 1)), ("rand", (128, 4)), ("randn", (2, 64, 8, 1))]


def test_generator_r64_vs_oracle_forward(inr_mode):
    """Headline geometry (64^2, S=24 flat and S=12 hierarchical) at b=1 against the CPU oracle."""
    d = torch.device("cuda:0")
    for S, hier in [(24, False), (12, True)]:
        G = seeded_generator(1234)
        g = torch.Generator().manual_seed(77)
        b, n = 1, 64 * 64
        E = 2 * S if hier else S
        zs = {"z_nerf": torch.randn(b, 256, generator=g), "z_inr": torch.randn(b, 512, generator=g)}
        rand = dict(jitter=torch.rand(b, n, S, 1, generator=g), theta=torch.randn(b, 1, generator=g),
                    phi=torch.randn(b, 1, generator=g), noise_c=torch.randn(b, n, S, 1, generator=g),
                    u=torch.rand(b * n, S, generator=g), noise_f=torch.randn(b, n, E, 1, generator=g))
        with torch.no_grad():
            ref = orc.generator_forward(dict(G.named_parameters()), zs, rand, 64, 12, 0.88, 1.12, S, 0.3, 0.155, hier)
        Gd = G.to(d)
        with torch.no_grad():
            imgs, py = Gd({k: v.to(d) for k, v in zs.items()}, img_size=64, fov=12, ray_start=0.88, ray_end=1.12,
                          num_steps=S, h_stddev=0.3, v_stddev=0.155, hierarchical_sample=hier, sample_dist="gaussian",
                          rand_override={k: v.to(d) for k, v in rand.items()})
        e = max_rel(imgs, ref["imgs"])
        print(f"r64 S={S} hier={hier} [{inr_mode}]: imgs max_rel {e:.3e}")
        assert e < TOL


@pytest.mark.parametrize("S,hier", [(24, False), (12, True)])
def test_generator_full_size_properties(S, hier):
    """BASELINE configuration C2 at its full size (64^2, 24 SIREN evaluations per ray, 32 images, default numeric
    mode), through properties that need no oracle run:
      * determinism: the same inputs give bit-identical images and parameter gradients (no atomics anywhere),
      * batch-sharding invariance (what the data-parallel path of SURVEY.md §8e relies on): images 8..15 rendered on
        their own equal rows 8..15 of the batch and the four quarter-batch gradients sum to the batch gradient — to
        fp32 summation-order noise, not bitwise: another batch size selects other GEMM tilings (hipBLASLt in the
        mapping MLPs); for the gradients that noise is amplified by LeakyReLU gate flips, see the comment at the
        assertion,
      * linearity of the backward in the upstream gradient: doubling it doubles every parameter gradient exactly
        (a power of two commutes with fp32 rounding and with the hi/lo bf16 split)."""
    d = torch.device("cuda:0")
    G = seeded_generator(1234, device=d)
    g = torch.Generator().manual_seed(5)
    b, n = 32, 64 * 64
    E = 2 * S if hier else S
    zs = {"z_nerf": torch.randn(b, 256, generator=g).to(d), "z_inr": torch.randn(b, 512, generator=g).to(d)}
    rand = dict(jitter=torch.rand(b, n, S, 1, generator=g), theta=torch.randn(b, 1, generator=g),
                phi=torch.randn(b, 1, generator=g), noise_c=torch.randn(b, n, S, 1, generator=g),
                u=torch.rand(b * n, S, generator=g), noise_f=torch.randn(b, n, E, 1, generator=g))
    rand = {k: v.to(d) for k, v in rand.items()}
    G0 = (torch.randn(b, 3, 64, 64, generator=g) / (b * 3 * 64 * 64)).to(d)
    params = [p for p in G.parameters()]

    from cips3d_amd import ops

    def run(sl, scale=1.0, pin=None, rec=None):
        rs = {k: (v[sl] if k != "u" else v.view(b, n, S)[sl].reshape(-1, S)) for k, v in rand.items()}
        for p in params:
            p.grad = None
        with ops.gate_debug(pin=pin, rec=rec):
            imgs, _ = G({k: v[sl] for k, v in zs.items()}, img_size=64, fov=12, ray_start=0.88, ray_end=1.12, num_steps=S,
                        h_stddev=0.3, v_stddev=0.155, hierarchical_sample=hier, sample_dist="gaussian", rand_override=rs)
        imgs.backward(G0[sl] * scale)
        return imgs.detach().clone(), [None if p.grad is None else p.grad.clone() for p in params]

    full = slice(0, b)
    gates = []
    im1, g1 = run(full, rec=gates)
    im2, g2 = run(full)
    assert torch.isfinite(im1).all() and im1.abs().max() <= 1.0
    assert torch.equal(im1, im2), "forward is not deterministic"
    for a_, b_ in zip(g1, g2):
        assert (a_ is None) == (b_ is None)
        if a_ is not None:
            assert torch.equal(a_, b_), "backward is not deterministic"
    _, g3 = run(full, scale=2.0)
    for a_, c_ in zip(g1, g3):
        if a_ is not None:
            assert torch.equal(a_ * 2, c_), "backward is not linear in the upstream gradient"
    acc = [None if x is None else torch.zeros_like(x, dtype=torch.float64) for x in g1]
    for q in range(4):
        sl = slice(8 * q, 8 * q + 8)
        # the quarter batch takes the LeakyReLU gates the full batch took: its mapping MLPs run on other hipBLASLt
        # kernels (8 rows instead of 32), which moves the styles by ~1e-7 and would flip a few of the 6.7e7 gates per
        # layer — a discontinuity of the function, not a sharding error
        imq, gq = run(sl, pin=[p[sl] for p in gates])
        e = max_rel(imq, im1[sl])
        assert e < 2e-5, f"images {8 * q}..{8 * q + 7} depend on the rest of the batch ({e:.2e})"
        for a_, x in zip(acc, gq):
            if a_ is not None:
                a_ += x.double()
    worst, rows = 0.0, []
    names = [k for k, _ in G.named_parameters()]
    for nm, a_, x in zip(names, acc, g1):
        if a_ is not None:
            e = rel_err(a_.float(), x)
            rows.append((e, nm))
            worst = max(worst, e)
    # With the gates fixed the gradient is smooth: what is left is fp32 summation order (mapping MLPs on another
    # hipBLASLt kernel, partial sums over 8 instead of 32 images).  A dropped image, chunk or partial sum would show up
    # at >= 0.15.
    print(f"   worst parameters: {sorted(rows, reverse=True)[:3]}")
    print(f"C2 full size S={S} hier={hier}: sum of quarter-batch gradients vs batch gradient (same gates), worst rel err {worst:.2e}")
    assert worst < 1e-3


@pytest.mark.parametrize("tag", ["g_r8_eval_psi_staged", "g_r8_eval_camera", "g_r8_eval_camera_staged"])
def test_generator_eval_paths_match_reference_golden(tag, inr_mode):
    """Inference path against vectors minted from the reference: psi truncation through
    generate_avg_frequencies, the staged forward (forward_points, ragged last chunk) with its per-image / per-chunk draw
    order, last_back / white_back / softplus, forward_camera_pos_and_lookup (one-shot: up_vector dropped like the
    reference does; staged: honoured)."""
    from test_oracle_golden import eval_avg_styles
    fix = load_golden(tag)
    d = torch.device("cuda:0")
    G = seeded_generator(fix["seed"], device=d)
    check_checksums(G.state_dict(), fix["state_checksums"])
    kw = dict(fix["G_kwargs"])
    zs = {k: v.to(d) for k, v in fix["zs"].items()}
    rand = {k: v.to(d) for k, v in fix["rand"].items()}
    az = eval_avg_styles(fix, seeded_generator(fix["seed"]))
    if az is not None:                      # the 10 000 averaging latents the reference drew (regenerated on the CPU)
        real_get_zs = G.get_zs
        G.get_zs = lambda n, **k: {k_: v.to(d) for k_, v in az.items()} if n == 10000 else real_get_zs(n, **k)
    common = dict(img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"], grad_points=None,
                  forward_points=fix["forward_points"], rand_override=rand)
    with torch.no_grad():
        if fix["camera"] is not None:
            cam = {k: v.to(d) for k, v in fix["camera"].items()}
            imgs, py = G.forward_camera_pos_and_lookup(zs, **common, **kw, **cam)
        else:
            imgs, py = G(zs, **common, **kw)
    if az is not None:
        ref = fix["avg"]["styles"]
        for k, v in G.avg_styles.items():
            assert max_rel(v, ref[k]) < 1e-4, k
    e = max_rel(imgs, fix["imgs"])
    print(f"{tag} [{inr_mode}]: imgs max_rel {e:.3e}")
    assert imgs.shape == fix["imgs"].shape and e < TOL
    assert max_rel(py, fix["pitch_yaw"]) < 1e-5 or float(fix["pitch_yaw"].abs().max()) == 0.0
    assert torch.equal(py.cpu() == 0, fix["pitch_yaw"] == 0)


def test_generator_camera_distributions_run():
    """Every camera distribution of comm_utils.sample_camera_positions goes through the HIP path (one-shot and staged);
    the default sample_dist=None is the reference's `assert 0`."""
    d = torch.device("cuda:0")
    G = seeded_generator(2, device=d)
    kw = dict(img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=4, h_stddev=0.3, v_stddev=0.155,
              hierarchical_sample=True, nerf_noise=0.)
    zs = G.get_zs(2)
    with torch.no_grad():
        for mode in ["uniform", "normal", "hybrid", "truncated_gaussian", "spherical_uniform", "mean"]:
            for fp in (None, 40):
                imgs, py = G(zs, sample_dist=mode, forward_points=fp, **kw)
                assert imgs.shape == (2, 3, 8, 8) and torch.isfinite(imgs).all() and py.shape == (2, 2), (mode, fp)
                if mode == "mean":
                    assert torch.allclose(py, torch.full_like(py, math.pi / 2))
        with pytest.raises(AssertionError):
            G(zs, **kw)


def test_camera_distributions_values_on_gpu_match_reference_golden(monkeypatch):
    """the non-gaussian camera modes were only checked for finiteness on the GPU.  Here every mode of
    comm_utils.sample_camera_positions runs with device = cuda:0 — all arithmetic on the GPU — on the reference's own draws:
    torch.rand / torch.randn are redirected to draw from the seeded CPU generator (as the reference did when the fixture was
    minted) and move the draw to the device.  Origin, pitch, yaw against tests/golden/camera_cases.pt."""
    import random
    from cips3d_amd.generator import sample_camera_positions
    d = torch.device("cuda:0")
    rand0, randn0 = torch.rand, torch.randn

    def on_cpu(fn):
        def f(*a, **k):
            dev = k.pop("device", None)
            t = fn(*a, **k)
            return t.to(dev) if dev is not None else t
        return f

    monkeypatch.setattr(torch, "rand", on_cpu(rand0))
    monkeypatch.setattr(torch, "randn", on_cpu(randn0))
    seen = set()
    for c in load_golden("camera_cases"):
        torch.manual_seed(c["seed"]); random.seed(c["seed"])
        o, phi, theta = sample_camera_positions(d, bs=5, r=1.3, horizontal_stddev=0.3, vertical_stddev=0.155,
                                                horizontal_mean=1.4, vertical_mean=1.7, mode=c["mode"])
        assert o.is_cuda and phi.is_cuda and theta.is_cuda
        e = max(max_rel(o, c["origin"]), max_rel(phi, c["phi"]), max_rel(theta, c["theta"]))
        assert e < 2e-6, (c["mode"], e)
        seen.add(c["mode"])
    assert {"uniform", "hybrid", "truncated_gaussian", "spherical_uniform"} <= seen, seen


@pytest.mark.parametrize("hidden_dim,hidden_layers", [(64, 3), (256, 2), (128, 1)])
def test_nerf_network_of_other_width_or_depth_runs_unfused_and_matches_the_oracle(hidden_dim, hidden_layers):
    """generator.py:151-340 builds NeRFNetwork for any hidden width / depth (its constructor default is hidden_dim 256); the fused
    SIREN kernels are specialised to the shipped 128 x 2.  Other shapes run the same arithmetic as GPU tensor operations: forward,
    parameter and style gradients against the oracle, and a whole generator step (flat and hierarchical sampling) on top of it."""
    from cips3d_amd.generator import NeRFNetwork, GeneratorNerfINR
    d = torch.device("cuda:0")
    torch.manual_seed(11)
    net = NeRFNetwork(in_dim=3, hidden_dim=hidden_dim, hidden_layers=hidden_layers, rgb_dim=32, style_dim=128)
    assert not net.fused
    g = torch.Generator().manual_seed(2)
    b, P = 2, 777
    pts = (torch.rand(b, P, 3, generator=g) - 0.5) * 0.3
    style = torch.randn(b, 128, generator=g)
    up = torch.randn(b, P, 33, generator=g)
    st_r = style.clone().requires_grad_(True)
    (orc.siren(dict(net.named_parameters()), pts, st_r, prefix="") * up).sum().backward()
    ref = {n: p.grad.clone() for n, p in net.named_parameters()}
    ref_style = st_r.grad.clone()
    with torch.no_grad():
        ref_out = orc.siren(dict(net.named_parameters()), pts, style, prefix="")
    net.zero_grad()
    nd = net.to(d)
    st = style.to(d).requires_grad_(True)
    sdict = {f"nerf_w{i}": st for i in range(hidden_layers)}
    sdict["nerf_rgb"] = st
    out = nd(pts.to(d), sdict)
    assert max_rel(out, ref_out) < 1e-4
    (out * up.to(d)).sum().backward()
    for n, p in nd.named_parameters():
        assert rel_err(p.grad, ref[n]) < 1e-4, n
    assert rel_err(st.grad, ref_style) < 1e-4
    # a generator built on it: both sampling modes run end to end through the unfused path and give finite images / gradients
    cfg = dict(G_CFG)
    cfg["nerf_cfg"] = dict(in_dim=3, hidden_dim=hidden_dim, hidden_layers=hidden_layers, rgb_dim=32, style_dim=128)
    torch.manual_seed(5)
    G = GeneratorNerfINR(**cfg, device=d).to(d); G.device = d
    assert not G.siren.fused
    kw = dict(fov=12, ray_start=0.88, ray_end=1.12, h_stddev=0.3, v_stddev=0.155, h_mean=math.pi / 2, v_mean=math.pi / 2,
              sample_dist="gaussian")
    for hier, S in ((False, 6), (True, 4)):
        imgs, _ = G(G.get_zs(2), img_size=16, num_steps=S, hierarchical_sample=hier, nerf_noise=0.1, return_aux_img=True,
                    grad_points=None, forward_points=None, **kw)
        assert imgs.shape[0] == 4 and imgs.shape[-1] == 16 and bool(torch.isfinite(imgs).all())
        imgs.square().mean().backward()
        gs = [p.grad for p in G.siren.parameters()]
        assert all(g_ is not None and bool(torch.isfinite(g_).all()) for g_ in gs) and any(float(g_.abs().max()) > 0 for g_ in gs)
        G.zero_grad()


@pytest.mark.parametrize("tag", ["g_r8_flat_noise", "g_r16_hier", "g_r8_freeze"])
def test_weight_gradient_tail_on_the_side_stream_gives_the_same_gradients(tag):
    """ops.INR_TAIL: the head's weight-gradient tail behind two gradient ports on the side stream (opened before the ray march,
    gated behind the compositing backward, co-resident kernel forms) against everything inside InrHeadX3Function on the caller's
    stream: the same images bit for bit, every parameter gradient present in both and equal up to the tail kernels' summation
    order; the ported form is the one that ran (except with a frozen NeRF, where nothing follows the head's backward), its
    ports waited for the event the compositing backward published, and no tail gate is left armed in either form."""
    from cips3d_amd import ops
    if ops.INR_MODE != "bf16x3":
        pytest.skip("the ports belong to the split-bf16 head")
    fix = load_golden(tag)
    d = torch.device("cuda:0")
    G = seeded_generator(fix["seed"], freeze=fix["freeze"], device=d)
    zs = {k: v.to(d) for k, v in fix["zs"].items()}
    rand = {k: v.to(d) for k, v in fix["rand"].items()}
    calls = []
    orig = ops.inr_head_with_ports
    ops.inr_head_with_ports = lambda *a, **k: (calls.append(a[3]), orig(*a, **k))[1]      # a[3]: the TailPorts
    out = {}
    keep = ops.INR_TAIL
    try:
        for mode in ("main", "side", "side"):
            ops.INR_TAIL = mode
            for p in G.parameters():
                p.grad = None
            n0 = len(calls)
            imgs, _ = G(zs, img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"],
                        grad_points=None, forward_points=None, rand_override=rand, **fix["G_kwargs"])
            (imgs * fix["G0"].to(d)).sum().backward()
            torch.cuda.synchronize()
            # (a frozen NeRF has no backward to run beside: the generator keeps the plain form there)
            assert (len(calls) - n0 == 1) == (mode == "side" and not fix["freeze"])
            # opened by _render ahead of its NeRF stage (_nerf_stage), the ports ran behind the compositing backward and waited for its event
            assert all(ports.waited for ports in calls[n0:])
            assert not ops._TAIL_GATE
            out.setdefault(mode, []).append((imgs.detach().clone(), {n: p.grad.clone() for n, p in G.named_parameters() if p.grad is not None}))
    finally:
        ops.INR_TAIL = keep
        ops.inr_head_with_ports = orig
    (im_m, g_m), (im_s, g_s), (im_s2, g_s2) = out["main"][0], out["side"][0], out["side"][1]
    assert torch.equal(im_m, im_s) and torch.equal(im_s, im_s2)
    assert g_m.keys() == g_s.keys() == g_s2.keys()
    for k in g_m:
        assert torch.equal(g_s[k], g_s2[k]), k                                  # the side-stream form is reproducible
        scale = float(g_m[k].abs().max()) + 1e-30
        assert float((g_m[k] - g_s[k]).abs().max()) <= 5e-6 * scale, (k, float((g_m[k] - g_s[k]).abs().max()) / scale)
