"""CPU: pin the oracle restatement (oracle/cips3d_oracle.py) against golden vectors minted from
the unmodified reference (oracle/make_golden.py).  Tolerances are tight (1e-5): both sides are
torch-CPU fp32, differences come only from op fusion order."""
import pytest
import torch

from conftest import load_golden, load_gates, seeded_generator, check_checksums, max_rel, pack_bitplane, unpack_bitplane
from oracle import cips3d_oracle as orc

CASES = ["g_r16_hier", "g_r8_flat_noise", "g_r8_hier_noise", "g_r8_freeze", "g_r16_part",
         "g_r16_part_odd"]   # _part: part_grad_forward (96 of 256 pixels; _odd: 100, not a multiple of the 32-pixel GEMM granule)


@pytest.mark.parametrize("tag", CASES)
def test_generator_oracle_matches_reference(tag):
    fix = load_golden(tag)
    G = seeded_generator(fix["seed"], freeze=fix["freeze"])
    check_checksums(G.state_dict(), fix["state_checksums"])
    sd = {k: v for k, v in G.named_parameters()}
    kw = fix["G_kwargs"]
    out = orc.generator_forward(sd, fix["zs"], fix["rand"], fix["img_size"], kw["fov"], kw["ray_start"],
                                kw["ray_end"], kw["num_steps"], kw["h_stddev"], kw["v_stddev"],
                                kw["hierarchical_sample"], nerf_noise=fix["nerf_noise"],
                                return_aux_img=fix["aux"], freeze_nerf=fix["freeze"], keep=True,
                                grad_points=fix.get("grad_points"))
    b, S, n = fix["b"], fix["S"], fix["img_size"] ** 2
    if "points" in fix:                  # whole-image cases also pin the intermediates
        assert torch.equal(out["points"], fix["points"])
        assert torch.equal(out["z"], fix["z"])
        assert max_rel(out["coarse"], fix["coarse"]) < 1e-5
        if fix["hier"]:
            assert max_rel(out["fine_z"].reshape(-1), fix["fine_z"].reshape(-1)) < 1e-6
            assert max_rel(out["fine"], fix["fine"]) < 1e-4
        assert max_rel(out["pixels_fea"], fix["pixels_fea"]) < 1e-5
        assert max_rel(out["weights"], fix["weights"]) < 1e-5
    assert max_rel(out["imgs"], fix["imgs"]) < 1e-5
    assert max_rel(out["pitch_yaw"], fix["pitch_yaw"]) < 1e-6
    (out["imgs"] * fix["G0"]).sum().backward()
    for name, p in G.named_parameters():
        d = fix["grads"][name]
        if d is None:
            assert p.grad is None, name
            continue
        g = p.grad.reshape(-1)
        got = g[::d["stride"]] if d["stride"] > 1 else g
        assert abs(float(g.double().norm()) - d["norm"]) <= 2e-4 * d["norm"] + 1e-12, name
        assert float((got - d["sample"]).norm() / d["sample"].norm().clamp_min(1e-30)) < 1e-3, name


@pytest.mark.parametrize("tag", CASES)
def test_generator_oracle_gates_match_reference_and_pin(tag):
    """The LeakyReLU gates of the reference's run (tests/golden/gates_*.pt): (1) the oracle's own fp32 run takes the
    same branch everywhere but at a handful of pre-activations within rounding of zero; (2) with the reference's
    gates pinned the oracle reproduces the reference's fp32 parameter gradients tightly (no gate allowance left);
    (3) the same in fp64 — the yardstick the GPU tests use — agrees with the reference's fp32 gradients to fp32
    rounding: with the gates fixed the gradient is a smooth function and the fp32-vs-fp64 jumps of 1e-3..1e-2 that
    the free-running comparison shows are gone."""
    fix = load_golden(tag)
    gates = load_gates(tag)
    kw = fix["G_kwargs"]

    def run(dtype, tape):
        G = seeded_generator(fix["seed"], freeze=fix["freeze"])
        cast = (lambda t: t.to(dtype) if torch.is_floating_point(t) else t)
        if dtype == torch.float64:
            G = G.double()
        torch.set_default_dtype(dtype)
        try:
            with orc.gate_tape(tape):
                out = orc.generator_forward(dict(G.named_parameters()), {k: cast(v) for k, v in fix["zs"].items()},
                                            {k: cast(v) for k, v in fix["rand"].items()}, fix["img_size"], kw["fov"],
                                            kw["ray_start"], kw["ray_end"], kw["num_steps"], kw["h_stddev"], kw["v_stddev"],
                                            kw["hierarchical_sample"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"],
                                            freeze_nerf=fix["freeze"], grad_points=fix.get("grad_points"))
        finally:
            torch.set_default_dtype(torch.float32)
        (out["imgs"] * cast(fix["G0"])).sum().backward()
        return G, out

    free = orc.GateTape()
    run(torch.float32, free)
    assert len(free.rec) == len(gates)
    total = sum(g.numel() for g in gates)
    flips = sum(int((a != b).sum()) for a, b in zip(free.rec, gates))
    print(f"{tag}: oracle fp32 vs reference fp32: {flips} of {total} gates differ")
    assert flips <= max(3, total // 200000)
    assert torch.equal(unpack_bitplane(pack_bitplane(gates[0])), gates[0])
    for dtype, tol in ((torch.float32, 1e-4), (torch.float64, 1e-4)):
        tape = orc.GateTape(pin=gates)
        G, out = run(dtype, tape)
        tape.done()
        assert max_rel(out["imgs"].float(), fix["imgs"]) < 1e-5
        worst = 0.0
        for name, p in G.named_parameters():
            d = fix["grads"][name]
            if d is None:
                assert p.grad is None, name
                continue
            g = p.grad.reshape(-1).double()
            got = g[::d["stride"]] if d["stride"] > 1 else g
            e = float((got - d["sample"].double()).norm() / d["sample"].double().norm().clamp_min(1e-300))
            worst = max(worst, e)
            assert e < tol and abs(float(g.norm()) - d["norm"]) <= tol * d["norm"], (name, e)
        print(f"{tag}: {dtype} oracle with the reference's gates pinned: worst parameter-gradient error vs the reference {worst:.2e}")


EVAL_CASES = ["g_r8_eval_psi_staged", "g_r8_eval_camera", "g_r8_eval_camera_staged"]


def eval_avg_styles(fix, G):
    """The 10 000 latents behind the reference's truncation average are not stored (30 MB): they are the two CPU draws
    that follow get_zs(b) under seed + 1.  Regenerate, check against the stored checksums, return them."""
    if fix["avg"] is None:
        return None
    torch.manual_seed(fix["seed"] + 1)
    G.get_zs(fix["b"])
    az = {"z_nerf": torch.randn(10000, 256), "z_inr": torch.randn(10000, 512)}
    for k, (s1, s2) in fix["avg"]["z_checksums"].items():
        assert abs(float(az[k].double().sum()) - s1) < 1e-6 * abs(s2) and abs(float(az[k].double().abs().sum()) - s2) < 1e-9 * s2, \
            "CPU RNG stream differs from the one the fixture was minted with"
    return az


@pytest.mark.parametrize("tag", EVAL_CASES)
def test_generator_oracle_eval_paths(tag):
    """Inference path: psi truncation + staged forward with last_back; explicit camera, softplus
    clamp, white_back and noise (one-shot: the reference drops `up_vector` there; staged, one image: it is honoured)."""
    fix = load_golden(tag)
    G = seeded_generator(fix["seed"])
    check_checksums(G.state_dict(), fix["state_checksums"])
    sd = {k: v for k, v in G.named_parameters()}
    kw = fix["G_kwargs"]
    avg = None
    az = eval_avg_styles(fix, G)
    with torch.no_grad():
        if az is not None:
            avg = (orc.mapping_nerf(sd, az["z_nerf"]).mean(0, keepdim=True), orc.mapping_inr(sd, az["z_inr"]).mean(0, keepdim=True))
            ref = fix["avg"]["styles"]
            assert max_rel(avg[0], next(v for k, v in ref.items() if k.startswith("nerf"))) < 1e-5
            assert max_rel(avg[1], next(v for k, v in ref.items() if k.startswith("inr"))) < 1e-5
        out = orc.generator_forward(sd, fix["zs"], fix["rand"], fix["img_size"], kw["fov"], kw["ray_start"], kw["ray_end"],
                                    kw["num_steps"], kw["h_stddev"], kw["v_stddev"], kw["hierarchical_sample"],
                                    nerf_noise=fix["nerf_noise"], clamp_mode=kw["clamp_mode"], return_aux_img=fix["aux"],
                                    last_back=kw["last_back"], white_back=kw["white_back"], psi=kw["psi"], avg_styles=avg,
                                    camera=fix["camera"], forward_points=fix["forward_points"])
    assert max_rel(out["imgs"], fix["imgs"]) < 1e-5
    assert max_rel(out["pitch_yaw"], fix["pitch_yaw"]) < 1e-6 or float(fix["pitch_yaw"].abs().max()) == 0.0
    assert torch.equal(out["pitch_yaw"] == 0, fix["pitch_yaw"] == 0)


def test_upfirdn2d_oracle_matches_reference_native():
    for c in load_golden("upfirdn2d_cases"):
        x = c["x"]                       # (major, h, w, minor) as the reference op sees it
        mj, h, w, mn = x.shape
        xin = x.permute(0, 3, 1, 2).reshape(1, mj * mn, h, w)
        y = orc.upfirdn2d(xin, c["k"], up=c["up"], down=c["down"], pad=c["pad"])
        y = y.reshape(mj, mn, y.shape[2], y.shape[3]).permute(0, 2, 3, 1)
        assert y.shape == c["y"].shape
        assert max_rel(y, c["y"]) < 1e-6


def test_camera_distributions_match_reference():
    """sample_camera_positions (host math of the product, comm_utils.py:451-535): every distribution of the reference,
    same draws in the same order under the same CPU seeds (torch and, for 'hybrid', Python's random)."""
    import random
    from cips3d_amd.generator import sample_camera_positions
    for c in load_golden("camera_cases"):
        torch.manual_seed(c["seed"]); random.seed(c["seed"])
        o, phi, theta = sample_camera_positions("cpu", bs=5, r=1.3, horizontal_stddev=0.3, vertical_stddev=0.155,
                                                horizontal_mean=1.4, vertical_mean=1.7, mode=c["mode"])
        assert max_rel(o, c["origin"]) < 1e-6 and max_rel(phi, c["phi"]) < 1e-6 and max_rel(theta, c["theta"]) < 1e-6, c["mode"]
    with pytest.raises(AssertionError):
        sample_camera_positions("cpu", mode=None)


def test_oracle_matches_pigan_lib_second_lineage():
    """Second, independent pin: vectors minted from the ORIGINAL pi-GAN implementations in
    piGAN_lib/generators/volumetric_rendering.py (fancy_integration with 3 colour channels, sample_pdf,
    get_initial_rays_trig + transform_sampled_points) — the oracle restates the exp/ copies of these functions and
    must reproduce the other lineage too."""
    fix = load_golden("pigan_cases")
    for c in fix["integrate"]:
        rgb, depth, w = orc.integrate(c["rgb_sigma"], c["z"], c["noise"], c["noise_std"], dim_rgb=3, clamp_mode=c["clamp"],
                                      last_back=c["last_back"], white_back=c["white_back"])
        assert torch.equal(rgb, c["rgb"]) and torch.equal(depth, c["depth"]) and torch.equal(w, c["weights"])
    for c in fix["sample_pdf"]:
        smp, book = orc.sample_pdf(c["bins"], c["weights"], c["u"])
        assert torch.equal(smp, c["samples"])
    for c in fix["rays"]:
        r = orc.rays(c["b"], c["img"], 12, 0.88, 1.12, c["S"], c["jitter"], c["theta"], c["phi"], 0.3, 0.155)
        assert torch.equal(r["points"], c["points"]) and torch.equal(r["z"], c["z"])
        assert torch.equal(r["dirs"], c["dirs"]) and torch.equal(r["origins"], c["origins"])
        assert torch.equal(r["pitch"], c["pitch"]) and torch.equal(r["yaw"], c["yaw"])


@pytest.mark.parametrize("tag", ["g_r8_flat_noise", "g_r8_hier_noise"])
def test_oracle_clamp_tape_records_and_replays_the_reference_branches(tag):
    """The relu clamp of fancy_integration (pigan_utils.py:246-252) as test instrumentation (round 4, oracle.ClampTape): on
    the golden cases that run with nerf_noise > 0, (1) a recording tape changes nothing — images and gradients stay the
    reference's —, (2) replaying the recorded branches (relu(x) -> x * branch) reproduces the recording run bit for bit,
    images and every gradient, and (3) the tape sees only the FINAL composite: one record of shape (b, n, E, 1) per forward
    (the coarse composite that feeds the resampler stays unpinned: the fine-sample placement has its own pin)."""
    fix = load_golden(tag)
    kw = fix["G_kwargs"]
    assert fix["nerf_noise"] > 0

    def run(tape):
        G = seeded_generator(fix["seed"], freeze=fix["freeze"])
        with orc.clamp_tape(tape):
            out = orc.generator_forward(dict(G.named_parameters()), fix["zs"], fix["rand"], fix["img_size"], kw["fov"], kw["ray_start"],
                                        kw["ray_end"], kw["num_steps"], kw["h_stddev"], kw["v_stddev"], kw["hierarchical_sample"],
                                        nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"], freeze_nerf=fix["freeze"])
        (out["imgs"] * fix["G0"]).sum().backward()
        return out["imgs"].detach(), {n: (None if p.grad is None else p.grad.clone()) for n, p in G.named_parameters()}

    rec = orc.ClampTape()
    img_rec, g_rec = run(rec)
    assert torch.equal(img_rec, run(None)[0])                                   # recording does not change the arithmetic
    assert max_rel(img_rec, fix["imgs"]) < 1e-6
    b, n = fix["zs"]["z_nerf"].shape[0], fix["img_size"] ** 2
    E = kw["num_steps"] * (2 if kw["hierarchical_sample"] else 1)
    assert len(rec.rec) == 1 and tuple(rec.rec[0].shape) == (b, n, E, 1)
    frac = float(rec.rec[0].float().mean())
    assert 0.0 < frac < 1.0                                                      # both branches occur: the pin is not vacuous
    pin = orc.ClampTape(pin=[rec.rec[0].to(torch.uint8)])
    img_pin, g_pin = run(pin)
    assert torch.equal(img_pin, img_rec)
    for name in g_rec:
        assert (g_rec[name] is None) == (g_pin[name] is None), name
        if g_rec[name] is not None:
            assert torch.equal(g_pin[name], g_rec[name]), name


G_SLICE_FP64_BAR = 1e-12         # fp64 rounding over the sums of a gradient (eps 1.1e-16 x their length), 10x the ~1e-13 expected
G_SLICE_FP32_BAR = None          # set below the test: 4 x the largest fp32 parameter-gradient difference measured


def test_generator_oracle_is_additive_over_batch_slices():
    """What the GPU tests at the training batches stand on (test_gpu_real_configs.py, the *_vs_sliced_oracle tests): nothing in
    the generator couples the images of a batch (PixelNorm is per row, every ray and style belongs to one image), so for the
    loss `(imgs * G0).sum()` the oracle's images on a batch are the concatenation, and its parameter gradients the sum, over
    slices of the batch evaluated on G0's rows of those images (with the aux image: rows i and b + i).  r16, S = 4 + 4
    hierarchical, aux image, nerf_noise 0.1, 4 images, whole against four slices of one image:
      fp64, nothing pinned:                   images 2.8e-15, worst parameter gradient 1.0e-14 (relative): the identity;
      fp32, the whole run's LeakyReLU gates, fine-sample placement and relu-clamp branches pinned in the slices:
                                              images 1.0e-06, worst parameter gradient 4.8e-06 (mapping_network_inr.base_net.1.weight);
                                              bar 4 x that, 1.9e-05.
    A gate, placement or branch that differs between the whole and the free-running sliced fp32 run is one of the path's
    discontinuities, not a slicing error: they are counted and printed (7 of 9.4 million gates, 1 of 4096 fine samples, no clamp branch here)."""
    from test_gpu_real_configs import _draws, _slice, KW
    b, img, S, noise = 4, 16, 4, 0.1
    n = img * img
    g = torch.Generator().manual_seed(416)
    zs, rand = _draws(g, b, img, S, True)
    G0 = torch.randn(2 * b, 3, img, img, generator=g) / (2 * b * 3 * img * img)

    def run(dtype, z1, r1, G01, pin=None, grad=True):
        G = seeded_generator(1234)
        cast = lambda t: t.to(dtype) if torch.is_floating_point(t) else t
        if dtype == torch.float64:
            G = G.double()
        tape = orc.GateTape(pin=pin and pin["gates"])
        ctape = orc.ClampTape(pin=pin and [pin["clamp"]])
        torch.set_default_dtype(dtype)
        try:
            with orc.gate_tape(tape), orc.clamp_tape(ctape), orc.fine_z_pin(pin and pin["fine_z"]), torch.set_grad_enabled(grad):
                out = orc.generator_forward(dict(G.named_parameters()), {k: cast(v) for k, v in z1.items()},
                                            {k: cast(v) for k, v in r1.items()}, img, KW["fov"], KW["ray_start"], KW["ray_end"], S,
                                            KW["h_stddev"], KW["v_stddev"], True, nerf_noise=noise, return_aux_img=True, keep=True)
            if grad:
                (out["imgs"] * cast(G01)).sum().backward()
        finally:
            torch.set_default_dtype(torch.float32)
        tape.done()
        return (out["imgs"].detach(), {k: p.grad.double() for k, p in G.named_parameters() if p.grad is not None},
                dict(gates=tape.rec, clamp=ctape.rec[0], fine_z=out["fine_z"].detach()))

    for dtype in (torch.float64, torch.float32):
        imgs, grads, whole = run(dtype, zs, rand, G0)
        assert len(grads) == 130
        s_imgs, s_grads, flips = torch.empty_like(imgs), {}, [0, 0, 0]
        for i in range(b):
            rows = torch.tensor([i, b + i])
            z1, r1 = _slice(zs, rand, i, b, n, S)
            pin = None
            if dtype == torch.float32:
                pin = dict(gates=[t[i:i + 1] for t in whole["gates"]], clamp=whole["clamp"][i:i + 1], fine_z=whole["fine_z"][i:i + 1])
                free = run(dtype, z1, r1, G0[rows], grad=False)[2]
                flips[0] += sum(int((a != w).sum()) for a, w in zip(free["gates"], pin["gates"]))
                flips[1] += int(((free["fine_z"] - pin["fine_z"]).abs() > 1e-4 * (KW["ray_end"] - KW["ray_start"])).sum())
                flips[2] += int((free["clamp"] != pin["clamp"]).sum())
            o, gs, _ = run(dtype, z1, r1, G0[rows], pin=pin)
            s_imgs[rows] = o
            for k, v in gs.items():
                s_grads[k] = v if k not in s_grads else s_grads[k] + v
        assert set(s_grads) == set(grads)
        errs = {k: float((s_grads[k] - v).norm() / v.norm().clamp_min(1e-300)) for k, v in grads.items()}
        wk = max(errs, key=errs.get)
        e_img = max_rel(s_imgs, imgs)
        print(f"G oracle whole vs sliced, {dtype}: images {e_img:.2e}, worst parameter gradient {errs[wk]:.2e} ({wk})"
              + (f"; free-running slices: {flips[0]} of {sum(t.numel() for t in whole['gates'])} gates, {flips[1]} of {whole['fine_z'].numel()} fine samples, {flips[2]} clamp branches differ from the whole run's"
                 if dtype == torch.float32 else ""))
        bar = G_SLICE_FP64_BAR if dtype == torch.float64 else G_SLICE_FP32_BAR
        assert e_img < bar and errs[wk] < bar, (dtype, e_img, wk, errs[wk])


G_SLICE_FP32_BAR = 4 * 4.75e-6
