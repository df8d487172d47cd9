"""GPU: the generator_v1 drop-ins (cips3d_amd/generator_v1.py) on the HIP path — against the golden vectors minted from the
reference's generator_v1 (scripts/make_golden_v1.py), against the CPU oracle at the AFHQ recipes' geometry, and for the one
thing v1 changes in the stream schedule: the caller's stream joins the INR mapping side stream before the first SIREN launch,
whose colour FiLM layer reads nerf_rgb_mapping's output."""
import pytest
import torch
import torch.nn.functional as F

from conftest import check_checksums, load_gates, load_golden, max_rel, pack_bitplane
from oracle import cips3d_oracle as orc
from test_generator_v1_cpu import seeded_generator_v1

pytestmark = pytest.mark.gpu
TOL = 1e-3
GRAD_TOL = 2e-4
GRAD_CASES = ["g_v1_r16_hier", "g_v1_r16_part", "g_v1_r8_freeze"]


@pytest.fixture(params=["f32", "bf16x3", "f32_all"])
def inr_mode(request):
    """the three numeric modes of test_gpu_generator.py: exact fp32 head / SIREN forward, the split-bf16 default, and no split
    operand anywhere (SIREN backward as the fp32 data pass too)"""
    from cips3d_amd import ops
    old = (ops.INR_MODE, ops.SIREN_FWD_MODE, ops.SIREN_BWD_MODE)
    ops.INR_MODE = "bf16x3" if request.param == "bf16x3" else "f32"
    ops.SIREN_FWD_MODE = "x3" if request.param == "bf16x3" else "f32"
    ops.SIREN_BWD_MODE = "staged_f32" if request.param == "f32_all" else "x3"
    yield request.param
    ops.INR_MODE, ops.SIREN_FWD_MODE, ops.SIREN_BWD_MODE = old


def _inputs(fix, d):
    return {k: v.to(d) for k, v in fix["zs"].items()}, {k: v.to(d) for k, v in fix["rand"].items()}


def _step(G, fix, d, pin=None):
    """one forward + backward of (imgs * G0).sum() on the fixture's latents and draws -> imgs, {name: grad or None}"""
    from cips3d_amd import ops
    zs, rand = _inputs(fix, d)
    for p in G.parameters():
        p.grad = None
    with ops.gate_debug(pin=pin):
        imgs, pitch_yaw = G(zs, img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"],
                            grad_points=fix.get("grad_points"), forward_points=None, rand_override=rand, **fix["G_kwargs"])
    (imgs * fix["G0"].to(d)).sum().backward()
    torch.cuda.synchronize()
    return imgs.detach(), pitch_yaw.detach(), {n: (None if p.grad is None else p.grad.detach().clone())
                                                for n, p in G.named_parameters()}


@pytest.mark.parametrize("tag", GRAD_CASES)
def test_generator_v1_matches_reference_golden(tag, inr_mode):
    """images within 1e-3 of the reference's generator_v1; with the head's LeakyReLU gates pinned to the reference's, every
    parameter gradient within 2e-4 of the reference's fp32 digest (nerf_rgb_mapping's included: the colour FiLM path back
    through the INR mapping network).  Which parameters get a gradient: the reference's set — for the freeze variant exactly,
    so mapping_network_inr.* and nerf_rgb_mapping.* get none (generator_v1.py:1982-1990)."""
    fix = load_golden(tag)
    d = torch.device("cuda:0")
    G = seeded_generator_v1(fix["seed"], freeze=fix["freeze"], device=d)
    check_checksums({k: v.cpu() for k, v in G.state_dict().items()}, fix["state_checksums"])
    imgs, pitch_yaw, grads = _step(G, fix, d, pin=[pack_bitplane(g) for g in load_gates(tag)])
    e = max_rel(imgs, fix["imgs"])
    assert imgs.shape == fix["imgs"].shape and e < TOL and max_rel(pitch_yaw, fix["pitch_yaw"]) < 1e-5
    ref_set = {n for n, dg in fix["grads"].items() if dg is not None}
    own_set = {n for n, g in grads.items() if g is not None}
    if fix["freeze"]:
        assert own_set == ref_set
        assert not any(n.startswith(("mapping_network_inr.", "nerf_rgb_mapping.", "siren.", "mapping_network_nerf.",
                                     "aux_to_rbg.")) for n in own_set)
    else:
        assert ref_set <= own_set and all(float(grads[n].abs().max()) == 0.0 for n in own_set - ref_set)
        assert {"nerf_rgb_mapping.weight", "nerf_rgb_mapping.bias"} <= ref_set
    rows = []
    for name in sorted(ref_set):
        dg, g = fix["grads"][name], grads[name].double().cpu().reshape(-1)
        ref = dg["sample"].double()
        eref = float((g[::dg["stride"]] - ref).norm() / ref.norm().clamp_min(1e-300))
        enorm = abs(float(g.norm()) - dg["norm"]) / max(dg["norm"], 1e-300)
        rows.append((max(eref, enorm), name))
    worst = max(rows)
    print(f"{tag} [{inr_mode}]: imgs max_rel {e:.3e}; {len(rows)} gradients, worst {worst[0]:.3e} at {worst[1]}")
    bad = [r for r in rows if r[0] > GRAD_TOL]
    assert not bad, bad


def test_generator_v1_eval_psi_staged_matches_reference_golden(inr_mode):
    """psi < 1 truncates towards generate_avg_frequencies' averages, nerf_rgb after nerf_rgb_mapping (the 10 000 latents the
    reference drew, regenerated on the CPU), rendered by the staged forward (forward_points) with its draw order"""
    from test_oracle_golden import eval_avg_styles
    fix = load_golden("g_v1_r8_eval_psi_staged")
    d = torch.device("cuda:0")
    G = seeded_generator_v1(fix["seed"], device=d)
    check_checksums({k: v.cpu() for k, v in G.state_dict().items()}, fix["state_checksums"])
    az = eval_avg_styles(fix, seeded_generator_v1(fix["seed"]))
    real_get_zs = G.get_zs
    G.get_zs = lambda n, **k: {k_: v.to(d) for k_, v in az.items()} if n == 10000 else real_get_zs(n, **k)
    zs, rand = _inputs(fix, d)
    with torch.no_grad():
        imgs, py = G(zs, img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"], grad_points=None,
                     forward_points=fix["forward_points"], rand_override=rand, **fix["G_kwargs"])
    ref = fix["avg"]["styles"]
    assert list(G.avg_styles) == list(ref) and G.avg_styles["nerf_rgb"].shape == (1, 128)
    for k, v in G.avg_styles.items():
        assert max_rel(v, ref[k]) < 1e-4, k
    e = max_rel(imgs, fix["imgs"])
    print(f"g_v1_r8_eval_psi_staged [{inr_mode}]: imgs max_rel {e:.3e}")
    assert imgs.shape == fix["imgs"].shape and e < TOL and max_rel(py, fix["pitch_yaw"]) < 1e-5


def test_generator_v1_ignores_up_vector():
    """generator_v1.py:1845 has no up_vector parameter: forward_camera_pos_and_lookup(..., up_vector=u, forward_points=...)
    renders the same images as without it, bit for bit — on the staged path, where v0's method honours it (checked on the same
    model, so the up vector used does change the picture)"""
    from cips3d_amd import generator
    d = torch.device("cuda:0")
    G = seeded_generator_v1(5, device=d)
    g = torch.Generator().manual_seed(9)
    b, img, S = 2, 8, 4
    n = img * img
    zs = {"z_nerf": torch.randn(b, 256, generator=g).to(d), "z_inr": torch.randn(b, 512, generator=g).to(d)}
    pos = F.normalize(torch.randn(b, 3, generator=g), dim=-1)
    cam = dict(camera_pos=pos.to(d), camera_lookup=(-pos + 0.05 * torch.randn(b, 3, generator=g)).to(d))
    rand = dict(jitter=torch.rand(b, n, S, 1, generator=g), noise_c=torch.randn(b, n, S, 1, generator=g),
                u=torch.rand(b * n, S, generator=g), noise_f=torch.randn(b, n, 2 * S, 1, generator=g))
    kw = dict(img_size=img, fov=12, ray_start=0.8, ray_end=1.2, num_steps=S, h_stddev=0.5, v_stddev=0.4, h_mean=1.5708,
              v_mean=1.5708, hierarchical_sample=True, sample_dist="gaussian", forward_points=40,
              rand_override={k: v.to(d) for k, v in rand.items()}, **cam)
    up = F.normalize(torch.tensor([[0.3, 1.0, 0.2]]), dim=-1).to(d)
    with torch.no_grad():
        plain, _ = G.forward_camera_pos_and_lookup(zs, **kw)
        with_up, _ = G.forward_camera_pos_and_lookup(zs, up_vector=up, **kw)
        honoured, _ = generator.GeneratorNerfINR.forward_camera_pos_and_lookup(G, zs, up_vector=up, **kw)
    assert torch.isfinite(plain).all() and torch.equal(plain, with_up)
    assert float((honoured - plain).abs().max()) > 1e-3


def test_generator_v1_joins_the_side_stream_before_the_colour_film(monkeypatch):
    """every FiLM launch of the SIREN (generator._film_all: w0, w1 and the colour layer in one call) runs after the caller's
    stream joined the INR mapping side stream — in grad-enabled forwards over the hierarchical path (gradient ports open), the
    fused ray march and part_grad_forward.  v0 keeps the fork open there (it joins before the head): the same probe sees it
    pending, so the probe can tell.  Then the race itself: a spin kernel queued on the side stream ahead of the INR mapping
    chain delays nerf_rgb, and the images stay bit-identical."""
    from cips3d_amd import generator
    from conftest import seeded_generator
    d = torch.device("cuda:0")
    fix = load_golden("g_v1_r16_hier")
    seen = []
    orig = generator._film_all

    def probe(layers, styles):
        seen.append((current[0], getattr(current[0], "_pending_side", None)))
        return orig(layers, styles)

    monkeypatch.setattr(generator, "_film_all", probe)
    current = [None]
    zs, rand = _inputs(fix, d)
    kw = dict(fix["G_kwargs"])
    G = seeded_generator_v1(fix["seed"], device=d)
    current[0] = G
    for hier, extra in ((True, {}), (False, {}), (True, {"grad_points": 96})):
        kw["hierarchical_sample"] = hier
        n0 = len(seen)
        imgs, _ = G(zs, img_size=fix["img_size"], nerf_noise=0.0, return_aux_img=True, forward_points=None,
                    rand_override=rand if hier and not extra else None, **extra, **kw)
        imgs.square().mean().backward()
        assert len(seen) > n0 and all(pending is None for _, pending in seen[n0:]), (hier, extra)
    # v0: pending at the same launch
    G0 = seeded_generator(fix["seed"], device=d)
    current[0] = G0
    kw["hierarchical_sample"] = True
    n0 = len(seen)
    G0(zs, img_size=fix["img_size"], nerf_noise=0.0, return_aux_img=True, forward_points=None, rand_override=rand, **kw)
    assert len(seen) > n0 and all(pending is not None for _, pending in seen[n0:])
    monkeypatch.setattr(generator, "_film_all", orig)
    # the race: delay the side stream's INR chain by a spin kernel; a missing join would read nerf_rgb before it is written
    if not hasattr(torch.cuda, "_sleep"):
        pytest.skip("torch.cuda._sleep unavailable")
    imgs_ref, _, grads_ref = _step(G, fix, d)
    real_map = type(G)._map_inr

    def slow_map(self, z_inr):
        torch.cuda._sleep(50_000_000)
        return real_map(self, z_inr)

    monkeypatch.setattr(type(G), "_map_inr", slow_map)
    imgs_slow, _, grads_slow = _step(G, fix, d)
    assert torch.equal(imgs_slow, imgs_ref)
    assert all((a is None) == (grads_slow[k] is None) and (a is None or torch.equal(a, grads_slow[k])) for k, a in grads_ref.items())


def test_captured_v1_step_replays_the_eager_images_and_gradients():
    """cips3d_amd.graph: a v1 G step (fork to the side stream, join before the march, gradient ports, backward) captured once
    replays to the eager step's images and gradients, bit for bit"""
    from cips3d_amd.graph import capture
    fix = load_golden("g_v1_r16_hier")
    d = torch.device("cuda:0")
    G = seeded_generator_v1(fix["seed"], device=d)
    zs, rand = _inputs(fix, d)
    G0 = fix["G0"].to(d)
    params = [p for p in G.parameters() if p.requires_grad]
    img_buf = torch.zeros_like(fix["imgs"], device=d)

    def step():
        for p in params:
            p.grad = None
        imgs, _ = G(zs, img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"], grad_points=None,
                    forward_points=None, rand_override=rand, **fix["G_kwargs"])
        (imgs * G0).sum().backward()
        img_buf.copy_(imgs.detach())

    step()
    torch.cuda.synchronize()
    eager_imgs = img_buf.clone()
    eager = [None if p.grad is None else p.grad.detach().clone() for p in params]
    cs = capture(step, warmup=1, params=params)
    for _ in range(2):
        cs()
    torch.cuda.synchronize()
    assert max_rel(eager_imgs, fix["imgs"]) < TOL
    assert torch.equal(img_buf, eager_imgs)
    n = 0
    for (name, p), g in zip([(n_, p_) for n_, p_ in G.named_parameters() if p_.requires_grad], eager):
        assert (p.grad is None) == (g is None), name
        if g is not None:
            n += 1
            assert torch.equal(p.grad, g), (name, float((p.grad - g).abs().max()))
    assert n > 100


@pytest.mark.parametrize("tag", ["g_v1_r16_hier", "g_v1_r8_freeze"])
def test_v1_weight_gradient_tail_on_the_side_stream_gives_the_same_gradients(tag):
    """ops.INR_TAIL with v1's earlier join: the ported tail (opened before the march, on the side stream that v1 joins before
    the march) against the plain head — the same images bit for bit, the same gradients up to the tail kernels' summation order,
    the ported form taken where a NeRF backward follows (not for the freeze variant), its ports waited for the compositing
    backward's event, and no gate left armed"""
    from cips3d_amd import ops
    if ops.INR_MODE != "bf16x3":
        pytest.skip("the ports belong to the split-bf16 head")
    fix = load_golden(tag)
    d = torch.device("cuda:0")
    G = seeded_generator_v1(fix["seed"], freeze=fix["freeze"], device=d)
    zs, rand = _inputs(fix, d)
    calls = []
    orig = ops.inr_head_with_ports
    ops.inr_head_with_ports = lambda *a, **k: (calls.append(a[3]), orig(*a, **k))[1]
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
            assert (len(calls) - n0 == 1) == (mode == "side" and not fix["freeze"])
            assert all(ports.waited for ports in calls[n0:])
            assert not ops._TAIL_GATE
            out.setdefault(mode, []).append((imgs.detach().clone(), {n: p.grad.clone() for n, p in G.named_parameters()
                                                                     if p.grad is not None}))
    finally:
        ops.INR_TAIL = keep
        ops.inr_head_with_ports = orig
    (im_m, g_m), (im_s, g_s), (im_s2, g_s2) = out["main"][0], out["side"][0], out["side"][1]
    assert torch.equal(im_m, im_s) and torch.equal(im_s, im_s2)
    assert g_m.keys() == g_s.keys() == g_s2.keys()
    for k in g_m:
        assert torch.equal(g_s[k], g_s2[k]), k
        scale = float(g_m[k].abs().max()) + 1e-30
        assert float((g_m[k] - g_s[k]).abs().max()) <= 5e-6 * scale, (k, float((g_m[k] - g_s[k]).abs().max()) / scale)


def test_afhq_recipe_geometry_r64_e96_forward_backward_vs_oracle(monkeypatch):
    """The AFHQ r64 recipes (afhq_exp/train_afhq_r64.sh passes G_kwargs.num_steps 48 over afhq_exp.yaml:64-77): r64, S = 48 + 48
    hierarchical (E = 96), fov 12, rays 0.8-1.2, h/v stddev 0.5/0.4, aux image, an image pair, nerf_noise 0.1 — forward and every
    parameter gradient of the v1 generator against the CPU oracle, through test_gpu_real_configs' C3 machinery (gates, fine-sample
    placement and relu-clamp branches pinned; bars against fp64).  The oracle's SIREN takes its colour FiLM style from
    nerf_rgb_mapping(w_inr) here, v1's composition."""
    import test_gpu_real_configs as rc
    captured = {}
    real_mapping_inr, real_siren = orc.mapping_inr, orc.siren

    def mapping_inr(sd, z, *a, **k):
        captured["w_inr"] = real_mapping_inr(sd, z, *a, **k)
        return captured["w_inr"]

    def siren_v1(sd, points, w_nerf, prefix="siren."):
        w_rgb = F.linear(captured["w_inr"], sd["nerf_rgb_mapping.weight"], sd["nerf_rgb_mapping.bias"])
        x = points * (2 / 0.24)
        idx = 0
        while prefix + f"network.{idx}.linear.weight" in sd:
            x = orc.film(sd, prefix + f"network.{idx}.", x, w_nerf)
            idx += 1
        sigma = F.linear(x, sd[prefix + "final_layer.weight"], sd[prefix + "final_layer.bias"])
        c = orc.film(sd, prefix + "color_layer_sine.", x, w_rgb)
        feat = F.linear(c, sd[prefix + "color_layer_linear.0.weight"], sd[prefix + "color_layer_linear.0.bias"])
        return torch.cat([feat, sigma], dim=-1)

    monkeypatch.setattr(orc, "mapping_inr", mapping_inr)
    monkeypatch.setattr(orc, "siren", siren_v1)
    monkeypatch.setattr(rc, "seeded_generator", seeded_generator_v1)
    monkeypatch.setattr(rc, "KW", dict(fov=12, ray_start=0.8, ray_end=1.2, h_stddev=0.5, v_stddev=0.4))
    n = rc._g_forward_backward_vs_oracle("AFHQ r64 b=2 S=48+48 (E=96), aux, nerf_noise 0.1, v1", 2, 64, 48, True, True, 0.1, 6448,
                                         pin_fine=True, pin_clamp=True, tol=2e-4)
    assert n == 132, n            # v0's 130 parameter gradients + nerf_rgb_mapping.weight / .bias
