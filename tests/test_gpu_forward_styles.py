"""GPU: the style-space entry points of the generator — styles(), forward_styles(), render_styles().

(a) forward_styles(styles(zs, psi)) is forward(zs, psi=psi) bit for bit, images and parameter gradients; likewise render_styles.
(b) style leaves (every key its own tensor, no parameter requires grad) against the fp64 oracle on two golden fixtures: the
    oracle knows one style per mapping network, so the leaves' gradients are summed per network.
(c) per key, with a different value in every key: a style enters the oracle only through its layer's style Linear(s), so
    s_k = w + delta_k is the shared style w with that layer's bias moved by W_k delta_k per image, and
    dL/ds_k = W_k^T dL/dbias_k, image by image.
(d) the freeze variant: the NeRF path runs under no_grad, its keys get no gradient."""
import math

import pytest
import torch

from conftest import G_CFG, load_gates, load_golden, max_rel, pack_bitplane, rel_err, seeded_generator
from oracle import cips3d_oracle as orc
from test_gpu_kernels import TOL, dev
from test_gpu_points_gradient import B_, KW, LOOK, POS, _gen_inputs

pytestmark = pytest.mark.gpu
FWD_TOL = 1e-3           # the forward bar of the golden tests (test_gpu_generator.TOL)


@pytest.fixture()
def x3(monkeypatch):
    from cips3d_amd import ops
    monkeypatch.setattr(ops, "SIREN_FWD_MODE", "x3")
    return ops


def _grads(G):
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in G.named_parameters()}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert (a[k] is None and b[k] is None) or (a[k] is not None and b[k] is not None and torch.equal(a[k], b[k])), k


def _pair(G, latent_call, style_call, zs, psi, G0):
    """one seed, the latent entry point; the same seed, styles() + the style entry point -> both results and gradients"""
    out = []
    for call in (lambda: latent_call(zs, psi), lambda: style_call(G.styles(zs, psi))):
        G.zero_grad(set_to_none=True)
        torch.manual_seed(77)
        r = call()
        imgs = r[0] if isinstance(r, tuple) else r.imgs
        loss = (imgs * G0.repeat(imgs.shape[0] // G0.shape[0], 1, 1, 1)).sum()
        if not isinstance(r, tuple):
            loss = loss + (r.depth * G0[:, :1]).sum() + (r.opacity * G0[:, 1:2]).sum()
        loss.backward()
        torch.cuda.synchronize()
        out.append((r, _grads(G)))
    return out


@pytest.mark.parametrize("psi,hier,aux,explicit", [(1, False, False, False), (0.7, False, False, False), (1, True, False, False),
                                                   (0.7, True, True, False), (1, False, True, False), (1, False, False, True),
                                                   (0.7, True, False, True)])
def test_forward_styles_is_forward(psi, hier, aux, explicit, x3):
    d = dev()
    G = seeded_generator(21, device=d)
    zs, rand, G0 = _gen_inputs(d, hier)
    kw = dict(KW, hierarchical_sample=hier, return_aux_img=aux, rand_override=rand)
    if explicit:
        cam = dict(camera_pos=POS.to(d), camera_lookup=LOOK.to(d))
        latent = lambda z, p: G.forward_camera_pos_and_lookup(z, h_mean=math.pi / 2, v_mean=math.pi / 2, psi=p, **kw, **cam)
        style = lambda st: G.forward_styles(st, **kw, **cam)
    else:
        latent = lambda z, p: G(z, psi=p, **kw)
        style = lambda st: G.forward_styles(st, **kw)
    (a, ga), (b, gb) = _pair(G, latent, style, zs, psi, G0)
    assert a[0].shape[0] == (2 * B_ if aux else B_)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert any(v is not None and float(v.abs().max()) > 0 for v in ga.values())
    _same(ga, gb)
    assert getattr(G, "_pending_side", None) is None and G.inr_net._tail is None


@pytest.mark.parametrize("psi,hier,explicit", [(1, False, False), (0.7, True, False), (1, True, True)])
def test_render_styles_is_render(psi, hier, explicit, x3):
    d = dev()
    G = seeded_generator(21, device=d)
    zs, rand, G0 = _gen_inputs(d, hier)
    kw = dict(KW, hierarchical_sample=hier, rand_override=rand)
    if explicit:
        kw.update(camera_pos=POS.to(d), camera_lookup=LOOK.to(d))
    (a, ga), (b, gb) = _pair(G, lambda z, p: G.render(z, psi=p, **kw), lambda st: G.render_styles(st, **kw), zs, psi, G0)
    assert torch.equal(a.imgs, b.imgs) and torch.equal(a.pitch_yaw, b.pitch_yaw)
    assert torch.equal(a.depth, b.depth) and torch.equal(a.opacity, b.opacity)
    assert b.depth.grad_fn is not None and b.opacity.grad_fn is not None
    _same(ga, gb)


def test_generator_v1_forward_styles_is_forward(x3):
    from cips3d_amd import generator_v1
    d = dev()
    torch.manual_seed(21)
    G = generator_v1.GeneratorNerfINR(**G_CFG, device="cpu").to(d)
    G.device = d
    zs, rand, G0 = _gen_inputs(d, True)
    kw = dict(KW, hierarchical_sample=True, rand_override=rand)
    (a, ga), (b, gb) = _pair(G, lambda z, p: G(z, psi=p, **kw), lambda st: G.forward_styles(st, **kw), zs, 0.7, G0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _same(ga, gb)
    st = G.styles(zs)
    assert tuple(st) == G.style_names and G.style_names[2] == "nerf_rgb" and st["nerf_rgb"].shape == (B_, 128)


def test_styles_is_joined_ordered_and_differentiable(x3):
    d = dev()
    G = seeded_generator(21, device=d)
    zs, _, _ = _gen_inputs(d, False)
    zs = {k: v.clone().requires_grad_(True) for k, v in zs.items()}
    st = G.styles(zs)
    assert tuple(st) == G.style_names and getattr(G, "_pending_side", None) is None
    assert all(st[n].shape == (B_, 128 if n.startswith("nerf") else 512) for n in st)
    sum(t.sum() for t in st.values()).backward()
    assert float(zs["z_nerf"].grad.abs().max()) > 0 and float(zs["z_inr"].grad.abs().max()) > 0
    assert G.mapping_network_nerf.base_net[0].weight.grad is not None and G.mapping_network_inr.base_net[0].weight.grad is not None
    with torch.no_grad():
        assert all(not t.requires_grad for t in G.styles(zs, psi=0.5).values())


# ---- (b), (c): style leaves against the fp64 oracle ----
def _style_linears(name):
    """style key -> the oracle's parameter prefixes of the Linear(s) the style enters through"""
    if name == "nerf_rgb":
        return ["siren.color_layer_sine.gain_fc.", "siren.color_layer_sine.bias_fc."]
    if name.startswith("nerf_w"):
        return [f"siren.network.{name[6:]}.gain_fc.", f"siren.network.{name[6:]}.bias_fc."]
    res, j = name[len("inr_w"):].split("_")
    return [f"inr_net.network.{res}.mod{int(j) + 1}.modulation."]


def _product(G, ops, fix, d, deltas, gates, fz):
    """forward_styles on leaves (styles(zs) + delta per key), every parameter frozen -> imgs, {key: leaf.grad}, the fine depths"""
    zs = {k: v.to(d) for k, v in fix["zs"].items()}
    rand = {k: v.to(d) for k, v in fix["rand"].items()}
    kw = {k: v for k, v in fix["G_kwargs"].items() if k != "psi"}
    kw.update(img_size=fix["img_size"], nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"], rand_override=rand)
    for p in G.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        st = G.styles(zs)
    leaves = {n: (t + deltas[n].to(d) if deltas else t.clone()).requires_grad_(True) for n, t in st.items()}
    if fz is None and fix["G_kwargs"]["hierarchical_sample"]:
        rec = []
        with torch.no_grad(), ops.gate_debug(pin=gates), ops.resample_debug(rec=rec):
            G.forward_styles(leaves, **kw)
        fz = rec[0]
    with ops.gate_debug(pin=gates), ops.resample_debug(pin=[fz] if fz is not None else None):
        imgs, _ = G.forward_styles(leaves, **kw)
    (imgs * fix["G0"].to(d)).sum().backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in G.parameters()), "a parameter's .grad was set"
    return imgs.detach(), {n: t.grad for n, t in leaves.items()}, fz


def _oracle(fix, ref_gates, fz, deltas):
    """fp64 oracle, gates and fine depths pinned -> imgs, dL/dw_nerf, dL/dw_inr, {key: dL/ds_key} (the last with deltas)"""
    G64 = seeded_generator(fix["seed"], freeze=fix["freeze"]).double()
    sd = dict(G64.named_parameters())
    kw = fix["G_kwargs"]
    dbl = lambda dd: {k: (v.double() if torch.is_floating_point(v) else v) for k, v in dd.items()}
    moved = {}
    if deltas:
        for name, dl in deltas.items():
            for pre in _style_linears(name):
                W = sd[pre + "weight"].detach()
                moved[pre] = (sd[pre + "bias"].detach() + dl.double() @ W.t()).requires_grad_(True)       # (b, out): per image
                sd[pre + "bias"] = moved[pre]
    tape = orc.GateTape(pin=ref_gates)
    torch.set_default_dtype(torch.float64)
    try:
        with orc.gate_tape(tape), orc.fine_z_pin(fz.detach().cpu().double() if fz is not None else None):
            o = orc.generator_forward(sd, dbl(fix["zs"]), dbl(fix["rand"]), fix["img_size"], kw["fov"], kw["ray_start"],
                                      kw["ray_end"], kw["num_steps"], kw["h_stddev"], kw["v_stddev"], kw["hierarchical_sample"],
                                      nerf_noise=fix["nerf_noise"], return_aux_img=fix["aux"], keep=True)
        tape.done()
        o["w_nerf"].retain_grad()
        o["w_inr"].retain_grad()
        (o["imgs"] * fix["G0"].double()).sum().backward()
    finally:
        torch.set_default_dtype(torch.float32)
    per_key = {}
    for name in (deltas or {}):
        per_key[name] = sum(moved[pre].grad @ sd[pre + "weight"].detach() for pre in _style_linears(name))
    return o["imgs"].detach(), o["w_nerf"].grad, o["w_inr"].grad, per_key


@pytest.mark.parametrize("tag", ["g_r8_flat_noise", "g_r16_hier"])
def test_style_leaves_sum_to_the_oracles_style_gradient(tag, x3):
    ops = x3
    d = dev()
    fix = load_golden(tag)
    ref_gates = load_gates(tag)
    G = seeded_generator(fix["seed"], device=d)
    fz = fix["fine_z"].reshape(-1, fix["G_kwargs"]["num_steps"]).to(d) if fix["G_kwargs"]["hierarchical_sample"] else None
    imgs, grads, _ = _product(G, ops, fix, d, None, [pack_bitplane(g) for g in ref_gates], fz)
    assert max_rel(imgs, fix["imgs"]) < FWD_TOL
    ref_imgs, g_nerf, g_inr, _ = _oracle(fix, ref_gates, fz, None)
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads.values())
    got_nerf = sum(g for n, g in grads.items() if n.startswith("nerf"))
    got_inr = sum(g for n, g in grads.items() if n.startswith("inr"))
    e = (max_rel(imgs, ref_imgs), rel_err(got_nerf, g_nerf), rel_err(got_inr, g_inr))
    print(f"style leaves {tag}: imgs {e[0]:.2e}; sum over NeRF keys {e[1]:.3e}, over INR keys {e[2]:.3e} against the fp64 oracle")
    assert e[0] < FWD_TOL and e[1] < TOL and e[2] < TOL


@pytest.mark.parametrize("tag", ["g_r8_flat_noise", "g_r16_hier"])
def test_every_style_key_on_its_own_value(tag, x3):
    ops = x3
    d = dev()
    fix = load_golden(tag)
    ref_gates = load_gates(tag)
    G = seeded_generator(fix["seed"], device=d)
    g = torch.Generator().manual_seed(31)
    b = fix["zs"]["z_nerf"].shape[0]
    # the styles have unit scale (the INR ones are LayerNorm outputs); a tenth of it moves every layer visibly
    deltas = {n: 0.1 * torch.randn(b, 128 if n.startswith("nerf") else 512, generator=g) for n in G.style_names}
    imgs, grads, fz = _product(G, ops, fix, d, deltas, [pack_bitplane(g_) for g_ in ref_gates], None)
    ref_imgs, _, _, per_key = _oracle(fix, ref_gates, fz, deltas)
    plain, _, _, _ = _oracle(fix, ref_gates, fz, None)
    assert max_rel(ref_imgs, plain) > 10 * FWD_TOL, "the deltas do not move the image: the case checks nothing"
    e_img = max_rel(imgs, ref_imgs)
    errs = {n: rel_err(grads[n], per_key[n]) for n in G.style_names}
    worst = max(errs, key=errs.get)
    print(f"style keys {tag}: imgs {e_img:.2e}; {len(errs)} keys, worst gradient rel err {errs[worst]:.3e} ({worst})")
    assert e_img < FWD_TOL
    for n, v in errs.items():
        assert float(per_key[n].abs().max()) > 0 and v < TOL, (n, v)


def test_freeze_variant_reaches_the_inr_keys_only(x3):
    d = dev()
    G = seeded_generator(21, freeze=True, device=d)
    zs, rand, G0 = _gen_inputs(d, False)
    for p in G.parameters():
        p.requires_grad_(False)
    with torch.no_grad():
        st = G.styles(zs)
    leaves = {n: t.clone().requires_grad_(True) for n, t in st.items()}
    imgs, _ = G.forward_styles(leaves, hierarchical_sample=False, rand_override=rand, **KW)
    (imgs * G0).sum().backward()
    for n, t in leaves.items():
        if n.startswith("nerf"):
            assert t.grad is None, n
        else:
            assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0, n
    assert all(p.grad is None for p in G.parameters())
