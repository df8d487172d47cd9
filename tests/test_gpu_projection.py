"""GPU: the projection loop (cips3d_amd/projection.py) — the rule of the reference's Projector on forward_styles /
render_styles, ops.pyramid_loss and FusedClipAdamEMA.  Every case: 16 x 16 images, 6 samples per ray, batch 2, mean styles of
64 latents, no style noise."""
import math

import pytest
import torch

from conftest import seeded_generator
from fit_loss_oracle import pyramid_loss64
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu
IMG, S_, B_ = 16, 6, 2
CAM = dict(fov=12, ray_start=0.88, ray_end=1.12, num_steps=S_)
KW = dict(CAM, img_size=IMG, h_stddev=0., v_stddev=0., hierarchical_sample=False, sample_dist="gaussian")
OPT = dict(init_samples=64, noise=0., seed=5, **CAM)
LR, ADAM_EPS = 1e-2, 1e-8


def _snapshot(G):
    return [(p.requires_grad, None if p.grad is None else p.grad.clone()) for p in G.parameters()]


def _check_untouched(G, snap):
    for (flag, grad), p in zip(snap, G.parameters()):
        assert p.requires_grad == flag
        assert (grad is None and p.grad is None) or torch.equal(grad, p.grad)


_TARGET = {}


def _target(G, d):
    """a target the generator can reach: its own render of truncated styles, with depth and a soft mask"""
    if "t" not in _TARGET:
        g = torch.Generator().manual_seed(900)
        zs = {"z_nerf": torch.randn(B_, 256, generator=g).to(d), "z_inr": torch.randn(B_, 512, generator=g).to(d)}
        with torch.no_grad():
            torch.manual_seed(901)
            r = G.render(zs, psi=0.7, **KW)
        _TARGET["t"] = (r.imgs.clone(), r.depth.clone(), r.opacity.clone())
    return _TARGET["t"]


def _first_step_gradient(G, target, level_weights, kind, eps, h_mean=math.pi / 2, camera=False):
    """the gradient of step 0, obtained without the loop: the mean styles as leaves -> forward_styles -> the torch loss that
    fit_loss_oracle checks in fp64 (here on the GPU tensors, in fp64) -> autograd"""
    d = target.device
    flags = [p.requires_grad for p in G.parameters()]
    for p in G.parameters():
        p.requires_grad_(False)
    try:
        torch.manual_seed(OPT["seed"])
        with torch.no_grad():
            avg = G.generate_avg_frequencies(num_samples=OPT["init_samples"], device=d)
        leaves = {n: avg[n].expand(B_, -1).clone().requires_grad_(True) for n in G.style_names}
        hm = torch.full((B_, 1), h_mean, device=d, requires_grad=camera)
        vm = torch.full((B_, 1), math.pi / 2, device=d, requires_grad=camera)
        imgs, _ = G.forward_styles(leaves, h_mean=hm if camera else h_mean, v_mean=vm if camera else math.pi / 2, **KW)
        p64 = imgs.double()
        d_ = p64 - target.double()
        loss = 0
        for l, lam in enumerate(level_weights):                     # fit_loss_oracle.pyramid_loss64, on the device
            if l:
                d_ = torch.nn.functional.avg_pool2d(d_, 2)
            r = d_ * d_ if kind == "mse" else torch.sqrt(d_ * d_ + eps * eps) - eps
            loss = loss + lam * r.sum(dim=(1, 2, 3)) / (3 * d_.shape[2] * d_.shape[3])
        assert torch.allclose(loss.detach().cpu(), pyramid_loss64(imgs.detach(), target, None, level_weights, kind, eps), rtol=1e-12)
        loss.sum().backward()
    finally:
        for p, f in zip(G.parameters(), flags):
            p.requires_grad_(f)
    return {n: t.grad for n, t in leaves.items()}, (hm.grad, vm.grad) if camera else None, loss.detach()


def _adam_first(g, lr=LR):
    return -lr * g / (g.abs() + ADAM_EPS)


@pytest.mark.parametrize("level_weights,kind", [((1.,), "mse"), ((1., 0.5, 0.25), "charbonnier")])
def test_first_step_is_adam_on_the_independent_gradient(level_weights, kind):
    from cips3d_amd.projection import project
    d = dev()
    G = seeded_generator(21, device=d)
    G.siren.final_layer.weight.grad = torch.ones_like(G.siren.final_layer.weight)       # a .grad the loop must leave alone
    G.inr_net.to_rgbs["4"].linear.weight.requires_grad_(False)                           # ... and a flag
    snap = _snapshot(G)
    target = _target(G, d)[0]
    want, _, loss0 = _first_step_gradient(G, target, level_weights, kind, 1e-2)
    res = project(G, target, steps=1, lr=LR, level_weights=level_weights, kind=kind, eps=1e-2, **OPT)
    _check_untouched(G, snap)
    assert res.losses.shape == (1, B_) and torch.allclose(res.losses[0].double(), loss0, rtol=1e-4)
    assert res.imgs.shape == (B_, 3, IMG, IMG) and tuple(res.offsets) == G.style_names == tuple(res.styles)
    worst = 0.0
    for n in G.style_names:
        assert float(want[n].abs().max()) > 0, n
        worst = max(worst, float((res.offsets[n] - _adam_first(want[n])).abs().max()))
        assert torch.equal(res.styles[n], G.avg_styles[n].expand(B_, -1) + res.offsets[n]), n
    print(f"projection step 1 {kind} {level_weights}: max |offset - Adam(g)| {worst:.2e} at lr {LR}")
    assert worst < 1e-6
    assert res.h_mean == math.pi / 2 and res.v_mean == math.pi / 2


def test_first_camera_step():
    from cips3d_amd.projection import project
    d = dev()
    G = seeded_generator(21, device=d)
    target = _target(G, d)[0]
    h0 = math.pi / 2 + 0.15
    want, (gh, gv), _ = _first_step_gradient(G, target, (1.,), "mse", 1e-3, h_mean=h0, camera=True)
    res = project(G, target, steps=1, lr=LR, fit_camera=True, camera_lr=2e-2, h_mean=h0, **OPT)
    assert res.h_mean.shape == (B_, 1) and res.v_mean.shape == (B_, 1) and not res.h_mean.requires_grad
    assert float(gh.abs().min()) > 0 and float(gv.abs().min()) > 0
    eh = float((res.h_mean - h0 - _adam_first(gh, 2e-2)).abs().max())
    ev = float((res.v_mean - math.pi / 2 - _adam_first(gv, 2e-2)).abs().max())
    eo = max(float((res.offsets[n] - _adam_first(want[n])).abs().max()) for n in G.style_names)
    print(f"projection camera step 1: h_mean {eh:.2e} v_mean {ev:.2e} offsets {eo:.2e}")
    # the angles are ~1.6: one fp32 ulp of them is 1.2e-7, so the absolute bar of the offsets holds for them too
    assert eh < 1e-6 and ev < 1e-6 and eo < 1e-6
    # the fitted angles come back per image, detached, and are what the style entry points take for a render
    with torch.no_grad():
        torch.manual_seed(8)
        both = G.forward_styles(res.styles, h_mean=res.h_mean, v_mean=res.v_mean, **KW)[0]
        torch.manual_seed(8)
        one = G.forward_styles({n: t[1:] for n, t in res.styles.items()}, h_mean=float(res.h_mean[1]), v_mean=float(res.v_mean[1]), **KW)[0]
    assert both.shape == (B_, 3, IMG, IMG) and one.shape == (1, 3, IMG, IMG)
    only = project(G, target, steps=1, lr=LR, fit_camera=True, fit_styles=False, h_mean=h0, **OPT)
    assert all(bool((t == 0).all()) for t in only.offsets.values()) and float((only.h_mean - h0).abs().min()) > 0


def test_mask_term_alone_moves_the_nerf_keys_only():
    from cips3d_amd.projection import project
    d = dev()
    G = seeded_generator(21, device=d)
    snap = _snapshot(G)
    target, depth, opacity = _target(G, d)
    mask = (opacity > opacity.median()).float()
    res = project(G, target, steps=3, lr=LR, level_weights=(0.,), target_mask=mask, mask_weight=1.0, **OPT)
    _check_untouched(G, snap)
    assert bool(torch.isfinite(res.losses).all()) and float(res.losses.min()) > 0
    for n, t in res.offsets.items():
        if n.startswith("inr"):
            assert bool((t == 0).all()), n
        elif n != "nerf_rgb":                # the opacity leaves the SIREN before the colour branch
            assert float(t.abs().max()) > 0, n
    # all three terms together run, too
    res = project(G, target, steps=2, lr=LR, target_depth=depth, depth_weight=0.5, target_mask=mask, mask_weight=0.25, **OPT)
    assert bool(torch.isfinite(res.losses).all()) and all(float(t.abs().max()) > 0 for t in res.offsets.values())


def test_fit_to_a_self_generated_target_reduces_the_loss():
    from cips3d_amd.projection import project
    d = dev()
    G = seeded_generator(21, device=d)
    snap = _snapshot(G)
    target = _target(G, d)[0]
    res = project(G, target, steps=40, lr=LR, level_weights=(1., 0.5), **OPT)
    _check_untouched(G, snap)
    losses = res.losses.cpu()
    assert losses.shape == (40, B_) and bool(torch.isfinite(losses).all())
    print(f"projection 40 steps: first {losses[0].tolist()} mean of the last five {losses[-5:].mean(0).tolist()}")
    assert bool((losses[-5:].mean(0) < losses[0]).all())


def test_render_views_is_forward_styles_per_angle():
    from cips3d_amd.evaluation import render_views
    d = dev()
    G = seeded_generator(21, device=d)
    g = torch.Generator().manual_seed(900)
    zs = {"z_nerf": torch.randn(B_, 256, generator=g).to(d), "z_inr": torch.randn(B_, 512, generator=g).to(d)}
    with torch.no_grad():
        styles = G.styles(zs)
    yaws, pitches = [math.pi / 2 - 0.3, math.pi / 2, math.pi / 2 + 0.3], [math.pi / 2, math.pi / 2 - 0.1, math.pi / 2]
    torch.manual_seed(3)
    views = render_views(G, styles, yaws, pitches, img_size=IMG, **CAM)
    assert len(views) == 3 and all(v.shape == (B_, 3, IMG, IMG) and not v.requires_grad for v in views)
    torch.manual_seed(3)
    with torch.no_grad():
        for v, yaw, pitch in zip(views, yaws, pitches):
            assert torch.equal(v, G.forward_styles(styles, h_mean=yaw, v_mean=pitch, **KW)[0])
    assert not torch.equal(views[0], views[2])
    with pytest.raises(ValueError):
        render_views(G, styles, yaws, pitches[:2], img_size=IMG, **CAM)
