"""Fitting styles (and optionally the camera) of a generator to an image: the reference's inverse-rendering demo
(`Projector`, exp/cips3d/models/st_web.py:66-186) on the native path.

The reference's loop calls `forward_with_frequencies` on styles; here that is GeneratorNerfINR.forward_styles /
render_styles.  Its rule is kept with its numbers: start at the mean styles of `init_samples` latents, one zero-initialised
offset per style key and image, styles = mean + offset + noise * randn * (steps - i) / steps, Adam(0.9, 0.999) with coupled
weight decay (grad += wd * offset), the learning rate times `lr_gamma` every `lr_decay_every` steps, a fixed camera
(h_stddev = v_stddev = 0).  Its loss, nn.MSELoss, is ops.pyramid_loss with one level; more levels stand in for the
perceptual term whose weights this repository does not have.  Depth and silhouette terms use render_styles' differentiable
depth and opacity maps."""
import math
from types import SimpleNamespace

import torch

from . import ops
from .optim import FusedClipAdamEMA


def lr_at(step, lr, lr_decay_every=100, lr_gamma=0.75):
    """the learning rate of 0-based step `step`: torch.optim.lr_scheduler.StepLR(step_size=lr_decay_every, gamma=lr_gamma)
    stepped once after every optimiser step (st_web.py:150-151, :184)"""
    return lr * lr_gamma ** (step // lr_decay_every)


def _maps(t, b, H, what):
    if t is None:
        return None
    if tuple(t.shape) != (b, 1, H, H):
        raise ValueError(f"project: {what} must be ({b}, 1, {H}, {H}), got {tuple(t.shape)}")
    return t.detach().float().contiguous()


def project(G, target, *, steps, img_size=None, fov=12, ray_start=0.88, ray_end=1.12, num_steps=24,
            hierarchical_sample=False, lr=1e-2, lr_decay_every=100, lr_gamma=0.75, weight_decay=1e-4, noise=0.03,
            init_samples=10000, level_weights=(1.,), kind="mse", eps=1e-3, weight=None, target_depth=None, depth_weight=0.,
            target_mask=None, mask_weight=0., fit_styles=True, fit_camera=False, camera_lr=None, h_mean=math.pi * 0.5,
            v_mean=math.pi * 0.5, seed=None, **render_kw):
    """Fit G's styles to `target` (b, 3, H, H) in [-1, 1], every image on its own (Adam is elementwise, nothing is clipped and
    the loss is per image) -> SimpleNamespace(styles, offsets, h_mean, v_mean, losses (steps, b), imgs).

    Per step: styles = mean + offset (+ annealed noise) -> forward_styles (render_styles when a depth or mask target is
    given) -> loss_b = pyramid_loss(imgs, target, weight, level_weights, kind, eps)
                       + depth_weight * pyramid_loss(depth, target_depth, target_mask, (1,), kind, eps)
                       + mask_weight * mse(opacity, target_mask)
    -> backward to the style leaves (and the camera leaves) -> FusedClipAdamEMA without clip or EMA.  A term whose weights
    are all zero is not built.  `fit_camera` makes h_mean / v_mean (b, 1) leaves with their own `camera_lr` (default lr);
    `fit_styles=False` keeps the offsets at zero.  G's parameters are frozen for the loop (requires_grad off, restored on
    exit) and no parameter's .grad is touched.  Nothing in the loop synchronises with the host: the losses go to a device
    tensor.  Random numbers: `seed` (if given) seeds torch first; then the `init_samples` latents of the mean styles are
    drawn (G.generate_avg_frequencies), then per step the noise (only if noise > 0) and the draws of the forward."""
    dev = next(G.parameters()).device
    if dev.type != 'cuda':
        raise RuntimeError("project runs on the GPU only (there is no CPU path)")
    if target.dim() != 4 or target.shape[1] != 3 or target.shape[2] != target.shape[3]:
        raise ValueError(f"project: target must be (b, 3, H, H), got {tuple(target.shape)}")
    b, H = target.shape[0], target.shape[2]
    if img_size is not None and img_size != H:
        raise ValueError(f"project: img_size {img_size} but the target is {H} x {H}")
    if steps < 1:
        raise ValueError("project: steps >= 1")
    target = target.detach().float().contiguous()
    weight, target_depth, target_mask = (_maps(t, b, H, n) for t, n in ((weight, "weight"), (target_depth, "target_depth"),
                                                                       (target_mask, "target_mask")))
    level_weights = tuple(float(v) for v in level_weights)
    use_img = any(v != 0 for v in level_weights)
    use_depth = target_depth is not None and depth_weight != 0
    use_mask = target_mask is not None and mask_weight != 0
    geo = target_depth is not None or target_mask is not None
    if not (use_img or use_depth or use_mask):
        raise ValueError("project: every loss term is switched off")
    if not (fit_styles or fit_camera):
        raise ValueError("project: nothing to fit (fit_styles and fit_camera are both off)")
    if seed is not None:
        torch.manual_seed(seed)

    kw = dict(img_size=H, fov=fov, ray_start=ray_start, ray_end=ray_end, num_steps=num_steps, h_stddev=0., v_stddev=0.,
              hierarchical_sample=hierarchical_sample, sample_dist='gaussian')
    kw.update(render_kw)
    flags = [p.requires_grad for p in G.parameters()]
    try:
        for p in G.parameters():
            p.requires_grad_(False)
        with torch.no_grad():
            avg = G.generate_avg_frequencies(num_samples=init_samples, device=dev)
            names = G.style_names
            # every key's (b, dim) block is contiguous in one flat buffer: the per-step arithmetic on the styles is a few
            # launches over all keys, and one optimiser tensor holds every offset
            sizes = [b * avg[n].shape[1] for n in names]
            starts = [sum(sizes[:i]) for i in range(len(names))]
            mean = torch.cat([avg[n].float().expand(b, -1).reshape(-1) for n in names])
            off = torch.zeros_like(mean)
            goff = torch.zeros_like(mean)

            def split(flat):
                return {n: flat[o:o + m].view(b, -1) for n, o, m in zip(names, starts, sizes)}

            losses = torch.zeros(steps, b, device=dev)
            cams = []
            if fit_camera:
                # one angle per image: a number, or a tensor of 1 or b elements
                h_mean, v_mean = (v.detach().to(dev, torch.float32).reshape(-1, 1).expand(b, 1).clone() if torch.is_tensor(v)
                                  else torch.full((b, 1), float(v), device=dev) for v in (h_mean, v_mean))
                cams = [h_mean.requires_grad_(True), v_mean.requires_grad_(True)]
        opt = cam_opt = None
        if fit_styles:
            # one optimiser tensor per key (views of the flat buffers): the optimiser walks a tensor in 64K-element chunks, one
            # workgroup each, so the flat buffer as ONE tensor would be updated by a workgroup or two (measured: 0.25 ms a step)
            params = list(split(off).values())
            for p, g in zip(params, split(goff).values()):
                p.grad = g
            opt = FusedClipAdamEMA(params, lr=lr, betas=(0.9, 0.999))
        if fit_camera:
            cam_opt = FusedClipAdamEMA(cams, lr=lr if camera_lr is None else camera_lr, betas=(0.9, 0.999))
        ones = torch.ones(b, device=dev)
        out = None
        for i in range(steps):
            with torch.no_grad():
                cur = mean + off
                if noise > 0:
                    cur.add_(torch.randn_like(cur), alpha=noise * (steps - i) / steps)
                leaves = split(cur)
                if fit_styles:
                    # coupled weight decay: the gradient buffer starts at wd * offset and autograd accumulates into it in
                    # place, through each key's view
                    torch.mul(off, weight_decay, out=goff)
                    for n, g in split(goff).items():
                        leaves[n].requires_grad_(True).grad = g
                for c in cams:
                    c.grad = None
            with torch.enable_grad():
                if geo:
                    out = G.render_styles(leaves, **kw, h_mean=h_mean, v_mean=v_mean)
                    imgs = out.imgs
                else:
                    imgs = G.forward_styles(leaves, **kw, h_mean=h_mean, v_mean=v_mean)[0]
                loss = None
                if use_img:
                    loss = ops.pyramid_loss(imgs, target, weight, level_weights, kind, eps)
                if use_depth:
                    t = ops.pyramid_loss(out.depth, target_depth, target_mask, (1.,), kind, eps) * depth_weight
                    loss = t if loss is None else loss + t
                if use_mask:
                    t = ops.pyramid_loss(out.opacity, target_mask, None, (1.,), "mse") * mask_weight
                    loss = t if loss is None else loss + t
            losses[i].copy_(loss.detach())
            torch.autograd.backward(loss, ones)
            if opt is not None:
                opt.lr = lr_at(i, lr, lr_decay_every, lr_gamma)
                opt.step()
            if cam_opt is not None:
                cam_opt.lr = lr_at(i, lr if camera_lr is None else camera_lr, lr_decay_every, lr_gamma)
                cam_opt.step()
    finally:
        for p, f in zip(G.parameters(), flags):
            p.requires_grad_(f)
    with torch.no_grad():
        styles = {n: t.clone() for n, t in split(mean + off).items()}
        offsets = {n: t.clone() for n, t in split(off).items()}
    det = lambda v: v.detach() if torch.is_tensor(v) else v
    return SimpleNamespace(styles=styles, offsets=offsets, h_mean=det(h_mean), v_mean=det(v_mean), losses=losses,
                           imgs=imgs.detach())
