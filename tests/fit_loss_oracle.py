"""The yardstick of the pyramid fit loss (cips3d_amd/csrc/fit_loss.hip, ops.pyramid_loss): its definition in fp64 torch,
avg_pool2d for the pyramids and autograd for the gradient.  Checked against closed forms in
test_fit_loss_yardstick_cpu.py; the GPU tests compare the kernel with it.

  d_0 = pred - target, d_{l+1} = 2x2 mean of d_l;   w_0 = weight (1 when None), w_{l+1} = 2x2 mean of w_l
  loss_b = sum_{l<L} lambda_l / (C H_l W_l) * sum_{c,y,x} w_l rho(d_l)
  rho(x) = x^2 ("mse")  or  sqrt(x^2 + eps^2) - eps ("charbonnier")"""
import torch
import torch.nn.functional as F


def rho(x, kind, eps):
    if kind == "mse":
        return x * x
    assert kind == "charbonnier" and eps > 0
    return torch.sqrt(x * x + eps * eps) - eps


def pyramid_loss64(pred, target, weight=None, level_weights=(1.,), kind="mse", eps=1e-3):
    """-> loss (b,) fp64 on the CPU, differentiable with respect to `pred` (give it as an fp64 tensor that requires grad)"""
    d = pred.double().cpu() - target.detach().double().cpu()
    b, C, H, W = d.shape
    w = torch.ones(b, 1, H, W, dtype=torch.float64) if weight is None else weight.detach().double().cpu()
    loss = torch.zeros(b, dtype=torch.float64)
    for l, lam in enumerate(level_weights):
        if l:
            d, w = F.avg_pool2d(d, 2), F.avg_pool2d(w, 2)
        loss = loss + float(lam) * (w * rho(d, kind, eps)).sum(dim=(1, 2, 3)) / (C * d.shape[2] * d.shape[3])
    return loss


def pyramid_loss64_grad(pred, target, weight=None, level_weights=(1.,), kind="mse", eps=1e-3, upstream=None):
    """-> loss (b,), d (sum_b upstream_b loss_b) / d pred (b,C,H,W), both fp64 (upstream: ones by default, which makes the
    gradient of image b the gradient of loss_b)"""
    p = pred.detach().double().cpu().requires_grad_(True)
    loss = pyramid_loss64(p, target, weight, level_weights, kind, eps)
    up = torch.ones_like(loss) if upstream is None else upstream.detach().double().cpu()
    grad, = torch.autograd.grad(loss, p, up)
    return loss.detach(), grad
