"""GPU: the pyramid fit loss kernel (csrc/fit_loss.hip, ops.pyramid_loss) against its fp64 yardstick (fit_loss_oracle.py).

Bars, derived: every term w_l rho(d_l) is non-negative and the terms are summed in a fixed tree of depth
<= log2(C H W) + 3 in fp32, so the loss carries a relative error of a few ulp per tree level, far below 1e-5; the gradient is a
sum of at most 8 products formed in fp64 and rounded to fp32 once (twice above level 5).  Both are held to max_rel < 1e-5
(conftest.max_rel).  Measured on one MI355X: loss <= 1.4e-7, gradient <= 1.3e-7."""
import pytest
import torch

from conftest import max_rel
from fit_loss_oracle import pyramid_loss64_grad

pytestmark = pytest.mark.gpu
BAR = 1e-5
# (b, C, H, W, L): a 1x1 top level, one level, ragged 32x32 tiles, non-square images, odd top sizes, C = 1 / 3, more than
# one tile per image, and the levels above the tile (L > 6)
SHAPES = [(1, 1, 2, 2, 2), (1, 3, 8, 8, 1), (2, 3, 8, 8, 4), (3, 1, 12, 20, 3), (2, 3, 24, 40, 4), (2, 3, 64, 64, 7),
          (1, 3, 128, 128, 5)]
LAMBDAS = (1.0, 0.5, 2.0, 0.25, 1.5, 0.75, 3.0, 0.6)
KINDS = [("mse", 1e-3), ("charbonnier", 1e-3), ("charbonnier", 0.5)]
WEIGHTS = ["none", "random", "zero_regions", "zero_image"]


def _inputs(b, C, H, W, wkind, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + b * 7 + C * 5 + H + W)
    pred = torch.rand(b, C, H, W, generator=g) * 2 - 1
    target = torch.rand(b, C, H, W, generator=g) * 2 - 1
    weight = None
    if wkind != "none":
        weight = torch.rand(b, 1, H, W, generator=g) + 0.05
        if wkind == "zero_regions":
            weight[:, :, : max(H // 2, 1), : max(W // 3, 1)] = 0
            weight[:, :, -1, :] = 0
        if wkind == "zero_image":
            weight[b - 1] = 0
    return pred, target, weight


def _run(ops, pred, target, weight, lw, kind, eps, upstream=None):
    d = torch.device("cuda:0")
    p = pred.to(d).requires_grad_(True)
    loss = ops.pyramid_loss(p, target.to(d), None if weight is None else weight.to(d), lw, kind, eps)
    up = torch.ones_like(loss) if upstream is None else upstream.to(d)
    grad, = torch.autograd.grad(loss, p, up)
    return loss.detach(), grad


@pytest.mark.parametrize("wkind", WEIGHTS)
@pytest.mark.parametrize("kind,eps", KINDS)
@pytest.mark.parametrize("b,C,H,W,L", SHAPES)
def test_kernel_against_the_fp64_yardstick(b, C, H, W, L, kind, eps, wkind):
    from cips3d_amd import ops
    pred, target, weight = _inputs(b, C, H, W, wkind)
    lw = LAMBDAS[:L]
    loss, grad = _run(ops, pred, target, weight, lw, kind, eps)
    want_loss, want_grad = pyramid_loss64_grad(pred, target, weight, lw, kind, eps)
    assert loss.shape == (b,) and grad.shape == pred.shape
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    el = float(((loss.cpu().double() - want_loss).abs() / want_loss.abs().clamp_min(1e-300)).max()) if wkind != "zero_image" \
        else max_rel(loss, want_loss)
    eg = max_rel(grad, want_grad)
    print(f"fit loss ({b},{C},{H},{W}) L={L} {kind} eps={eps} weight={wkind}: loss {el:.2e} grad {eg:.2e}")
    assert max_rel(loss, want_loss) < BAR and eg < BAR
    if wkind == "zero_image":
        assert float(loss[b - 1]) == 0 and bool((grad[b - 1] == 0).all())
        if b > 1:
            assert max_rel(grad[0], want_grad[0]) < BAR
    else:
        assert el < BAR                                  # every image on its own, not only the largest loss of the batch
        for i in range(b):
            assert max_rel(grad[i], want_grad[i]) < BAR, i


@pytest.mark.parametrize("kind,eps", KINDS)
@pytest.mark.parametrize("b,C,H,W,L", SHAPES)
def test_equal_images_give_zero_loss_and_zero_gradient(b, C, H, W, L, kind, eps):
    from cips3d_amd import ops
    pred, _, weight = _inputs(b, C, H, W, "random")
    loss, grad = _run(ops, pred, pred.clone(), weight, LAMBDAS[:L], kind, eps)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all())
    assert bool((loss == 0).all()) and bool((grad == 0).all())


@pytest.mark.parametrize("wkind", ["none", "random"])
@pytest.mark.parametrize("b,C,H,W,L", SHAPES)
def test_bits_repeat_and_do_not_depend_on_the_batch(b, C, H, W, L, wkind):
    """two calls give equal bits; image i of the batch gives the bits of the same image alone"""
    from cips3d_amd import ops
    pred, target, weight = _inputs(b, C, H, W, wkind, seed=2)
    lw = LAMBDAS[:L]
    loss, grad = _run(ops, pred, target, weight, lw, "charbonnier", 1e-2)
    loss2, grad2 = _run(ops, pred, target, weight, lw, "charbonnier", 1e-2)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    for i in range(b):
        li, gi = _run(ops, pred[i:i + 1], target[i:i + 1], None if weight is None else weight[i:i + 1], lw, "charbonnier", 1e-2)
        assert torch.equal(li, loss[i:i + 1]) and torch.equal(gi, grad[i:i + 1]), i


@pytest.mark.parametrize("b,C,H,W,L", [(3, 1, 12, 20, 3), (2, 3, 64, 64, 7)])
def test_backward_scales_the_stored_gradient_by_the_upstream(b, C, H, W, L):
    from cips3d_amd import ops
    pred, target, weight = _inputs(b, C, H, W, "random", seed=3)
    lw = LAMBDAS[:L]
    _, stored = _run(ops, pred, target, weight, lw, "mse", 1e-3)
    up = torch.tensor([1.75, 0.0, -0.3][:b])
    _, grad = _run(ops, pred, target, weight, lw, "mse", 1e-3, upstream=up)
    assert torch.equal(grad, stored * up.to(stored.device).view(b, 1, 1, 1))
    assert bool((grad[1] == 0).all()) and float(grad[0].abs().max()) > 0
    want = pyramid_loss64_grad(pred, target, weight, lw, "mse", 1e-3, upstream=up)[1]
    assert max_rel(grad, want) < BAR


def test_non_contiguous_inputs_and_a_loss_through_autograd():
    """what the projection loop hands over: a permuted view of the head's (b, H, W, 3) output, and a scalar made of the losses"""
    from cips3d_amd import ops
    d = torch.device("cuda:0")
    pred, target, _ = _inputs(2, 3, 16, 16, "none", seed=4)
    nhwc = pred.permute(0, 2, 3, 1).contiguous().to(d).requires_grad_(True)
    loss = ops.pyramid_loss(nhwc.permute(0, 3, 1, 2), target.to(d), None, (1., 1.), "mse")
    (loss * torch.tensor([2.0, 0.5], device=d)).sum().backward()
    want = pyramid_loss64_grad(pred, target, None, (1., 1.), "mse", upstream=torch.tensor([2.0, 0.5]))[1]
    assert max_rel(nhwc.grad.permute(0, 3, 1, 2), want) < BAR
