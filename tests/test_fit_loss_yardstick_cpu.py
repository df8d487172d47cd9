"""CPU: the fp64 yardstick of the pyramid fit loss (fit_loss_oracle.py) against closed forms, and the projection loop's
learning-rate schedule as a pure function."""
import math

import pytest
import torch
import torch.nn.functional as F

from fit_loss_oracle import pyramid_loss64, pyramid_loss64_grad, rho

LAMBDAS = (1.0, 0.5, 2.0, 0.25)


def _case(b, C, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, C, H, W, generator=g, dtype=torch.float64), torch.randn(b, C, H, W, generator=g, dtype=torch.float64),
            torch.rand(b, 1, H, W, generator=g, dtype=torch.float64) + 0.1)


def test_one_level_mse_is_mse_loss_per_image():
    pred, target, _ = _case(3, 3, 6, 10)
    got = pyramid_loss64(pred, target)
    want = torch.stack([F.mse_loss(pred[i], target[i]) for i in range(3)])
    assert torch.allclose(got, want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("kind", ["mse", "charbonnier"])
@pytest.mark.parametrize("weighted", [False, True])
def test_constant_difference_gives_the_sum_of_rho(kind, weighted):
    """d = c everywhere: every level's mean is c, and with a constant weight w every level's weight is w"""
    c, w, eps = -0.37, 1.7, 1e-2
    target = _case(2, 3, 16, 24)[1]
    weight = torch.full((2, 1, 16, 24), w, dtype=torch.float64) if weighted else None
    got = pyramid_loss64(target + c, target, weight, LAMBDAS, kind, eps)
    want = sum(LAMBDAS) * float(rho(torch.tensor(c, dtype=torch.float64), kind, eps)) * (w if weighted else 1.0)
    assert torch.allclose(got, torch.full((2,), want, dtype=torch.float64), rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind", ["mse", "charbonnier"])
def test_gradient_agrees_with_central_differences(kind):
    pred, target, weight = _case(2, 2, 8, 8, seed=3)
    up = torch.tensor([0.7, -1.3], dtype=torch.float64)
    _, grad = pyramid_loss64_grad(pred, target, weight, LAMBDAS, kind, 1e-1, upstream=up)
    h = 1e-6
    g = torch.Generator().manual_seed(9)
    for _ in range(24):
        i = tuple(int(torch.randint(0, s, (1,), generator=g)) for s in pred.shape)
        e = torch.zeros_like(pred)
        e[i] = h
        f = lambda p: float((pyramid_loss64(p, target, weight, LAMBDAS, kind, 1e-1) * up).sum())
        fd = (f(pred + e) - f(pred - e)) / (2 * h)
        assert abs(fd - float(grad[i])) <= 1e-8 * max(1.0, abs(fd)), (i, fd, float(grad[i]))


@pytest.mark.parametrize("kind", ["mse", "charbonnier"])
def test_zero_weight_gives_zero_loss_and_zero_gradient(kind):
    pred, target, weight = _case(2, 3, 8, 8, seed=5)
    weight[1] = 0
    loss, grad = pyramid_loss64_grad(pred, target, weight, LAMBDAS, kind, 1e-3)
    assert float(loss[1]) == 0 and bool((grad[1] == 0).all())
    assert float(loss[0]) > 0 and float(grad[0].abs().max()) > 0


def test_image_results_do_not_depend_on_the_batch():
    pred, target, weight = _case(3, 3, 8, 8, seed=6)
    loss, grad = pyramid_loss64_grad(pred, target, weight, LAMBDAS[:3])
    l1, g1 = pyramid_loss64_grad(pred[1:2], target[1:2], weight[1:2], LAMBDAS[:3])
    assert torch.equal(loss[1:2], l1) and torch.equal(grad[1:2], g1)


def test_learning_rate_schedule():
    """StepLR(step_size, gamma) stepped after every optimiser step: step i runs at lr * gamma ** (i // step_size)"""
    from cips3d_amd.projection import lr_at
    assert lr_at(0, 1e-2) == 1e-2 and lr_at(99, 1e-2) == 1e-2
    assert lr_at(100, 1e-2) == 1e-2 * 0.75 and lr_at(199, 1e-2) == 1e-2 * 0.75
    assert lr_at(1000, 1e-2) == 1e-2 * 0.75 ** 10
    assert lr_at(7, 0.5, lr_decay_every=3, lr_gamma=0.1) == pytest.approx(0.5 * 0.1 ** 2, rel=1e-15)
    sched = torch.optim.lr_scheduler.StepLR(torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=1e-2), step_size=4, gamma=0.75)
    for i in range(13):
        assert math.isclose(sched.get_last_lr()[0], lr_at(i, 1e-2, 4, 0.75), rel_tol=1e-12)
        sched.optimizer.step()
        sched.step()
