"""CPU: the yardstick of tests/test_gpu_density_gradient.py — the gradient of the oracle's sigma w.r.t. its points argument by
fp64 autograd — against central differences of the same fp64 function."""
import pytest
import torch

from oracle import cips3d_oracle as orc
from test_gpu_kernels import _siren_inputs


@pytest.mark.parametrize("seed,b,P", [(5, 2, 32 * 7 + 5), (11, 2, 4096 + 160)])
def test_fp64_autograd_of_the_oracle_agrees_with_central_differences(seed, b, P):
    """h = 1e-6: the truncation error is h^2 / 6 times the third derivative and the rounding error 2^-53 |sigma| / h, both
    orders below the 1e-8 of max |grad sigma| asked for (measured: 1.8e-10 and 1.6e-10)"""
    G, pts, style = _siren_inputs(seed, b, P)
    sd = {k: v.detach().double() for k, v in G.named_parameters()}
    st = style.double()
    p = pts.double().clone().requires_grad_(True)
    grad, = torch.autograd.grad(orc.siren(sd, p, st)[..., 32].sum(), p)
    h = 1e-6
    fd = torch.empty_like(grad)
    with torch.no_grad():
        for a in range(3):
            e = torch.zeros(3, dtype=torch.float64)
            e[a] = h
            fd[..., a] = (orc.siren(sd, pts.double() + e, st)[..., 32] - orc.siren(sd, pts.double() - e, st)[..., 32]) / (2 * h)
    err = float((grad - fd).abs().max() / grad.abs().max())
    print(f"oracle fp64 autograd vs central differences, seed {seed} ({b}, {P}): {err:.2e} of max |grad sigma|")
    assert grad.shape == (b, P, 3) and torch.isfinite(grad).all()
    assert err < 1e-8
