"""CPU: the point-colour reference of tests/color_refs.py against the oracle, and the identity that makes a per-point auxiliary
colour a principled quantity: the auxiliary image is the volume rendering of the per-point field W f(x) + b."""
import copy

import torch
import torch.nn.functional as F

from color_refs import one_hot_projection, rgb_ref
from conftest import seeded_generator
from oracle import cips3d_oracle as orc
from siren_refs import generator_tensors, make_points, make_style, siren_ref


def _case(seed=21, B=2, P=257):
    G = seeded_generator(seed)
    style = make_style(B, seed)
    pts = make_points("box", B, P, seed)
    with torch.no_grad():
        t = [v.detach() for v in generator_tensors(G, style)]
    return G, style, pts, t


def test_rgb_ref_is_the_oracle_siren_through_the_auxiliary_layer():
    """fp32: the reference runs the oracle's operations in the oracle's order, so the two differ by nothing or by the order of a
    BLAS sum — a few ulp of values in [-1, 1] (2^-22 = 4 ulp at 1); fp64: 1e-13.  With and without tanh, with the module's own
    auxiliary layer and with a one-hot map (which must return the feature itself)."""
    G, style, pts, t = _case()
    W, b = G.aux_to_rbg[0].weight.detach(), G.aux_to_rbg[0].bias.detach()
    sd = {k: v.detach() for k, v in G.named_parameters()}
    with torch.no_grad():
        feat32 = orc.siren(sd, pts, style)[..., :32]
        feat64 = orc.siren({k: v.double() for k, v in sd.items()}, pts.double(), style.double())[..., :32]
        # the oracle forms the FiLM vectors in the dtype of its call: the fp64 comparison takes them formed in fp64 too
        t64 = [v.detach() for v in generator_tensors(copy.deepcopy(G).double(), style.double())]
    for tanh in (True, False):
        post = torch.tanh if tanh else (lambda y: y)
        own32 = rgb_ref(pts, t, W, b, tanh, dtype=torch.float32)
        assert own32.shape == (2, 257, 3) and own32.dtype == torch.float32
        assert float((own32 - post(F.linear(feat32, W, b))).abs().max()) <= 2.0 ** -22
        own64 = rgb_ref(pts, t64, W, b, tanh)
        assert own64.dtype == torch.float64
        assert float((own64 - post(F.linear(feat64, W.double(), b.double()))).abs().max()) <= 1e-13
    assert float(own64.abs().max()) > 1e-3                  # not a comparison of zeros
    Wh, bh = one_hot_projection((5, 17, 30))
    assert torch.equal(rgb_ref(pts, t64, Wh, bh, False), feat64[..., [5, 17, 30]])


def test_affine_colour_commutes_with_compositing_when_the_weights_sum_to_one():
    """for ray weights w_k >= 0 with sum 1 (last_back):  W (sum_k w_k f_k) + b == sum_k w_k (W f_k + b)  — in fp64 up to the
    rounding of two 32-term sums; without the normalisation the bias term breaks it"""
    G, style, pts, t = _case(seed=22, B=2, P=12 * 16)
    W, b = G.aux_to_rbg[0].weight.detach().double(), G.aux_to_rbg[0].bias.detach().double()
    with torch.no_grad():
        f = siren_ref(pts.double(), [v.double() for v in t])[..., :32].reshape(2, 16, 12, 32)       # 16 rays of 12 samples
    w = torch.rand(2, 16, 12, 1, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    w = w / w.sum(2, keepdim=True)
    image = F.linear((w * f).sum(2), W, b)                   # the auxiliary image before tanh
    field = (w * F.linear(f, W, b)).sum(2)                   # the rendering of the per-point colour
    assert float((image - field).abs().max()) <= 1e-14 * float(image.abs().max() + 1)
    w2 = 0.5 * w                                             # weights that sum to 0.5: the bias no longer carries over
    assert float((F.linear((w2 * f).sum(2), W, b) - (w2 * F.linear(f, W, b)).sum(2) - 0.5 * b).abs().max()) <= 1e-14
