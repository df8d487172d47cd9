"""CPU, shapes only: the per-call plan of the discriminator's convolution engine (_conv_plan) — what it answers about the
planes-only gradient, one condition flipped per case — and the two kinds of stride-0 zero tensors the engine makes: the
weight-port handles (ordinary tensors) and the planes-only placeholders (no values)."""
import pytest
import torch

BLUR = (None, 2, 2, 1)          # the folded Blur of a 3 x 3 stride-2 ConvLayer: only pads and sampling stride are read

# (x_shape, w_shape, stride, pad, pre, forms, planes-only without a data gradient, with one)
CASES = {
    "base": ((2, 64, 16, 16), (64, 64, 3, 3), 1, 1, None, ("implicit",) * 3, True, True),
    "wgrad_declined": ((1, 64, 4, 4), (64, 64, 3, 3), 1, 1, None, ("implicit",) * 3, False, False),      # B N = 16, no multiple of 32
    "dgrad_f32": ((2, 64, 17, 17), (64, 64, 3, 3), 2, 0, None, ("implicit", "f32", "implicit"), True, False),
    "wgrad_not_implicit": ((2, 48, 16, 16), (64, 48, 3, 3), 1, 1, None, ("f32",) * 3, False, False),
    "parity": ((2, 64, 16, 16), (64, 64, 3, 3), 2, 0, BLUR, ("implicit", "parity", "implicit"), True, True),
    "parity_one_ktile": ((2, 64, 16, 16), (32, 64, 3, 3), 2, 0, BLUR, ("implicit", "f32", "implicit"), True, False),
}


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", list(CASES))
def test_planes_only_truth_table(case, mode, monkeypatch):
    from cips3d_amd import discriminator as dm
    x_shape, w_shape, stride, pad, pre, forms, po, po_dx = CASES[case]
    monkeypatch.setattr(dm, "CONV_MODE", mode)
    plan = dm._conv_plan(x_shape, w_shape, stride, pad, pre)
    assert plan.forms == forms == dm._conv_forms(x_shape, w_shape, stride, pad, pre)
    assert plan.planes_only == (po, po_dx)
    assert plan.wgrad_declined == (case == "wgrad_declined")
    # the tensor part of _planes_only_ok: a CPU gradient is never planes-only
    dout = torch.empty(plan.out_shape)
    assert not dm._planes_only_ok(x_shape, w_shape, stride, pad, pre, True, dout)
    assert not dm._planes_only_ok(x_shape, w_shape, stride, pad, pre, False, dout)


def test_plan_shapes_and_single_pass_flags(monkeypatch):
    from cips3d_amd import discriminator as dm
    plan = dm._conv_plan((2, 64, 16, 16), (64, 64, 3, 3), 2, 0, BLUR)
    assert plan.blurred == (17, 17) == dm._pre_shape(16, 16, BLUR) and plan.out_shape == (2, 64, 8, 8)
    assert dm._conv_plan((4, 3, 9, 7), (8, 3, 1, 1), 1, 0).out_shape == (4, 8, 9, 7)
    for case, (x_shape, w_shape, stride, pad, pre, forms, _, _) in CASES.items():
        assert dm._conv_plan(x_shape, w_shape, stride, pad, pre).single == (False,) * 3          # mode "bf16x3"
    monkeypatch.setattr(dm, "CONV_MODE", "bf16")
    for case, (x_shape, w_shape, stride, pad, pre, forms, _, _) in CASES.items():
        plan = dm._conv_plan(x_shape, w_shape, stride, pad, pre)
        rule = dm._single_pass(x_shape, w_shape, stride, pad, pre)
        for form, flag, shape_ok in zip(plan.forms, plan.single, rule):
            assert flag is (form in ("implicit", "parity") and shape_ok), (case, form)
    # the shape rule alone says yes for the f32 data gradient of the stride-2 convolution without a Blur: the plan does not
    x_shape, w_shape, stride, pad, pre = CASES["dgrad_f32"][:5]
    assert dm._single_pass(x_shape, w_shape, stride, pad, pre)[1] is True
    assert dm._conv_plan(x_shape, w_shape, stride, pad, pre).single == (True, False, True)
    assert dm._conv_plan((4, 3, 8, 8), (512, 3, 1, 1), 1, 0).single == (False,) * 3               # "rgb"
    # no plan outlives the mode it was made for
    monkeypatch.setattr(dm, "CONV_MODE", "f32")
    assert dm._conv_plan(x_shape, w_shape, stride, pad, pre).forms == ("f32",) * 3
    monkeypatch.setattr(dm, "CONV_MODE", "bf16x2")
    with pytest.raises(ValueError):
        dm._conv_plan(x_shape, w_shape, stride, pad, pre)


def test_port_handles_are_dense_zeros_and_placeholders_are_not():
    from cips3d_amd import discriminator as dm
    w = torch.zeros(3)
    handle = dm._zero1(w).expand(2, 4, 8, 8)                      # what _WeightGradPort.forward returns
    assert not dm._is_planes_only(handle)
    dense = dm._dense(handle)
    assert dense.is_contiguous() and dense.shape == (2, 4, 8, 8) and not dense.any()
    g = torch.randn(2, 4, 8, 8)
    planes = object()                                             # stands for the ops.Planes of the gated gradient
    ph = dm._placeholder(g, planes)                               # what FusedLeakyReLUFunctionBackward hands on
    assert ph.shape == g.shape and ph.data_ptr() != handle.data_ptr()
    assert dm._is_planes_only(ph) and dm._grad_planes(ph) is planes
    for lost in (ph.detach(), ph[:1], ph.view(2, 4, 64)):         # new Python objects: neither flag nor planes
        assert not hasattr(lost, "_cips_planes_only") and dm._is_planes_only(lost)
        with pytest.raises(RuntimeError):
            dm._dense(lost)
        with pytest.raises(RuntimeError):
            dm._nhwc(lost)
    del ph._cips_planes_only
    assert dm._is_planes_only(ph)
    with pytest.raises(RuntimeError):
        dm._dense(ph)
    assert not dm._is_planes_only(g.sum(dim=(2, 3), keepdim=True).expand(2, 4, 8, 8))            # an ordinary stride-0 tensor
