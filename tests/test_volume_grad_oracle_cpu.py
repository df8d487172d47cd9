"""CPU: tests/volume_grad_oracle.py holds itself.  The rule of cips_volume_render_bwd restated by hand equals fp64 autograd of
volume_oracle.render; in fp32 it stays inside the bar that tests/test_gpu_volume_grad.py holds the kernel to; and every
deliberately wrong rule leaves that bar on every case where it can show."""
import pytest
import torch

import volume_grad_oracle as go
import volume_oracle as vo

CASES = go.all_cases()
SEES = [n for n in CASES if not n.startswith("miss_")]
# where each wrong rule can show (volume_grad_oracle's module text)
APPLIES = dict(
    no_top_up=[n for n in SEES if CASES[n].last_back and go.last_sample_inside(CASES[n])],
    go_sign=[n for n in SEES if CASES[n].clamp_mode == 'relu'],
    swap_t=SEES,
    relu_one=[n for n in SEES if CASES[n].clamp_mode == 'relu'],
    delta_prev=[n for n in SEES if CASES[n].clamp_mode == 'softplus' or go.last_sample_inside(CASES[n], every=True)],
)


def test_the_extra_case_has_no_near_pixel_and_sees_the_volume():
    for name in go.extra_cases():
        ref = vo.render(CASES[name], bars=True)
        assert int(ref.near.sum()) == 0 and float(ref.sees.float().mean()) > 0.2


@pytest.mark.parametrize("name", list(CASES))
def test_hand_rule_equals_autograd_in_fp64(name):
    ref = go.reference(name)
    m = go.measure(go.hand_rule(ref.case, ref.ups), ref.g64)
    print(f"{name}: hand rule fp64 sigma {m[0]:.2e}, colour {m[1]:.2e}")
    assert m[0] <= 1e-9 and m[1] <= 1e-9
    assert bool(torch.isfinite(ref.g64).all())


@pytest.mark.parametrize("name", list(CASES))
def test_hand_rule_in_fp32_stays_inside_the_bar(name):
    ref = go.reference(name)
    m = go.measure(go.hand_rule(ref.case, ref.ups, torch.float32), ref.g64)
    print(f"{name}: hand rule fp32 sigma {m[0]:.2e} (bar {ref.bar[0]:.2e}), colour {m[1]:.2e} (bar {ref.bar[1]:.2e})")
    assert go.within(m, ref.bar)


@pytest.mark.parametrize("variant,name", [(v, n) for v, names in APPLIES.items() for n in names])
def test_wrong_rules_leave_the_bar(variant, name):
    ref = go.reference(name)
    m = go.measure(go.hand_rule(ref.case, ref.ups, variant=variant), ref.g64)
    print(f"{variant} on {name}: sigma {m[0]:.2e} (bar {ref.bar[0]:.2e}), colour {m[1]:.2e} (bar {ref.bar[1]:.2e})")
    assert not go.within(m, ref.bar)


def test_every_wrong_rule_is_tried_somewhere():
    assert set(APPLIES) == set(go.VARIANTS) - {None} and all(APPLIES.values())


def test_a_camera_that_misses_has_an_exactly_zero_gradient():
    ref = go.reference("miss_5x7_s12_relu_white")
    assert bool((ref.g64 == 0).all()) and bool((go.hand_rule(ref.case, ref.ups, torch.float32) == 0).all())
    assert go.measure(ref.g64, ref.g64) == (0.0, 0.0) and ref.bar == (go.FLOOR, go.FLOOR)


@pytest.mark.parametrize("which", ["rgb", "depth", "opacity"])
def test_each_output_alone(which):
    """a None upstream is a zero upstream, in the yardstick and in the hand rule"""
    for name in ("inside_16_s12_relu_last_white", "outside_16_s12_softplus_last"):
        ref = go.reference(name, 1, (which,))
        assert sum(u is not None for u in ref.ups) == 1
        hand = go.hand_rule(ref.case, ref.ups)
        if which == "opacity" and ref.case.clamp_mode == 'softplus':
            # opacity is 1 whatever the nodes are (the last alpha is exactly 1): what is left of its gradient is the 1e-10 of
            # 1 - alpha + 1e-10 times rounding, in the yardstick and in the hand rule alike
            assert float(ref.g64.abs().max()) < 1e-8 and float(hand.abs().max()) < 1e-8
            continue
        assert float(ref.g64.abs().max()) > 1e-3
        m = go.measure(hand, ref.g64)
        assert m[0] <= 1e-9 and m[1] <= 1e-9
