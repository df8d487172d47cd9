"""CPU: the yardstick of the baked-volume renderer's camera gradient (tests/volume_cam_grad_oracle.py) checked against itself —
its cases satisfy the cap on flagged pixels, the rule restated by hand agrees with torch autograd in fp64, the same rule in
fp32 arithmetic stays inside the bar, and six deliberately wrong rules leave the bar wherever they can show (and agree to
rounding where it is derived that they cannot).  Nothing here runs code of the library but the camera construction.

MEASURED (fp64 unless said): flagged pixels per camera 0 - 0.8 % (one or two of 256), never near a box face; hand rule against
autograd 0 ... 1.1e-15; bars 9.5e-7 ... 2.8e-4; the hand rule in fp32 at 0.12 - 0.17 of the bar; the wrong rules at 5 ... 9e5
bars where they can show and at most 3e-10 of a bar where they cannot."""
import pytest
import torch

import volume_cam_grad_oracle as co

CASES = list(co.all_cases())


@pytest.mark.parametrize("name", CASES)
def test_few_pixels_are_flagged(name):
    fl = co.named_flags(name)
    for i in range(fl.any.shape[0]):
        frac = float(fl.any[i].float().mean())
        print(f"{name} camera {i}: flagged {frac:.4f} (near {int(fl.near[i].sum())}, face {int(fl.face[i].sum())}, "
              f"zero {int(fl.zero[i].sum())})")
        assert frac <= co.CAP
    ups = co.named_upstreams(name)
    assert all(bool((u[fl.any.unsqueeze(1).expand_as(u)] == 0).all()) for u in ups)


@pytest.mark.parametrize("name", CASES)
def test_the_yardstick_is_well_formed_and_the_hand_rule_agrees(name):
    ref = co.reference(name)
    g64 = ref.g64
    assert g64.dtype == torch.float64 and g64.shape == (ref.case.cam2world.shape[0], 4, 4)
    assert bool(torch.isfinite(g64).all()) and bool((g64[:, 3] == 0).all())
    if name.startswith(("miss", "nonpositive_16")):         # nothing is seen / relu clamps every sample and nothing tops up
        assert bool((g64 == 0).all())
    else:
        assert all(float(g64[i].abs().max()) > 1.0 for i in range(g64.shape[0]))
    hand = co.hand_rule(ref.case, ref.ups)
    m = co.measure(hand, g64)
    print(f"{name}: hand rule against autograd {m}, bar {ref.bar}")
    assert max(m) <= 1e-9 and bool((hand[:, 3] == 0).all())
    assert all(v >= co.FLOOR for v in ref.bar) and all(v < 1e-3 for v in ref.bar)
    m32 = co.measure(co.hand_rule(ref.case, ref.ups, torch.float32), g64)
    print(f"{name}: hand rule in fp32 / bar {[a / b for a, b in zip(m32, ref.bar)]}")
    assert co.within(m32, ref.bar)


@pytest.mark.parametrize("which", ["rgb", "depth", "opacity"])
def test_each_upstream_alone(which):
    ref = co.reference("inside_16_s12_relu_last_white", 1, (which,))
    m = co.measure(co.hand_rule(ref.case, ref.ups), ref.g64)
    assert max(m) <= 1e-9 and float(ref.g64.abs().max()) > 1e-3


@pytest.mark.parametrize("variant", co.VARIANTS[1:])
def test_wrong_rules_leave_the_bar_where_they_can_show(variant):
    shown = 0
    for name in CASES:
        ref = co.reference(name)
        m = co.measure(co.hand_rule(ref.case, ref.ups, variant=variant), ref.g64)
        can = co.can_show(ref.case, ref.ups, variant)
        for i, (mi, bi, ci) in enumerate(zip(m, ref.bar, can)):
            if ci:
                shown += 1
                assert mi > bi, (name, i, mi, bi)
            elif not (variant == "no_top_up" and ref.case.last_back):
                # derived: the wrong rule's extra or missing term is zero here, so the two rules are the same sums
                assert mi <= 1e-9, (name, i, mi)
    assert shown >= 2
