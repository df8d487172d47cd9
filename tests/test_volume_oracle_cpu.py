"""CPU: the yardstick of the baked-volume renderer (tests/volume_oracle.py) held to itself.  Its per-pixel error bar is derived
from fp32 eps, not from any kernel; this file shows that the bar means something.  On every case the GPU test uses:
  - the same rule in fp32 torch arithmetic stays within the bar on every pixel that is not `near`,
  - three deliberately wrong rules (nearest node instead of trilinear, depths shifted by one sample, x and z axes of the volume
    swapped) each leave the bar on more than half of the pixels that see the volume,
  - a fourth, last_back's top-up dropped from the colour, leaves it on every pixel whose top-up is larger than twice the bar, and
    the relu cases have such pixels by the dozen: the bar is not vacuous where the last delta = 1e10 meets a negative sigma,
  - `near` (a sample within the position bar of a box face, where fp32 may decide the inside test the other way) flags at most
    2 % of the pixels: the cases are three-quarter views whose ray_start lies on no face."""
import pytest
import torch

import volume_oracle as vo

CASES = vo.cases()


@pytest.mark.parametrize("name", list(CASES))
def test_the_rule_in_fp32_stays_within_the_bar(name):
    ref = vo.reference(name)
    got = vo.render(CASES[name], dtype=torch.float32)
    assert got.rgb.dtype == torch.float32
    q = vo.compare(ref, got.rgb, got.depth, got.opacity)
    print(f"{name}: fp32 torch at rgb {q.rgb:.4f}, depth {q.depth:.4f}, opacity {q.opacity:.4f} of the bar")
    assert max(q.rgb, q.depth, q.opacity) <= 1
    assert torch.equal(got.sees, ref.sees) or bool((got.sees != ref.sees).sum() <= ref.near.sum())


@pytest.mark.parametrize("variant", ["nearest", "shift", "swap_xz"])
@pytest.mark.parametrize("name", list(CASES))
def test_a_wrong_rule_leaves_the_bar(name, variant):
    ref = vo.reference(name)
    sees = ref.sees & ~ref.near
    if name.startswith("miss"):
        assert int(ref.sees.sum()) == 0                      # nothing to tell apart: every ray misses the box
        return
    assert int(sees.sum()) >= 8
    got = vo.render(CASES[name], variant=variant)
    q = vo.compare(ref, got.rgb, got.depth, got.opacity)
    share = float((q.over & sees).sum()) / float(sees.sum())
    print(f"{name} / {variant}: outside the bar on {share:.3f} of the {int(sees.sum())} pixels that see the volume")
    assert share > 0.5


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.last_back and c.clamp_mode == "relu"])
def test_a_dropped_top_up_leaves_the_bar(name):
    """Under relu a last sample with sigma below -e_sigma is clamped for certain: its alpha carries no error however large the
    last delta is.  A bar that forgot that would swallow the whole top-up 1 - sum w."""
    case, ref = CASES[name], vo.reference(name)
    got = vo.render(case, variant="no_top_up")
    top_up = (ref.rgb - got.rgb).abs()                                       # |1 - sum w| |c_last| per channel, from the oracle alone
    large = ((top_up > 2 * ref.bar_rgb).any(1)) & ~ref.near
    q = vo.compare(ref, got.rgb, got.depth, got.opacity)
    print(f"{name}: the top-up exceeds twice the bar on {int(large.sum())} of {large.numel()} pixels (largest {float(top_up.max()):.3f}); "
          f"largest bar_rgb {float(ref.bar_rgb.max()):.2e}, bar_opacity {float(ref.bar_opacity.max()):.2e}")
    if name.startswith(("corner", "inside_16_s12_relu_last_smooth")):        # the last sample lies inside the box on many rays
        assert int(large.sum()) >= 48
        assert int((top_up.amax(1) > 0.1).sum()) >= 48 and bool(large[top_up.amax(1) > 0.1].all())
    assert bool(q.over[large].all())


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.clamp_mode == "relu"])
def test_relu_bars_are_not_vacuous(name):
    """no relu case has a pixel whose opacity bar is a visible share of the whole range"""
    ref = vo.reference(name)
    print(f"{name}: largest bar_opacity {float(ref.bar_opacity.max()):.2e}")
    assert float(ref.bar_opacity.max()) <= 0.05


@pytest.mark.parametrize("name", list(CASES))
def test_few_pixels_are_near_a_face(name):
    ref = vo.reference(name)
    share = float(ref.near.sum()) / ref.near.numel()
    print(f"{name}: {int(ref.near.sum())} of {ref.near.numel()} pixels near a face; {int(ref.sees.sum())} see the volume")
    assert share <= 0.02


def test_the_cases_cover_what_they_claim():
    """outside: most pixels see the volume; inside: all do, from the first sample on; corner: some do and some do not"""
    sees = {name: vo.reference(name).sees for name in CASES}
    assert all(bool(sees[n].all()) for n in CASES if n.startswith("inside"))
    assert all(0 < int(sees[n].sum()) < sees[n].numel() for n in CASES if n.startswith("corner"))
    assert all(int(sees[n].sum()) > sees[n].numel() // 2 for n in CASES if n.startswith(("outside", "turntable", "pairs")))
    assert {(c.H, c.W) for c in CASES.values()} == {(5, 7), (16, 16)} and {c.S for c in CASES.values()} == {2, 12}
    for flag in ("last_back", "white_back"):
        assert {getattr(c, flag) for c in CASES.values()} == {False, True}
    assert {c.clamp_mode for c in CASES.values()} == {"relu", "softplus"}
    assert {(c.sigma.shape[0], c.cam2world.shape[0]) for c in CASES.values()} == {(1, 1), (1, 3), (2, 2)}


def test_all_nonpositive_volume_renders_nothing():
    case = CASES["outside_5x7_s12_relu"]
    empty = vo.make_case(-case.sigma.abs(), case.rgb, case.cam2world, 24, 5, 7, 0.8, 1.2, 12)
    got = vo.render(empty)
    assert bool((got.opacity == 0).all()) and bool((got.depth == 0).all()) and bool((got.rgb == 0).all())
