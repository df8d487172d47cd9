"""CPU: the fp64 yardstick of the feature-volume renderer (tests/feature_volume_oracle.py) held to itself, before the GPU tests
hold the kernel to it.  The same rule in fp32 torch arithmetic stays inside the bars on every pixel that is not `near` a box
face; two deliberately wrong rules leave the bars on most pixels of at least one case; and no case hides behind `near`."""
import pytest
import torch

import feature_volume_oracle as fo

# the largest share of a case's pixels that may be `near` a box face (exempt from the bars).  The cameras are three-quarter
# views and no ray_start lies on a face, so a sample within a few fp32 roundings of a face is an accident of one pixel, not of a
# row: 2 % of a 16 x 16 image is five pixels, of a 5 x 7 image none.
NEAR_CAP = 0.02


@pytest.mark.parametrize("name", fo.NAMES)
def test_fp32_arithmetic_stays_inside_the_bars(name):
    ref = fo.reference(name)
    got = fo.render(fo.cases()[name], dtype=torch.float32)
    assert got.fea.shape == ref.fea.shape == (fo.cases()[name].cam2world.shape[0], ref.near.shape[1] * ref.near.shape[2], 32)
    q = fo.compare(ref, got.fea, got.depth, got.opacity)
    print(f"{name}: fea {q.fea:.4f}, depth {q.depth:.4f}, opacity {q.opacity:.4f} of the bar")
    assert q.fea <= 1 and q.depth <= 1 and q.opacity <= 1 and not bool(q.over.any())
    assert bool(torch.isfinite(ref.bar_fea).all()) and bool(torch.isfinite(ref.fea).all())


@pytest.mark.parametrize("name", fo.NAMES)
def test_few_pixels_are_near_a_face(name):
    near = fo.reference(name).near
    share = float(near.double().mean())
    print(f"{name}: {int(near.sum())} of {near.numel()} pixels near a face")
    assert share <= NEAR_CAP


def test_the_cases_cover_what_they_claim():
    c = fo.cases()
    assert set(fo.NAMES) <= set(c) and len(fo.NAMES) >= 9
    assert (c["outside_5x7_s12_relu"].H, c["outside_5x7_s12_relu"].W) == (5, 7)                  # partial tiles
    assert c["outside_16_s2_relu_white"].S == 2
    assert c["turntable_16_s12_relu"].cam2world.shape[0] == 3 and c["turntable_16_s12_relu"].feat.shape[0] == 1
    assert c["pairs_5x7_s12_softplus_last"].cam2world.shape[0] == 2 and c["pairs_5x7_s12_softplus_last"].feat.shape[0] == 2
    assert not bool(fo.reference("miss_5x7_s12_relu_white").sees.any())                         # a complete miss
    assert bool(fo.reference("inside_16_s12_relu_last_smooth").sees.all())                      # the camera inside the box
    for name in fo.NAMES:
        assert c[name].feat.shape[-1] == 32 and float(c[name].feat.abs().max()) <= 1


@pytest.mark.parametrize("variant", ["wrong_group", "top_up_3"])
def test_a_wrong_rule_leaves_the_bars(variant):
    shares = {}
    for name in fo.NAMES:
        ref = fo.reference(name)
        got = fo.render(fo.cases()[name], dtype=torch.float32, variant=variant)
        shares[name] = float(fo.compare(ref, got.fea, got.depth, got.opacity).over.double().mean())
    print(variant, {k: round(v, 3) for k, v in shares.items()})
    assert max(shares.values()) > 0.5
    if variant == "top_up_3":        # a rule that differs only in the top-ups is the right rule where there is none
        assert shares["outside_5x7_s12_relu"] == 0 and shares["turntable_16_s12_relu"] == 0
        assert shares["miss_5x7_s12_relu_white"] == 1       # 1 - sum w = 1 on every pixel, missing from channels 3..31
