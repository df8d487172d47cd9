"""CPU: CIPS_D_CONV_MODE=bf16 over the shipped discriminator — the walk of
test_discriminator_cpu.test_conv_dispatch_rule_over_the_shipped_discriminator (its helper re-stated here), asking what the
single-pass mode adds to the dispatch rule: nothing to the form names, and one shape predicate, _single_pass."""
import math

import pytest
import torch


def _call_of(layer, h):
    """(input shape without the batch, stride, pad, pre) of the convolution call ConvLayer.forward makes on an h x h map"""
    conv, blur = layer.equal_conv, getattr(layer, "down_blur", None)
    c = conv.weight.shape[1]
    if blur is None:
        return (c, h, h), conv.stride, conv.padding, None
    if conv.weight.shape[2] == 1:                          # the skip branch: Blur sampled at stride 2, 1 x 1 at stride 1
        return (c, h, h), 1, 0, (None, blur.pad[0], blur.pad[1], 2)
    return (c, h, h), conv.stride, conv.padding, (None, blur.pad[0], blur.pad[1], 1)


def _walk(dm):
    """every convolution call of Discriminator_MultiScale (with and without the stddev channel) at input sizes 16 ... 1024:
    (size, weight shape, (c, h, w), stride, pad, pre)"""
    for stddev_group in (0, 4):
        D = dm.Discriminator_MultiScale(diffaug=False, max_size=1024, channel_multiplier=2, stddev_group=stddev_group)
        for size in (16, 32, 64, 128, 256, 512, 1024):
            log_size = int(math.log2(size))
            calls = []
            for i in range(log_size, 2, -1):
                blk, h = D.convs[f"{2 ** i}"], 2 ** i
                for layer, h_in in ((blk.conv1, h), (blk.conv2, h // 2 if hasattr(blk.conv1, "down_blur") else h), (blk.skip, h)):
                    calls.append((layer.equal_conv, _call_of(layer, h_in)))
            calls.append((D.final_conv.equal_conv, _call_of(D.final_conv, 4)))
            calls.append((D.conv_in[f"{size}"].equal_conv, _call_of(D.conv_in[f"{size}"], size)))
            for conv, (chw, stride, pad, pre) in calls:
                yield size, tuple(conv.weight.shape), chw, stride, pad, pre


def test_bf16_mode_over_the_shipped_discriminator(monkeypatch):
    """In mode "bf16" the three form names are those of "bf16x3" for every convolution, size and batch.  _single_pass — shapes
    only, the same answer in every mode — is true for the forward and the data gradient of every "implicit" / "parity"
    convolution of the shipped channel table whose contraction the 64-deep k-tiles fit: 64-channel multiples, 128 long at
    least.  The shipped table has exactly three kinds of convolution that do not fit, all in the 512 and 1024 blocks (none
    at the training sizes up to 256): the 32-channel layers of the 1024 block (forward C = 32; data gradients over O = 32 and,
    in the parity form, O = 64), and the 1 x 1 skip convolution with 64 input channels (one 64-deep k-tile forward) — listed
    below and compared as a set.  They run 3-pass in "bf16" mode.  For weight gradients _single_pass is true exactly where
    ops.conv2d_bf16_wgrad_declines is false."""
    from cips3d_amd import discriminator as dm
    from cips3d_amd import ops
    assert dm.CONV_MODE == "bf16x3" and dm.FOLD_BLUR
    monkeypatch.setattr(torch, "randn", torch.empty)           # only shapes are read: 37 M parameters stay uninitialised
    calls = list(_walk(dm))
    assert len(calls) == 2 * sum(3 * (ls - 2) + 2 for ls in range(4, 11))
    not_fwd, not_dgrad, n_wgrad_single, n_checked = set(), set(), 0, 0
    for size, w_shape, (c, h, w), stride, pad, pre in calls:
        O, _, kh, kw = w_shape
        hb, wb = dm._pre_shape(h, w, pre)
        n = ((hb + 2 * pad - kh) // stride + 1) ** 2
        for B in range(1, 33):
            args = ((B, c, h, w), w_shape, stride, pad, pre)
            monkeypatch.setattr(dm, "CONV_MODE", "bf16x3")
            x3_forms, x3_single = dm._conv_forms(*args), dm._single_pass(*args)
            monkeypatch.setattr(dm, "CONV_MODE", "bf16")
            forms, single = dm._conv_forms(*args), dm._single_pass(*args)
            assert forms == x3_forms and single == x3_single, (size, B, w_shape)
            assert all(isinstance(s, bool) for s in single)
            n_checked += 1
            if forms[0] == "implicit" and not single[0]:
                not_fwd.add((size, c, O, kh))
            if forms[1] in ("implicit", "parity") and not single[1]:
                not_dgrad.add((size, c, O, kh, forms[1]))
            if forms[0] == "implicit":
                assert single[0] == (c % 64 == 0 and kh * kw * c >= 128)
            if forms[1] == "parity":
                assert single[1] == (O % 64 == 0 and O >= 128)
            if forms[1] == "implicit":
                assert single[1] == (O % 64 == 0 and kh * kw * O >= 128)
            if forms[2] == "implicit":
                assert single[2] == (not ops.conv2d_bf16_wgrad_declines(B, n)), (size, B, w_shape)
                assert single[2] == ((B * n) % 64 == 0 and B * n >= 128)
                n_wgrad_single += single[2]
                if single[2]:
                    assert not ops.conv2d_x3_wgrad_declines(B, n)       # what the single pass takes, the 3-pass form takes too
    monkeypatch.setattr(dm, "CONV_MODE", "bf16x3")
    assert n_checked == 32 * len(calls) and n_wgrad_single > 0
    # every implicit / parity forward and data gradient of the shipped channel table is single-pass, except:
    assert not_fwd == {(1024, 32, 32, 3), (1024, 32, 64, 3), (1024, 32, 64, 1),        # the 1024 block: 32 input channels
                       (512, 64, 128, 1), (1024, 64, 128, 1)}                           # 1 x 1 on 64 channels: K = 64, one k-tile
    assert not_dgrad == {(1024, 32, 32, 3, "implicit"), (1024, 32, 64, 3, "parity"), (1024, 32, 64, 1, "implicit")}
    # ... none of them at the training sizes
    assert all(k[0] >= 512 for k in not_fwd | not_dgrad)
    # _planes_only_ok's premise holds in "bf16" mode: a weight gradient the single-pass kernel declines is the 3-pass kernel's
    # wherever that does not decline either — both consumers of a planes-only gradient still read planes
    assert ops.conv2d_bf16_wgrad_declines(6, 16) and not ops.conv2d_x3_wgrad_declines(6, 16)
    assert ops.conv2d_bf16_wgrad_declines(4, 16) and not ops.conv2d_bf16_wgrad_declines(8, 16)


def test_bf16_mode_keeps_rgb_and_f32_forms_and_prepares_the_same_planes(monkeypatch):
    from cips3d_amd import discriminator as dm
    monkeypatch.setattr(dm, "CONV_MODE", "bf16")
    assert dm._conv_forms((4, 3, 8, 8), (512, 3, 1, 1), 1, 0) == ("rgb",) * 3
    assert dm._conv_forms((4, 513, 4, 4), (512, 513, 3, 3), 1, 1) == ("f32",) * 3
    assert dm._conv_forms((4, 512, 8, 8), (512, 512, 3, 3), 1, 1) == ("implicit",) * 3
    assert dm._conv_forms((4, 512, 9, 9), (512, 512, 3, 3), 2, 0, (None, 2, 2, 1)) == ("implicit", "parity", "implicit")
    # eligibility is the shape's, not the mode's
    assert dm._single_pass((4, 512, 8, 8), (512, 512, 3, 3), 1, 1) == (True, True, True)
    assert dm._single_pass((1, 512, 8, 8), (512, 512, 3, 3), 1, 1) == (True, True, False)        # 64 pixels: one k-tile
    assert dm._single_pass((2, 32, 16, 16), (64, 32, 3, 3), 1, 1) == (False, True, True)
    assert dm._single_pass((2, 64, 17, 17), (64, 64, 3, 3), 2, 0, (None, 0, 0, 1))[1] is False    # O = 64 behind a Blur


def test_an_unknown_mode_string_raises(monkeypatch):
    """only "bf16x3", "f32" and "bf16" are values: anything else used to select exact fp32 silently"""
    from cips3d_amd import discriminator as dm
    assert dm.CONV_MODES == ("bf16x3", "f32", "bf16")
    for bad in ("bf16x2", "BF16", "", "fp32", None):
        monkeypatch.setattr(dm, "CONV_MODE", bad)
        with pytest.raises(ValueError):
            dm._conv_forms((4, 512, 8, 8), (512, 512, 3, 3), 1, 1)
        with pytest.raises(ValueError):
            dm.prepare_weight_planes([])
    for good in dm.CONV_MODES:
        monkeypatch.setattr(dm, "CONV_MODE", good)
        dm._conv_forms((4, 512, 8, 8), (512, 512, 3, 3), 1, 1)


def test_an_unknown_mode_in_the_environment_raises_at_import():
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, CIPS_D_CONV_MODE="bf16x2")
    r = subprocess.run([sys.executable, "-c", "import cips3d_amd.discriminator"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "CIPS_D_CONV_MODE" in r.stderr
