"""CPU: the drop-in discriminator reproduces the reference's initial state_dict bit-for-bit, and the
oracle's discriminator restatement is pinned to the golden vectors minted from the reference
(forward logits, R1 gradient w.r.t. the input, loss)."""
import pytest
import torch

from conftest import load_golden, load_gates, check_checksums, max_rel, D_CFG, ReplayDraws
from oracle import cips3d_oracle as orc


def seeded_discriminator(seed, diffaug=False):
    from cips3d_amd.discriminator import Discriminator_MultiScale_Aux
    torch.manual_seed(seed)
    return Discriminator_MultiScale_Aux(**dict(D_CFG, diffaug=diffaug))


def test_diffaugment_matches_reference_golden():
    """DiffAugment: the oracle's restatement gives the reference's output and input gradient under
    the reference's recorded draws (incl. its cutout ratio 0.2).  The product's DiffAugment is the HIP operator: its
    check against the same vectors is the GPU test test_diffaugment_hip_operator_matches_reference_golden."""
    for c in load_golden("diffaug_cases"):
        x = c["x"].clone().requires_grad_(True)
        y = orc.diff_augment(x, iter(t for _, t in c["draws"]), c["policy"])
        assert torch.equal(y, c["y"])
        gx, = torch.autograd.grad((y * c["g0"]).sum(), x)
        assert max_rel(gx, c["gx"]) < 1e-6


def test_diffaugment_product_has_no_torch_restatement():
    """The product's DiffAugment is the fused HIP operator only (round-2 verdict: the op-by-op torch path was a renamed
    copy of the reference's diffaug.py): no CPU path, no per-stage torch functions, policies checked."""
    import inspect
    from cips3d_amd import discriminator as dm
    src = inspect.getsource(dm)
    for name in ("_rand_brightness", "_rand_saturation", "_rand_contrast", "_rand_translation", "_rand_cutout", "_AUGMENT_FNS",
                 "meshgrid"):
        assert name not in src, name
    with pytest.raises(RuntimeError):
        dm.DiffAugment(torch.zeros(1, 3, 8, 8), policy="color")           # CPU tensor
    with pytest.raises(ValueError):
        dm.DiffAugment(torch.zeros(1, 3, 8, 8), policy="cutout,colour")   # unknown stage name
    with pytest.raises(RuntimeError):
        dm.DiffAugment(torch.zeros(1, 3, 8, 8), policy="cutout,color")    # any order of known stages is a policy; CPU is not
    assert dm.DiffAugment(torch.zeros(1, 3, 8, 8), policy="") is not None


@pytest.mark.parametrize("tag", ["d_r16", "d_r16_aux_alpha", "d_r16_diffaug"])
def test_discriminator_oracle_matches_reference(tag):
    fix = load_golden(tag)
    D = seeded_discriminator(fix["seed"], diffaug=fix.get("diffaug", False))
    check_checksums(D.state_dict(), fix["state_checksums"])
    assert sum(p.numel() for p in D.parameters()) == 37518914
    sd = dict(D.state_dict())
    sd.update(dict(D.named_parameters()))
    x = fix["x"].clone().requires_grad_(True)
    out = orc.discriminator_forward(sd, x, alpha=fix["alpha"], use_aux_disc=fix["use_aux"],
                                    draws=[t for _, t in fix["draws"]] if fix.get("diffaug") else None)
    assert max_rel(out, fix["out"]) < 1e-5
    g, = torch.autograd.grad(out.sum(), x, create_graph=True)
    assert max_rel(g, fix["grad_real"]) < 1e-4
    loss = torch.nn.functional.softplus(-out).mean() + 0.5 * 10. * g.flatten(1).pow(2).sum(1).mean()
    assert abs(float(loss) - fix["loss"]) < 1e-5 * max(1.0, abs(fix["loss"]))


def d_loss_grads(fix, dtype, tape):
    """full d_loss of train.py:385-409 (logits, R1 penalty through the double-backward graph) on the oracle -> logits,
    grad_real, {name: parameter gradient}"""
    D = seeded_discriminator(fix["seed"], diffaug=fix.get("diffaug", False))
    if dtype == torch.float64:
        D = D.double()
    sd = dict(D.state_dict())
    sd.update(dict(D.named_parameters()))
    x = fix["x"].to(dtype).clone().requires_grad_(True)
    draws = [t.to(dtype) if torch.is_floating_point(t) else t for _, t in fix["draws"]] if fix.get("diffaug") else None
    torch.set_default_dtype(dtype)
    try:
        with orc.gate_tape(tape):
            out = orc.discriminator_forward(sd, x, alpha=fix["alpha"], use_aux_disc=fix["use_aux"], draws=draws)
        g, = torch.autograd.grad(out.sum(), x, create_graph=True)
        loss = torch.nn.functional.softplus(-out).mean() + 0.5 * 10. * g.flatten(1).pow(2).sum(1).mean()
        loss.backward()
    finally:
        torch.set_default_dtype(torch.float32)
    return out.detach(), g.detach(), {n: p.grad for n, p in D.named_parameters()}


@pytest.mark.parametrize("tag", ["d_r16", "d_r16_aux_alpha", "d_r16_diffaug"])
def test_discriminator_oracle_gates_pinned(tag):
    """With the reference's LeakyReLU gates pinned (tests/golden/gates_*.pt), the oracle's R1 input gradient and the
    parameter gradients of the full d_loss equal the reference's to fp32 rounding — in fp32 and in fp64 (the GPU
    tests' yardstick): no gate allowance."""
    fix = load_golden(tag)
    gates = load_gates(tag)
    free = orc.GateTape()
    d_loss_grads(fix, torch.float32, free)
    flips = sum(int((a != b).sum()) for a, b in zip(free.rec, gates))
    total = sum(g.numel() for g in gates)
    print(f"{tag}: oracle fp32 vs reference fp32: {flips} of {total} gates differ")
    assert len(free.rec) == len(gates) and flips <= 2
    for dtype in (torch.float32, torch.float64):
        tape = orc.GateTape(pin=gates)
        out, g, grads = d_loss_grads(fix, dtype, tape)
        tape.done()
        assert max_rel(out.float(), fix["out"]) < 1e-5
        assert max_rel(g.float(), fix["grad_real"]) < 1e-4
        worst = 0.0
        for name, gr in grads.items():
            dg = fix["grads"][name]
            if dg is None:
                assert gr is None or float(gr.abs().max()) == 0.0, name
                continue
            v = gr.reshape(-1).double()
            got = v[::dg["stride"]] if dg["stride"] > 1 else v
            e = float((got - dg["sample"].double()).norm() / dg["sample"].double().norm().clamp_min(1e-300))
            worst = max(worst, e)
            assert e < 1e-4 and abs(float(v.norm()) - dg["norm"]) <= 1e-4 * dg["norm"], (name, e)
        print(f"{tag}: {dtype} oracle, reference gates pinned: worst parameter-gradient error {worst:.2e}")


D_SLICE_FP64_BAR = 1e-12         # fp64 rounding over the sums of a gradient (eps 1.1e-16 x their length), 10x the ~1e-13 expected
D_SLICE_FP32_BAR = None          # set below the test: 4 x the largest fp32 parameter-gradient difference measured


def test_discriminator_oracle_is_additive_over_batch_slices():
    """What the GPU tests at the training batches stand on (test_gpu_real_configs.py, the *_vs_sliced_oracle tests): nothing in
    Discriminator_MultiScale_Aux couples the images of a batch (stddev_group = 0), so with the loss written as sums over the
    images — softplus(-out).sum() / n + 5 * |dout/dx|^2.sum() / n — the oracle's logits and R1 input gradient on a batch are
    the concatenation, and its parameter gradients the sum, over slices [i, n/2 + i] (image i of the main network's half and
    of the auxiliary network's half).  32 x 32, 2 + 2 images, fade-in alpha 0.6, whole against two slices of 1 + 1:
      fp64, nothing pinned:                          logits 1.3e-15, R1 input gradient 0, worst parameter gradient
                                                     1.5e-15 (relative): the identity, at rounding level;
      fp32, the whole run's gates pinned in slices:  logits 8.9e-07, R1 input gradient 9.7e-07, worst parameter gradient
                                                     8.5e-07 (main_disc.convs.32.conv1.equal_conv.weight); bar 4 x that, 3.4e-06.
    A gate that differs between the whole and the free-running sliced fp32 run is the discontinuity of DESIGN.md §0 (a
    pre-activation within rounding of 0), not a slicing error: they are counted and printed (0 here)."""
    F = torch.nn.functional
    size, b, alpha = 32, 2, 0.6
    n = 2 * b
    g = torch.Generator().manual_seed(3232)
    x0 = torch.rand(n, 3, size, size, generator=g) * 2 - 1

    def run(dtype, rows, pin=None, grad=True):
        D = seeded_discriminator(4321)
        if dtype == torch.float64:
            D = D.double()
        sd = dict(D.state_dict())
        sd.update(dict(D.named_parameters()))
        x = x0[rows].to(dtype).clone().requires_grad_(grad)
        tape = orc.GateTape(pin=pin)
        torch.set_default_dtype(dtype)
        try:
            with orc.gate_tape(tape), torch.set_grad_enabled(grad):
                out = orc.discriminator_forward(sd, x, alpha=alpha, use_aux_disc=True)
            if not grad:
                return tape.rec
            gr, = torch.autograd.grad(out.sum(), x, create_graph=True)
            (F.softplus(-out).sum() / n + 0.5 * 10. * gr.flatten(1).pow(2).sum() / n).backward()
        finally:
            torch.set_default_dtype(torch.float32)
        tape.done()
        return out.detach(), gr.detach(), {k: p.grad.double() for k, p in D.named_parameters() if p.grad is not None}, tape.rec

    slices = [torch.tensor([i, b + i]) for i in range(b)]
    for dtype in (torch.float64, torch.float32):
        out, gr, grads, gates = run(dtype, torch.arange(n))
        assert all(t.shape[0] == b for t in gates)
        s_out, s_gr, s_grads, flips = torch.empty_like(out), torch.empty_like(gr), {}, 0
        for i, rows in enumerate(slices):
            pin = None
            if dtype == torch.float32:
                free = run(dtype, rows, grad=False)
                flips += sum(int((a != w[i:i + 1]).sum()) for a, w in zip(free, gates))
                pin = [w[i:i + 1] for w in gates]
            o, g_, gs, _ = run(dtype, rows, pin=pin)
            s_out[rows], s_gr[rows] = o, g_
            for k, v in gs.items():
                s_grads[k] = v if k not in s_grads else s_grads[k] + v
        assert set(s_grads) == set(grads) and len(grads) == 50          # every parameter the 32 x 32 pass reaches
        errs = {k: float((s_grads[k] - v).norm() / v.norm().clamp_min(1e-300)) for k, v in grads.items()}
        wk = max(errs, key=errs.get)
        e_out, e_gr = max_rel(s_out, out), max_rel(s_gr, gr)
        print(f"D oracle whole vs sliced, {dtype}: logits {e_out:.2e}, R1 input gradient {e_gr:.2e}, worst parameter gradient "
              f"{errs[wk]:.2e} ({wk})" + (f"; {flips} of {sum(t.numel() for t in gates)} gates differ free-running" if dtype == torch.float32 else ""))
        bar = D_SLICE_FP64_BAR if dtype == torch.float64 else D_SLICE_FP32_BAR
        assert e_out < bar and e_gr < bar and errs[wk] < bar, (dtype, e_out, e_gr, wk, errs[wk])


D_SLICE_FP32_BAR = 4 * 8.5e-7


def test_conv_dispatch_rule_over_the_shipped_discriminator(monkeypatch):
    """_conv_forms — the one rule that the convolution functions, the planes-only gradient and the conv + activation fusion
    consult — over every convolution of Discriminator_MultiScale (channel_multiplier 2, with and without the stddev channel
    in front of the final convolution) at input sizes 16 ... 1024 and batches 1 ... 32: the conv_in layers take the streaming
    RGB kernels, everything else the implicit-GEMM family (the data gradient of a 3 x 3 stride-2 convolution behind its Blur
    as parity sub-convolutions), and the exact fp32 form is met at the 513-channel final convolution only.  The layer list is
    the module's own (_conv_layers + conv_in); shapes and the folded Blur are derived from the ConvLayers as ConvLayer.forward
    does.  Also: the weight gradient the rule calls "implicit" is declined by ops.conv2d_x3_wgrad exactly where the batch's
    pixel count B * N is no multiple of 32 — restated here from the shapes: the 4 x 4 output planes at odd B."""
    import math
    from cips3d_amd import discriminator as dm
    from cips3d_amd import ops
    assert dm.CONV_MODE == "bf16x3" and dm.FOLD_BLUR
    monkeypatch.setattr(torch, "randn", torch.empty)           # only shapes are read: 37 M parameters stay uninitialised

    def call_of(layer, h):
        """(input shape without the batch, stride, pad, pre) of the convolution call ConvLayer.forward makes on an h x h map"""
        conv, blur = layer.equal_conv, getattr(layer, "down_blur", None)
        c = conv.weight.shape[1]
        if blur is None:
            return (c, h, h), conv.stride, conv.padding, None
        if conv.weight.shape[2] == 1:                          # the skip branch: Blur sampled at stride 2, 1 x 1 at stride 1
            return (c, h, h), 1, 0, (None, blur.pad[0], blur.pad[1], 2)
        return (c, h, h), conv.stride, conv.padding, (None, blur.pad[0], blur.pad[1], 1)

    seen_f32, declined, n_layers = set(), set(), 0
    for stddev_group in (0, 4):
        D = dm.Discriminator_MultiScale(diffaug=False, max_size=1024, channel_multiplier=2, stddev_group=stddev_group)
        c_final = D.final_conv.equal_conv.weight.shape[1]
        assert c_final == (513 if stddev_group else 512)
        for size in (16, 32, 64, 128, 256, 512, 1024):
            log_size = int(math.log2(size))
            listed = D._conv_layers(log_size)
            calls = []                                         # (EqualConv2d, call, expected forms)
            for i in range(log_size, 2, -1):
                blk, h = D.convs[f"{2 ** i}"], 2 ** i
                for layer, h_in in ((blk.conv1, h), (blk.conv2, h // 2 if hasattr(blk.conv1, "down_blur") else h), (blk.skip, h)):
                    call = call_of(layer, h_in)
                    parity = call[3] is not None and layer.equal_conv.weight.shape[2] == 3
                    assert parity or call[1] == 1              # stride 1, or a 3 x 3 stride-2 convolution behind its Blur
                    calls.append((layer.equal_conv, call, ("implicit", "parity" if parity else "implicit", "implicit")))
            calls.append((D.final_conv.equal_conv, call_of(D.final_conv, 4), ("f32",) * 3 if c_final == 513 else ("implicit",) * 3))
            assert [c for c, _ in listed] == [c for c, _, _ in calls]
            for (conv, alt), (_, _, want) in zip(listed, calls):             # the weight form prepared for the data gradient
                assert alt == ("s2banks" if want[1] == "parity" else "flipT")
            conv_in = D.conv_in[f"{size}"].equal_conv
            calls.append((conv_in, call_of(D.conv_in[f"{size}"], size), ("rgb",) * 3))
            for conv, ((c, h, w), stride, pad, pre), want in calls:
                hb, wb = dm._pre_shape(h, w, pre)
                kh = conv.weight.shape[2]
                n = ((hb + 2 * pad - kh) // stride + 1) ** 2
                for B in range(1, 33):
                    got = dm._conv_forms((B, c, h, w), tuple(conv.weight.shape), stride, pad, pre)
                    assert got == want, (size, B, tuple(conv.weight.shape), stride, pad, got, want)
                    n_layers += 1
                    if "f32" in got:
                        seen_f32.add(c)
                    if got[2] == "implicit":
                        declines = (B * n) % 32 != 0
                        assert ops.conv2d_x3_wgrad_declines(B, n) == declines
                        if declines:
                            declined.add((n, B))
    assert seen_f32 == {513}
    assert declined == {(16, B) for B in range(1, 33, 2)}
    assert n_layers == 2 * 32 * sum(3 * (ls - 2) + 2 for ls in range(4, 11))
    # CONV_MODE "f32": no split-bf16 form anywhere, the RGB kernels stay
    monkeypatch.setattr(dm, "CONV_MODE", "f32")
    assert dm._conv_forms((4, 512, 8, 8), (512, 512, 3, 3), 1, 1) == ("f32",) * 3
    assert dm._conv_forms((4, 512, 9, 9), (512, 512, 3, 3), 2, 0, (None, 2, 2, 1)) == ("f32",) * 3
    assert dm._conv_forms((4, 3, 8, 8), (512, 3, 1, 1), 1, 0) == ("rgb",) * 3
    monkeypatch.setattr(dm, "CONV_MODE", "bf16x3")
    # shapes outside the networks that the removed split-bf16 im2col forms used to take are exact fp32 now
    assert dm._conv_forms((2, 64, 17, 17), (32, 64, 3, 3), 2, 0)[1] == "f32"          # a stride-2 data gradient without a Blur
    assert dm._conv_forms((2, 48, 16, 16), (64, 48, 2, 2), 1, 0) == ("f32",) * 3      # channels that are no multiple of 32
    assert dm._conv_forms((2, 64, 17, 17), (32, 64, 3, 3), 2, 0, (None, 2, 2, 1))[1] == "f32"   # O = 32 behind a Blur: one k-tile
