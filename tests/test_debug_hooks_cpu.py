"""The four pin / record hooks (ops.gate_debug, ops.clamp_debug, ops.resample_debug, discriminator.gate_debug) are
instances of one class: what a `with hook(pin=..., rec=...)` block sets, restores and asserts.  No GPU."""
import pytest
import torch

from cips3d_amd import discriminator, ops

HOOKS = {"ops.gate_debug": ops.gate_debug, "ops.clamp_debug": ops.clamp_debug, "ops.resample_debug": ops.resample_debug,
         "discriminator.gate_debug": discriminator.gate_debug}
GATES = ["ops.gate_debug", "discriminator.gate_debug"]
OTHERS = ["ops.clamp_debug", "ops.resample_debug"]


def _idle(hook):
    return hook.pin is None and hook.rec is None


@pytest.mark.parametrize("name", sorted(HOOKS))
def test_nesting_restores_outer_pin_and_rec(name):
    hook = HOOKS[name]
    assert _idle(hook)
    outer_rec, inner_rec = [], []
    with hook(pin=[1, 2], rec=outer_rec):
        outer_pin = hook.pin
        assert next(hook.pin) == 1 and hook.rec is outer_rec
        with hook(pin=None, rec=inner_rec):
            assert hook.pin is None and hook.rec is inner_rec
        assert hook.pin is outer_pin and hook.rec is outer_rec
        with hook(pin=[7]):
            assert next(hook.pin) == 7 and hook.rec is None
        assert hook.pin is outer_pin and hook.rec is outer_rec
        assert next(hook.pin) == 2                       # the outer iterator went on where it was
    assert _idle(hook)


@pytest.mark.parametrize("name", GATES)
def test_gate_hooks_assert_leftover_pins_on_clean_exit_only(name):
    hook = HOOKS[name]
    with pytest.raises(AssertionError, match="left over"):
        with hook(pin=[1, 2]):
            next(hook.pin)
    assert _idle(hook)
    with hook(pin=[1]):                                  # every pin drawn: nothing to assert
        next(hook.pin)
    with hook(rec=[]):                                   # not pinned: nothing to assert
        pass
    with pytest.raises(KeyError):                        # the block's own exception, not the assertion
        with hook(pin=[1, 2]):
            raise KeyError("from the block")
    assert _idle(hook)


@pytest.mark.parametrize("name", OTHERS)
def test_clamp_and_resample_hooks_never_assert_leftovers(name):
    hook = HOOKS[name]
    with hook(pin=[1, 2, 3]):
        next(hook.pin)
    with hook(pin=[1]):
        pass
    assert _idle(hook)


def test_fine_z_debug_passes_records_and_pins():
    z = torch.arange(6.).reshape(2, 3).requires_grad_(True)
    assert ops.fine_z_debug(z) is z
    rec = []
    with ops.resample_debug(rec=rec):
        assert ops.fine_z_debug(z) is z
    assert len(rec) == 1 and torch.equal(rec[0], z) and rec[0] is not z and not rec[0].requires_grad
    assert rec[0].data_ptr() != z.data_ptr()
    pinned = torch.arange(6.) + 10
    with ops.resample_debug(pin=[pinned], rec=rec):
        out = ops.fine_z_debug(z)
    assert out is not z and out.shape == z.shape and torch.equal(out, pinned.reshape(2, 3))
    assert len(rec) == 2 and torch.equal(rec[1], z)      # what the forward drew is recorded, not what replaced it


def test_head_and_discriminator_gate_hooks_are_independent():
    assert ops.gate_debug is not discriminator.gate_debug
    rec = []
    with discriminator.gate_debug(pin=[1], rec=rec):
        assert _idle(ops.gate_debug)
        with ops.gate_debug(pin=[2], rec=[]):
            assert discriminator.gate_debug.rec is rec and next(discriminator.gate_debug.pin) == 1
            assert next(ops.gate_debug.pin) == 2
        assert _idle(ops.gate_debug) and discriminator.gate_debug.rec is rec
    with ops.gate_debug(rec=rec):
        assert _idle(discriminator.gate_debug)
    assert _idle(ops.gate_debug) and _idle(discriminator.gate_debug)
