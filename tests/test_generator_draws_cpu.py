"""CPU: the random draws of the generator's render path (cips3d_amd.generator.draw_randoms / draw_part_randoms) and the
freeze variants' mapping hooks.

The draws must reproduce the reference's calls, shapes and order in every mode, so that a same-device, same-seed run
consumes torch's generator as the reference does.  Each test records the torch.rand / randn /
randperm calls of one mode, compares them with the list the reference issues, replays that list from the same seed and
asks for the same tensors and the same generator state afterwards.  No library, no reference tree: pure torch."""
import contextlib
import math

import pytest
import torch

from cips3d_amd import generator, generator_v1
from cips3d_amd.generator import RenderSettings, draw_part_randoms, draw_randoms
from conftest import G_CFG

B, N, S = 2, 16, 4
CPU = torch.device("cpu")
_FNS = ("rand", "randn", "randperm")


def settings(**kw):
    return RenderSettings(**{**dict(img_size=4, fov=12, ray_start=0.88, ray_end=1.12, num_steps=S, h_stddev=0.3, v_stddev=0.155,
                                    h_mean=math.pi * 0.5, v_mean=math.pi * 0.5, hierarchical_sample=True,
                                    sample_dist="gaussian"), **kw})


@contextlib.contextmanager
def recorded():
    """-> the list of (name, shape) of every torch.rand / randn / randperm call made inside"""
    calls, orig = [], {name: getattr(torch, name) for name in _FNS}

    def wrap(name):
        def fn(*a, **k):
            calls.append((name, tuple(a[0]) if isinstance(a[0], (tuple, list, torch.Size)) else a))
            return orig[name](*a, **k)
        return fn

    for name in _FNS:
        setattr(torch, name, wrap(name))
    try:
        yield calls
    finally:
        for name in _FNS:
            setattr(torch, name, orig[name])


def run(fn, seed=1234):
    """fn() under the seed -> its result, the recorded calls, the generator state afterwards"""
    torch.manual_seed(seed)
    with recorded() as calls:
        out = fn()
    return out, calls, torch.get_rng_state()


def replay(calls, seed=1234):
    """the same calls inline from the same seed -> their tensors, the generator state afterwards"""
    torch.manual_seed(seed)
    return [getattr(torch, name)(*shape) for name, shape in calls], torch.get_rng_state()


def check(d, want):
    for name, t in want.items():
        got = getattr(d, name)
        assert (got is None) if t is None else torch.equal(got, t), name


ONE_SHOT_HIER = [("rand", (2, 16, 4, 1)), ("randn", (2, 1)), ("randn", (2, 1)), ("randn", (2, 16, 4, 1)), ("rand", (32, 4)),
                 ("randn", (2, 16, 8, 1))]
ONE_SHOT_FLAT = ONE_SHOT_HIER[:3] + [("randn", (2, 16, 4, 1))]


def test_one_shot_hierarchical_draws():
    d, calls, state = run(lambda: draw_randoms(settings(), B, CPU))
    assert calls == ONE_SHOT_HIER
    t, state_ref = replay(calls)
    check(d, dict(jitter=t[0], theta=t[1], phi=t[2], noise_c=t[3], u=t[4], noise_f=t[5]))
    assert torch.equal(state, state_ref)


@pytest.mark.parametrize("dist", ["gaussian", "uniform"])
def test_one_shot_flat_draws(dist):
    d, calls, state = run(lambda: draw_randoms(settings(hierarchical_sample=False, sample_dist=dist), B, CPU))
    cam = "rand" if dist == "uniform" else "randn"
    assert calls == [ONE_SHOT_FLAT[0], (cam, (2, 1)), (cam, (2, 1)), ONE_SHOT_FLAT[3]]
    t, state_ref = replay(calls)
    check(d, dict(jitter=t[0], theta=t[1], phi=t[2], noise_c=None, u=None, noise_f=t[3]))      # theta / phi: the RAW draws
    assert torch.equal(state, state_ref)


@pytest.mark.parametrize("hier", [True, False])
def test_explicit_camera_draws_no_angles(hier):
    cam = dict(camera_pos=torch.tensor([[0., 0., 1.]] * B), camera_lookup=torch.tensor([[0., 0., -1.]] * B))
    d, calls, state = run(lambda: draw_randoms(settings(hierarchical_sample=hier, **cam), B, CPU))
    full = ONE_SHOT_HIER if hier else ONE_SHOT_FLAT
    assert calls == full[:1] + full[3:]
    t, state_ref = replay(calls)
    check(d, dict(jitter=t[0], theta=None, phi=None, noise_c=t[1] if hier else None, u=t[2] if hier else None, noise_f=t[-1]))
    assert torch.equal(state, state_ref)


def test_staged_draws_per_image_and_chunk():
    d, calls, state = run(lambda: draw_randoms(settings(forward_points=6), B, CPU))
    image = [("rand", (1, 16, 4, 1)), ("randn", (1, 1)), ("randn", (1, 1))]
    for c in (6, 6, 4):
        image += [("randn", (1, c, 4, 1)), ("rand", (c, 4)), ("randn", (1, c, 8, 1))]
    assert calls == image * 2
    t, state_ref = replay(calls)
    per = len(image)
    chunk = lambda k: [t[i * per + 3 + 3 * c + k] for i in range(B) for c in range(3)]       # image by image, chunk by chunk
    check(d, dict(jitter=torch.cat([t[0], t[per]]), theta=torch.cat([t[1], t[per + 1]]), phi=torch.cat([t[2], t[per + 2]]),
                  noise_c=torch.cat(chunk(0), 1).view(B, N, S, 1), u=torch.cat(chunk(1), 0),
                  noise_f=torch.cat(chunk(2), 1).view(B, N, 2 * S, 1)))
    assert [tuple(x.shape) for x in (d.jitter, d.theta, d.phi, d.noise_c, d.u, d.noise_f)] == [s for _, s in ONE_SHOT_HIER]
    assert torch.equal(state, state_ref)


def test_part_draws_permutation_then_both_subsets():
    s = settings(grad_points=5, forward_points=6)          # part_grad_forward is not handed forward_points: not staged
    (d, ((idx_g, noise_g), (idx_r, noise_r))), calls, state = run(
        lambda: (draw_randoms(s, B, CPU), draw_part_randoms(s, B, CPU)))
    assert calls == [("rand", (2, 16, 4, 1)), ("randn", (2, 1)), ("randn", (2, 1)), ("randperm", (16,)),
                     ("randn", (2, 5, 4, 1)), ("rand", (10, 4)), ("randn", (2, 5, 8, 1)),
                     ("randn", (2, 11, 4, 1)), ("rand", (22, 4)), ("randn", (2, 11, 8, 1))]
    t, state_ref = replay(calls)
    check(d, dict(jitter=t[0], theta=t[1], phi=t[2], noise_c=None, u=None, noise_f=None))
    assert torch.equal(idx_g, t[3][:5]) and torch.equal(idx_r, t[3][5:])
    assert all(torch.equal(a, b) for a, b in zip(noise_g + noise_r, t[4:]))
    assert torch.equal(state, state_ref)


def test_grad_points_of_a_whole_image_is_the_one_shot_mode():
    _, calls, _ = run(lambda: draw_randoms(settings(grad_points=N), B, CPU))
    assert calls == ONE_SHOT_HIER


def test_one_shot_override_is_still_drawn_then_replaced():
    g = torch.Generator().manual_seed(5)
    ro = dict(jitter=torch.rand(B * N * S, generator=g, dtype=torch.float64), noise_f=torch.randn(B, N * 2 * S, generator=g))
    d, calls, state = run(lambda: draw_randoms(settings(rand_override=ro), B, CPU))
    assert calls == ONE_SHOT_HIER                                              # the generator is consumed all the same
    t, state_ref = replay(calls)
    check(d, dict(jitter=ro["jitter"].reshape(B, N, S, 1).float(), theta=t[1], phi=t[2], noise_c=t[3], u=t[4],
                  noise_f=ro["noise_f"].reshape(B, N, 2 * S, 1)))
    assert d.jitter.dtype == torch.float32 and d.jitter.device == CPU
    assert torch.equal(state, state_ref)


def test_staged_override_is_taken_as_given():
    ro = dict(jitter=torch.rand(B, N, S, 1, dtype=torch.float64), u=torch.rand(B * N, S))
    d, calls, state = run(lambda: draw_randoms(settings(forward_points=6, rand_override=ro), B, CPU))
    assert d.jitter is ro["jitter"] and d.u is ro["u"]
    _, state_ref = replay(calls)
    assert len(calls) == 2 * (3 + 3 * 3) and torch.equal(state, state_ref)


@pytest.mark.parametrize("mod,nerf_side,inr_side", [(generator, False, True), (generator_v1, False, False)])
def test_freeze_variants_map_the_nerf_side_under_no_grad(mod, nerf_side, inr_side, monkeypatch):
    """mapping_network() calls the _map_nerf / _map_inr hooks: v0's freeze variant runs the NeRF mapping under no_grad and
    trains the INR mapping; v1's runs both under no_grad (only the CIPS head trains)"""
    torch.manual_seed(0)
    G = mod.GeneratorNerfINR_freeze_NeRF(**G_CFG, device="cpu")
    seen = {}

    def nerf(z):
        seen["nerf"] = torch.is_grad_enabled()
        return {"nerf_w0": z}

    def inr(self, z):
        seen["inr"] = torch.is_grad_enabled()
        return {"inr_w4_0": z}

    monkeypatch.setattr(G.mapping_network_nerf, "forward", nerf)
    monkeypatch.setattr(mod.GeneratorNerfINR, "_map_inr", inr)          # the hook the freeze variant's own override calls
    assert torch.is_grad_enabled()
    styles = G.mapping_network(torch.zeros(2, 256), torch.zeros(2, 512))
    assert seen == {"nerf": nerf_side, "inr": inr_side} and list(styles) == ["nerf_w0", "inr_w4_0"]
    # the unfrozen classes map both sides with gradients
    seen.clear()
    torch.manual_seed(0)
    G = mod.GeneratorNerfINR(**G_CFG, device="cpu")
    monkeypatch.setattr(G.mapping_network_nerf, "forward", nerf)
    G.mapping_network(torch.zeros(2, 256), torch.zeros(2, 512))
    assert seen == {"nerf": True, "inr": True}
