"""CPU: every public entry point of GeneratorNerfINR hands down the RenderSettings it was asked for, and keeps its signature.

The entry points build their settings by name out of their own arguments (RenderSettings.of), so a parameter bound to the
wrong field — or one that silently keeps its default — would show only as a tolerance failure far away.  Here nothing
renders: the methods the settings are handed to (_render_styles behind the latent and style entry points, _density_camera
behind geometry() and surface()) and the GPU guard are replaced, every argument is a value of its own ('<its name>'), and
the captured settings are compared field by field with expectations written out below by hand, never through the builder."""
import dataclasses
import inspect
import math

import pytest
import torch

from conftest import seeded_generator
from test_generator_v1_cpu import seeded_generator_v1

REQ = inspect.Parameter.empty
HALF_PI = math.pi * 0.5

# name -> [(parameter, default)], as the entry points were before they shared one settings builder ('**' marks **kwargs)
SIGNATURES = {
    "forward": [
        ("zs", REQ), ("img_size", REQ), ("fov", REQ), ("ray_start", REQ), ("ray_end", REQ), ("num_steps", REQ), ("h_stddev", REQ),
        ("v_stddev", REQ), ("hierarchical_sample", REQ), ("h_mean", HALF_PI), ("v_mean", HALF_PI), ("psi", 1), ("sample_dist", None),
        ("lock_view_dependence", False), ("clamp_mode", "relu"), ("nerf_noise", 0.), ("white_back", False), ("last_back", False),
        ("return_aux_img", False), ("grad_points", None), ("forward_points", None), ("**kwargs", REQ)],
    "forward_camera_pos_and_lookup": [
        ("zs", REQ), ("img_size", REQ), ("fov", REQ), ("ray_start", REQ), ("ray_end", REQ), ("num_steps", REQ), ("h_stddev", REQ),
        ("v_stddev", REQ), ("h_mean", REQ), ("v_mean", REQ), ("hierarchical_sample", REQ), ("camera_pos", REQ), ("camera_lookup", REQ),
        ("psi", 1), ("sample_dist", None), ("lock_view_dependence", False), ("clamp_mode", "relu"), ("nerf_noise", 0.),
        ("white_back", False), ("last_back", False), ("return_aux_img", False), ("grad_points", None), ("forward_points", None),
        ("up_vector", None), ("**kwargs", REQ)],
    "forward_styles": [
        ("styles", REQ), ("img_size", REQ), ("fov", REQ), ("ray_start", REQ), ("ray_end", REQ), ("num_steps", REQ), ("h_stddev", REQ),
        ("v_stddev", REQ), ("hierarchical_sample", REQ), ("h_mean", HALF_PI), ("v_mean", HALF_PI), ("sample_dist", None),
        ("lock_view_dependence", False), ("clamp_mode", "relu"), ("nerf_noise", 0.), ("white_back", False), ("last_back", False),
        ("return_aux_img", False), ("grad_points", None), ("forward_points", None), ("camera_pos", None), ("camera_lookup", None),
        ("up_vector", None), ("**kwargs", REQ)],
    "render": [
        ("zs", REQ), ("img_size", REQ), ("fov", REQ), ("ray_start", REQ), ("ray_end", REQ), ("num_steps", REQ), ("h_stddev", REQ),
        ("v_stddev", REQ), ("hierarchical_sample", REQ), ("h_mean", HALF_PI), ("v_mean", HALF_PI), ("psi", 1), ("sample_dist", None),
        ("clamp_mode", "relu"), ("nerf_noise", 0.), ("white_back", False), ("last_back", False), ("return_aux_img", False),
        ("camera_pos", None), ("camera_lookup", None), ("up_vector", None), ("rand_override", None), ("grad_points", None),
        ("forward_points", None)],
    "render_styles": [
        ("styles", REQ), ("img_size", REQ), ("fov", REQ), ("ray_start", REQ), ("ray_end", REQ), ("num_steps", REQ), ("h_stddev", REQ),
        ("v_stddev", REQ), ("hierarchical_sample", REQ), ("h_mean", HALF_PI), ("v_mean", HALF_PI), ("sample_dist", None),
        ("clamp_mode", "relu"), ("nerf_noise", 0.), ("white_back", False), ("last_back", False), ("return_aux_img", False),
        ("camera_pos", None), ("camera_lookup", None), ("up_vector", None), ("rand_override", None), ("grad_points", None),
        ("forward_points", None)],
    "geometry": [
        ("zs", REQ), ("img_size", REQ), ("fov", REQ), ("ray_start", REQ), ("ray_end", REQ), ("num_steps", REQ), ("h_stddev", REQ),
        ("v_stddev", REQ), ("hierarchical_sample", REQ), ("h_mean", HALF_PI), ("v_mean", HALF_PI), ("psi", 1), ("sample_dist", None),
        ("clamp_mode", "relu"), ("white_back", False), ("last_back", False), ("camera_pos", None), ("camera_lookup", None),
        ("up_vector", None), ("rand_override", None)],
    "surface": [
        ("zs", REQ), ("level", REQ), ("img_size", REQ), ("fov", REQ), ("ray_start", REQ), ("ray_end", REQ), ("num_steps", REQ),
        ("h_stddev", REQ), ("v_stddev", REQ), ("h_mean", HALF_PI), ("v_mean", HALF_PI), ("psi", 1), ("sample_dist", None),
        ("camera_pos", None), ("camera_lookup", None), ("up_vector", None), ("refine", 8), ("normals", True),
        ("rand_override", None)],
}
# generator_v1's forward_camera_pos_and_lookup: v0's without the up_vector parameter (a keyword one lands in **kwargs)
V1_CAMERA_SIGNATURE = [p for p in SIGNATURES["forward_camera_pos_and_lookup"] if p[0] != "up_vector"]

# the settings each entry point must hand down when every argument `x` is given as '<x>': all 22 fields, by hand
EXPECTED = {
    "forward": dict(
        img_size="<img_size>", fov="<fov>", ray_start="<ray_start>", ray_end="<ray_end>", num_steps="<num_steps>",
        h_stddev="<h_stddev>", v_stddev="<v_stddev>", h_mean="<h_mean>", v_mean="<v_mean>",
        hierarchical_sample="<hierarchical_sample>", sample_dist="<sample_dist>", clamp_mode="<clamp_mode>",
        nerf_noise="<nerf_noise>", white_back="<white_back>", last_back="<last_back>", return_aux_img="<return_aux_img>",
        forward_points="<forward_points>", grad_points="<grad_points>", camera_pos=None, camera_lookup=None, up_vector=None,
        rand_override="<rand_override>"),
    "forward_camera_pos_and_lookup": dict(
        img_size="<img_size>", fov="<fov>", ray_start="<ray_start>", ray_end="<ray_end>", num_steps="<num_steps>",
        h_stddev="<h_stddev>", v_stddev="<v_stddev>", h_mean="<h_mean>", v_mean="<v_mean>",
        hierarchical_sample="<hierarchical_sample>", sample_dist="<sample_dist>", clamp_mode="<clamp_mode>",
        nerf_noise="<nerf_noise>", white_back="<white_back>", last_back="<last_back>", return_aux_img="<return_aux_img>",
        forward_points="<forward_points>", grad_points="<grad_points>", camera_pos="<camera_pos>",
        camera_lookup="<camera_lookup>", up_vector="<up_vector>", rand_override="<rand_override>"),
    "v1.forward_camera_pos_and_lookup": dict(
        img_size="<img_size>", fov="<fov>", ray_start="<ray_start>", ray_end="<ray_end>", num_steps="<num_steps>",
        h_stddev="<h_stddev>", v_stddev="<v_stddev>", h_mean="<h_mean>", v_mean="<v_mean>",
        hierarchical_sample="<hierarchical_sample>", sample_dist="<sample_dist>", clamp_mode="<clamp_mode>",
        nerf_noise="<nerf_noise>", white_back="<white_back>", last_back="<last_back>", return_aux_img="<return_aux_img>",
        forward_points="<forward_points>", grad_points="<grad_points>", camera_pos="<camera_pos>",
        camera_lookup="<camera_lookup>", up_vector=None, rand_override="<rand_override>"),
    "forward_styles": dict(
        img_size="<img_size>", fov="<fov>", ray_start="<ray_start>", ray_end="<ray_end>", num_steps="<num_steps>",
        h_stddev="<h_stddev>", v_stddev="<v_stddev>", h_mean="<h_mean>", v_mean="<v_mean>",
        hierarchical_sample="<hierarchical_sample>", sample_dist="<sample_dist>", clamp_mode="<clamp_mode>",
        nerf_noise="<nerf_noise>", white_back="<white_back>", last_back="<last_back>", return_aux_img="<return_aux_img>",
        forward_points="<forward_points>", grad_points="<grad_points>", camera_pos="<camera_pos>",
        camera_lookup="<camera_lookup>", up_vector="<up_vector>", rand_override="<rand_override>"),
    "render": dict(
        img_size="<img_size>", fov="<fov>", ray_start="<ray_start>", ray_end="<ray_end>", num_steps="<num_steps>",
        h_stddev="<h_stddev>", v_stddev="<v_stddev>", h_mean="<h_mean>", v_mean="<v_mean>",
        hierarchical_sample="<hierarchical_sample>", sample_dist="<sample_dist>", clamp_mode="<clamp_mode>",
        nerf_noise="<nerf_noise>", white_back="<white_back>", last_back="<last_back>", return_aux_img="<return_aux_img>",
        forward_points=None, grad_points=None, camera_pos="<camera_pos>", camera_lookup="<camera_lookup>",
        up_vector="<up_vector>", rand_override="<rand_override>"),
    "render_styles": dict(
        img_size="<img_size>", fov="<fov>", ray_start="<ray_start>", ray_end="<ray_end>", num_steps="<num_steps>",
        h_stddev="<h_stddev>", v_stddev="<v_stddev>", h_mean="<h_mean>", v_mean="<v_mean>",
        hierarchical_sample="<hierarchical_sample>", sample_dist="<sample_dist>", clamp_mode="<clamp_mode>",
        nerf_noise="<nerf_noise>", white_back="<white_back>", last_back="<last_back>", return_aux_img="<return_aux_img>",
        forward_points=None, grad_points=None, camera_pos="<camera_pos>", camera_lookup="<camera_lookup>",
        up_vector="<up_vector>", rand_override="<rand_override>"),
    "geometry": dict(
        img_size="<img_size>", fov="<fov>", ray_start="<ray_start>", ray_end="<ray_end>", num_steps="<num_steps>",
        h_stddev="<h_stddev>", v_stddev="<v_stddev>", h_mean="<h_mean>", v_mean="<v_mean>",
        hierarchical_sample="<hierarchical_sample>", sample_dist="<sample_dist>", clamp_mode="<clamp_mode>",
        nerf_noise=0., white_back="<white_back>", last_back="<last_back>", return_aux_img=False,
        forward_points=None, grad_points=None, camera_pos="<camera_pos>", camera_lookup="<camera_lookup>",
        up_vector="<up_vector>", rand_override="<rand_override>"),
    "surface": dict(
        img_size="<img_size>", fov="<fov>", ray_start="<ray_start>", ray_end="<ray_end>", num_steps="<num_steps>",
        h_stddev="<h_stddev>", v_stddev="<v_stddev>", h_mean="<h_mean>", v_mean="<v_mean>",
        hierarchical_sample=False, sample_dist="<sample_dist>", clamp_mode="relu",
        nerf_noise=0., white_back=False, last_back=False, return_aux_img=False,
        forward_points=None, grad_points=None, camera_pos="<camera_pos>", camera_lookup="<camera_lookup>",
        up_vector="<up_vector>", rand_override="<rand_override>"),
}


class _Captured(Exception):
    """ends an entry point where it hands its settings down"""


@pytest.fixture(scope="module")
def generators():
    return {"": seeded_generator(3), "v1.": seeded_generator_v1(3)}


def _call(G, monkeypatch, name, lead, **extra):
    """G.<name>(lead, <every other named parameter x>='<x>', **extra) with nothing rendered -> the settings handed down.
    psi stays 1 (it selects the truncation, it is no settings field); render / render_styles refuse grad_points and
    forward_points, so they are left out there."""
    def capture(*args, **kwargs):
        raise _Captured([a for a in args if dataclasses.is_dataclass(a)][0])

    monkeypatch.setattr(G, "_render_styles", capture)
    monkeypatch.setattr(G, "_density_camera", capture)
    monkeypatch.setattr(G, "_gpu_only", lambda name: torch.device("cpu"))
    skip = {"psi"} | ({"grad_points", "forward_points"} if name.startswith("render") else set())
    params = list(inspect.signature(getattr(G, name)).parameters.values())[1:]
    args = {p.name: f"<{p.name}>" for p in params if p.kind is not p.VAR_KEYWORD and p.name not in skip}
    with pytest.raises(_Captured) as e:
        getattr(G, name)(lead, **args, **extra)
    return e.value.args[0]


def _assert_fields(s, expected):
    from cips3d_amd.generator import RenderSettings
    assert type(s) is RenderSettings
    assert set(expected) == {f.name for f in dataclasses.fields(RenderSettings)}
    for field, want in expected.items():
        got = getattr(s, field)
        assert type(got) is type(want) and got == want, (field, got, want)


@pytest.mark.parametrize("name", ["forward", "forward_camera_pos_and_lookup", "v1.forward_camera_pos_and_lookup", "forward_styles",
                                  "render", "render_styles", "geometry", "surface"])
def test_entry_point_hands_down_the_settings_it_was_asked_for(generators, monkeypatch, name):
    G, method = generators[name[:-len(name.split(".")[-1])]], name.split(".")[-1]
    zs = {"z_nerf": torch.zeros(1, 256), "z_inr": torch.zeros(1, 512)}
    lead = G.styles(zs) if method.endswith("_styles") else zs
    # the entry points with **kwargs take rand_override from there; generator_v1's camera entry point also an up_vector,
    # which it drops
    extra = {}
    if "**kwargs" in [p[0] for p in SIGNATURES.get(method, [])]:
        extra["rand_override"] = "<rand_override>"
    if name.startswith("v1."):
        extra["up_vector"] = "<up_vector>"
    _assert_fields(_call(G, monkeypatch, method, lead, **extra), EXPECTED[name])


@pytest.mark.parametrize("name", ["render", "render_styles"])
def test_render_refuses_points_before_anything_else(generators, monkeypatch, name):
    """any value but None, and before the GPU guard (which here would pass) and the settings"""
    G = generators[""]
    zs = {"z_nerf": torch.zeros(1, 256), "z_inr": torch.zeros(1, 512)}
    monkeypatch.setattr(G, "_gpu_only", lambda name: pytest.fail("the refusal of grad_points / forward_points comes first"))
    a = dict(img_size=8, fov=12, ray_start=0.88, ray_end=1.12, num_steps=4, h_stddev=0.3, v_stddev=0.155, hierarchical_sample=False)
    for kw, word in ((dict(grad_points=64), "grad_points"), (dict(forward_points=64), "forward_points"), (dict(grad_points=0), "whole images")):
        with pytest.raises(ValueError, match=word):
            getattr(G, name)(G.styles(zs) if name == "render_styles" else zs, **a, **kw)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature_is_unchanged(name):
    from cips3d_amd import generator, generator_v1

    def listed(fn):
        return [("**" + p.name if p.kind is p.VAR_KEYWORD else p.name, p.default)
                for p in list(inspect.signature(fn).parameters.values())[1:]]

    assert listed(getattr(generator.GeneratorNerfINR, name)) == SIGNATURES[name]
    assert listed(getattr(generator.GeneratorNerfINR_freeze_NeRF, name)) == SIGNATURES[name]
    want_v1 = V1_CAMERA_SIGNATURE if name == "forward_camera_pos_and_lookup" else SIGNATURES[name]
    assert listed(getattr(generator_v1.GeneratorNerfINR, name)) == want_v1
    assert listed(getattr(generator_v1.GeneratorNerfINR_freeze_NeRF, name)) == want_v1
