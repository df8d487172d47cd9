"""CPU: the generator_v1 drop-ins (cips3d_amd/generator_v1.py) — the classes the AFHQ recipes build.

  * registry_v1 registers both classes under tl2's MODEL_REGISTRY contract, and `build_model` with the reference's own
    G_cfg_3D2D (afhq_exp.yaml, tests/golden/reference_layout_v1.pt) gives the reference's 174 keys, shapes, parameter count
    and module_name_list;
  * under the reference's torch seed the initial state_dict equals the reference's (the golden fixtures' checksums);
  * v1 checkpoint directories round-trip through cips3d_amd.checkpoint, and into the reference's own v1 class where the
    reference checkout exists.
No compute: there is no GPU here."""
import copy
import os
import sys

import pytest
import torch

from conftest import G_CFG, ROOT, check_checksums, load_golden

REF = "/root/reference"
has_ref = os.path.isdir(os.path.join(REF, "exp", "cips3d"))
V1_CASES = ["g_v1_r16_hier", "g_v1_r16_part", "g_v1_r8_freeze", "g_v1_r8_eval_psi_staged"]


def seeded_generator_v1(seed, freeze=False, device="cpu"):
    """conftest.seeded_generator for the v1 classes: the product module under the reference's seed"""
    from cips3d_amd.generator_v1 import GeneratorNerfINR, GeneratorNerfINR_freeze_NeRF
    torch.manual_seed(seed)
    cls = GeneratorNerfINR_freeze_NeRF if freeze else GeneratorNerfINR
    G = cls(**G_CFG, device="cpu")
    if device != "cpu":
        G = G.to(device)
        G.device = device
    return G


@pytest.fixture()
def own_tl2(monkeypatch):
    """the package's tl2 stand-in (cips3d_amd/compat/shims) in front of sys.path; tl2 modules another test installed are set
    aside for the test, the stand-in's dropped again afterwards"""
    before = set(sys.modules)
    for name in [m for m in sys.modules if m.split(".")[0] == "tl2"]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(os.path.join(ROOT, "cips3d_amd", "compat", "shims"))
    yield
    for name in set(sys.modules) - before:
        if name.split(".")[0] == "tl2":
            sys.modules.pop(name, None)


@pytest.fixture()
def reference_v1(monkeypatch):
    """the reference's own exp.cips3d.models.generator_v1, imported through oracle/ref_shim.py; every module it added and its
    sys.path entry are dropped again afterwards"""
    if not has_ref:
        pytest.skip("reference checkout only exists in the build container")
    shimmed = ("tl2", "exp", "easydict", "streamlit", "torchvision")
    before = set(sys.modules)
    for name in [m for m in sys.modules if m.split(".")[0] in shimmed]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setattr(sys, "path", list(sys.path))
    from oracle import ref_shim
    ref_shim.install()
    import importlib
    yield importlib.import_module("exp.cips3d.models.generator_v1")
    for name in set(sys.modules) - before:
        if name.split(".")[0] in shimmed:
            sys.modules.pop(name, None)


def test_registry_v1_builds_the_v1_drop_ins_from_the_reference_yaml(own_tl2):
    from tl2.proj.fvcore import MODEL_REGISTRY, build_model
    import cips3d_amd.compat.registry_v1 as reg
    from cips3d_amd.generator_v1 import GeneratorNerfINR, GeneratorNerfINR_freeze_NeRF
    names = reg.register(MODEL_REGISTRY)
    assert names == ["cips3d_amd.compat.registry_v1.GeneratorNerfINR",
                     "cips3d_amd.compat.registry_v1.GeneratorNerfINR_freeze_NeRF"]
    assert all(n in MODEL_REGISTRY for n in names)
    lay = load_golden("reference_layout_v1")            # afhq_exp.yaml's G_cfg_3D2D and the reference v1 model's layout
    assert lay["G_cfg_3D2D"]["name"] == "exp.cips3d.models.generator_v1.GeneratorNerfINR"
    for cls in (GeneratorNerfINR, GeneratorNerfINR_freeze_NeRF):
        cfg = dict(lay["G_cfg_3D2D"], register_modules=["cips3d_amd.compat.registry_v1"],
                   name=f"cips3d_amd.compat.registry_v1.{cls.__name__}")
        torch.manual_seed(0)
        G = build_model(cfg, device="cpu")                                   # train.py:228
        assert type(G) is cls
        sd = G.state_dict()
        assert len(sd) == 174 and sum(p.numel() for p in G.parameters()) == 11353407 == lay["num_params"]
        assert [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in sd.items()] == list(lay["G_state"])
        assert G.module_name_list == lay["module_name_list"] == ["siren", "mapping_network_nerf", "inr_net",
                                                                 "mapping_network_inr", "nerf_rgb_mapping", "aux_to_rbg"]
        # nerf_rgb is the INR mapping network's first head, no longer the SIREN's (generator_v1.py:1192-1206)
        assert list(G.mapping_network_inr.head_dim_dict) == lay["mapping_inr_heads"] and lay["mapping_inr_heads"][0] == "nerf_rgb"
        assert list(G.siren.style_dim_dict) == lay["siren_styles"] == ["nerf_w0", "nerf_w1"]
        assert list(G.mapping_network_nerf.head_dim_dict) == ["nerf_w0", "nerf_w1"]


@pytest.mark.parametrize("tag", V1_CASES)
def test_seeded_v1_initial_state_matches_the_reference(tag):
    """same torch seed -> the reference's initial state_dict, bit for bit (nerf_rgb_mapping draws before aux_to_rbg)"""
    fix = load_golden(tag)
    G = seeded_generator_v1(fix["seed"], freeze=fix["freeze"])
    check_checksums(G.state_dict(), fix["state_checksums"])


def test_v1_differs_from_v0_only_by_nerf_rgb_mapping_and_the_draws_after_it():
    """v0 and v1 share every key but nerf_rgb_mapping.*; under one seed their weights agree up to mapping_network_inr and
    aux_to_rbg differs (its draws come after nerf_rgb_mapping's)"""
    from conftest import seeded_generator
    v0, v1 = seeded_generator(7).state_dict(), seeded_generator_v1(7).state_dict()
    assert [k for k in v1 if k not in v0] == ["nerf_rgb_mapping.weight", "nerf_rgb_mapping.bias"] and set(v0) <= set(v1)
    assert all(torch.equal(v0[k], v1[k]) for k in v0 if not k.startswith("aux_to_rbg."))
    assert not torch.equal(v0["aux_to_rbg.0.weight"], v1["aux_to_rbg.0.weight"])


def test_v1_checkpoint_directory_round_trips(tmp_path):
    """a {generator, G_ema, state_dict} directory of v1 models (174 keys each) loads strictly into fresh v1 models, values bit
    for bit; the freeze variant loads it too and load_nerf_ema copies the INR-side mapping and nerf_rgb_mapping as well"""
    from cips3d_amd.checkpoint import save_models, load_models, Checkpointer
    G = seeded_generator_v1(11)
    G_ema = copy.deepcopy(G)
    with torch.no_grad():
        for p in G_ema.parameters():
            p.mul_(0.5)
    state = {"cur_fid": 20.0, "best_fid": 18.5, "worst_fid": 300.0, "step": 77}
    d = str(tmp_path / "v1")
    save_models(d, {"generator": G, "G_ema": G_ema, "state_dict": state})
    assert len(torch.load(os.path.join(d, "generator.pth"), weights_only=False)) == 174
    G2, G2_ema, st = seeded_generator_v1(12), seeded_generator_v1(13), {}
    load_models(d, {"generator": G2, "G_ema": G2_ema, "state_dict": st}, strict=True)
    assert st == state
    for a, b in ((G2, G), (G2_ema, G_ema)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    G3 = seeded_generator_v1(14)
    Checkpointer(G3).load_state_dict_from_file(os.path.join(d, "G_ema.pth"))
    assert all(torch.equal(v, G_ema.state_dict()[k]) for k, v in G3.state_dict().items())
    Gf = seeded_generator_v1(15, freeze=True)
    load_models(d, {"generator": Gf}, strict=True)
    Gf.load_nerf_ema(G_ema)                              # generator_v1.py:1973-1980
    for name in ("siren", "mapping_network_nerf", "aux_to_rbg", "mapping_network_inr", "nerf_rgb_mapping"):
        sa, sb = getattr(Gf, name).state_dict(), getattr(G_ema, name).state_dict()
        assert all(torch.equal(sa[k], sb[k]) for k in sa), name
    assert torch.equal(Gf.inr_net.to_rgbs["4"].linear.weight, G.inr_net.to_rgbs["4"].linear.weight)
    # a v0 directory (172 keys) is not a v1 checkpoint
    from conftest import seeded_generator
    d0 = str(tmp_path / "v0")
    save_models(d0, {"generator": seeded_generator(1)})
    with pytest.raises(RuntimeError, match="nerf_rgb_mapping"):
        load_models(d0, {"generator": seeded_generator_v1(1)}, strict=True)


def test_v1_checkpoint_loads_into_the_reference_v1_class_and_back(tmp_path, reference_v1):
    """the reference's own generator_v1.GeneratorNerfINR reads a directory the drop-in wrote (strict) and vice versa"""
    from cips3d_amd.checkpoint import save_models, load_models
    G = seeded_generator_v1(21)
    d = str(tmp_path / "from_mi355x")
    save_models(d, {"generator": G, "G_ema": G})
    torch.manual_seed(22)
    R = reference_v1.GeneratorNerfINR(**G_CFG, device="cpu")
    load_models(d, {"G_ema": R}, strict=True)
    assert list(R.state_dict()) == list(G.state_dict())
    assert all(torch.equal(v, G.state_dict()[k]) for k, v in R.state_dict().items())
    with torch.no_grad():
        for p in R.parameters():
            p.add_(0.25)
    d2 = str(tmp_path / "from_reference")
    save_models(d2, {"generator": R})
    G2 = seeded_generator_v1(23)
    load_models(d2, {"generator": G2}, strict=True)
    assert all(torch.equal(v, R.state_dict()[k]) for k, v in G2.state_dict().items())
