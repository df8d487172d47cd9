"""CPU (build container): the shipped reference-side bindings (cips3d_amd/compat).

  * the UNMODIFIED reference files exp/comm/op/fused_act.py and exp/comm/op/upfirdn2d.py import on top of the HIP-backed
    `fused` / `upfirdn2d_op` stand-ins (their module-level `load(...)` calls receive the stand-ins), and the pybind call
    signatures match what those files call (fused_bias_act.cpp:11-21, upfirdn2d.cpp:12-23);
  * the registry module registers the drop-in classes under tl2's MODEL_REGISTRY contract, and `build_model` with the
    reference's own YAML config (ffhq_exp.yaml) constructs them with the reference's parameter count and key order;
  * checkpoint directories round-trip between the drop-in classes and the reference's state_dict layout.
No compute: there is no GPU here (the ops raise the reference's "must be a CUDA tensor" error on CPU tensors).
The first test runs the reference's own files and skips where the reference checkout is absent; the registry and checkpoint
tests read the reference's configuration and state_dict layout from tests/golden/reference_layout.pt (oracle/make_golden.py)."""
import importlib.util
import inspect
import os
import sys

import pytest
import torch

from conftest import load_golden

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="reference checkout only exists in the build container")


def _load_ref_file(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference_layout_module(entries):
    """A module whose state_dict has exactly the reference's keys, order, shapes and dtypes (`entries` from
    reference_layout.pt), filled from torch's current seed: what the reference's own classes write to and read from a
    checkpoint directory"""
    root = torch.nn.Module()
    for key, shape, dtype in entries:
        *path, leaf = key.split(".")
        m = root
        for name in path:
            if name not in m._modules:
                m.add_module(name, torch.nn.Module())
            m = m._modules[name]
        t = torch.randn(shape).to(getattr(torch, dtype))
        m.register_parameter(leaf, torch.nn.Parameter(t, requires_grad=t.is_floating_point()))
    assert [(k, tuple(v.shape)) for k, v in root.state_dict().items()] == [(k, tuple(s_)) for k, s_, _ in entries]
    return root


@needs_ref
def test_unmodified_reference_op_files_bind_to_the_hip_standins():
    from cips3d_amd import compat
    import torch.utils.cpp_extension as ce
    real = ce.load
    compat.patch_cpp_extension_load()
    try:
        fa = _load_ref_file("_ref_fused_act", "exp/comm/op/fused_act.py")          # runs `fused = load('fused', ...)`
        up = _load_ref_file("_ref_upfirdn2d", "exp/comm/op/upfirdn2d.py")          # runs `upfirdn2d_op = load('upfirdn2d', ...)`
    finally:
        ce.load = real
    assert fa.fused is compat.fused and up.upfirdn2d_op is compat.upfirdn2d_op
    # the pybind signatures (argument order and names of fused_bias_act.cpp:11-12 / upfirdn2d.cpp:12-14)
    assert list(inspect.signature(compat.fused.fused_bias_act).parameters) == \
        ["input", "bias", "refer", "act", "grad", "alpha", "scale"]
    assert list(inspect.signature(compat.upfirdn2d_op.upfirdn2d).parameters) == \
        ["input", "kernel", "up_x", "up_y", "down_x", "down_y", "pad_x0", "pad_x1", "pad_y0", "pad_y1"]
    # the reference's autograd classes and module exist on top of them and reach the op with the reference's calls:
    # on a CPU tensor the op raises the reference's CHECK_CUDA error (fused_bias_act.cpp:13) instead of computing
    m = fa.FusedLeakyReLU(4)
    assert isinstance(m, torch.nn.Module) and m.bias.shape == (4,)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        fa.fused_leaky_relu(torch.zeros(1, 4, 2, 2), torch.zeros(4))
    k = torch.ones(4, 4) / 16
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        up.upfirdn2d(torch.zeros(1, 2, 8, 8), k, up=1, down=1, pad=(2, 1))
    with pytest.raises(RuntimeError, match="no HIP stand-in"):
        compat.load("something_else")


@pytest.fixture()
def own_tl2(monkeypatch):
    """tl2 is not installed here: the package's own stand-in (cips3d_amd/compat/shims) provides its registry contract; tl2
    modules another test installed are set aside for the test, the stand-in's dropped again afterwards"""
    before = set(sys.modules)
    for name in [m for m in sys.modules if m.split(".")[0] == "tl2"]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cips3d_amd", "compat", "shims"))
    yield
    for name in set(sys.modules) - before:
        if name.split(".")[0] == "tl2":
            sys.modules.pop(name, None)


def test_registry_builds_the_drop_in_models_from_the_reference_yaml(own_tl2):
    from tl2.proj.fvcore import MODEL_REGISTRY, build_model
    import cips3d_amd.compat.registry as reg
    names = reg.register(MODEL_REGISTRY)
    assert "cips3d_amd.compat.registry.GeneratorNerfINR" in names
    cfg = load_golden("reference_layout")               # ffhq_exp.yaml's G_cfg_3D2D / D_cfg and the reference models' layout
    g_cfg = dict(cfg["G_cfg_3D2D"], register_modules=["cips3d_amd.compat.registry"],
                 name="cips3d_amd.compat.registry.GeneratorNerfINR")
    d_cfg = dict(cfg["D_cfg"], register_modules=["cips3d_amd.compat.registry"],
                 name="cips3d_amd.compat.registry.Discriminator_MultiScale_Aux")
    torch.manual_seed(0)
    G = build_model(g_cfg, device="cpu")                 # train.py:228
    D = build_model(d_cfg, kwargs_priority=True, diffaug=False)          # train.py:229
    from cips3d_amd import GeneratorNerfINR, Discriminator_MultiScale_Aux
    assert type(G) is GeneratorNerfINR and type(D) is Discriminator_MultiScale_Aux
    assert sum(p.numel() for p in G.parameters()) == 11287743 and len(G.state_dict()) == 172
    assert sum(p.numel() for p in D.parameters()) == 37518914 and len(D.state_dict()) == 160
    # same key order, shapes and dtypes as the reference's own classes built from the same YAML
    for net, ref in ((G, cfg["G_state"]), (D, cfg["D_state"])):
        assert [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in net.state_dict().items()] == list(ref)


def test_checkpoint_directory_round_trips_with_the_reference_classes(tmp_path):
    """tl2-layout checkpoint directory ({generator, G_ema, discriminator, state_dict}.pth; train.py:249-256): a directory
    written from modules with the REFERENCE's state_dict layout (keys, order, shapes, dtypes of its classes built from
    ffhq_exp.yaml, tests/golden/reference_layout.pt) loads into the drop-in classes (strict) and a directory written from the
    drop-in classes loads into such modules (strict), values bit for bit; `Checkpointer(...)
    .load_state_dict_from_file(G_ema.pth)` (gen_images.py:102) reads the single-network file."""
    import copy
    from cips3d_amd import GeneratorNerfINR, Discriminator_MultiScale_Aux
    from cips3d_amd.checkpoint import save_models, load_models, Checkpointer
    from conftest import G_CFG, D_CFG
    lay = load_golden("reference_layout")
    torch.manual_seed(5)
    Gr = _reference_layout_module(lay["G_state"])
    Dr = _reference_layout_module(lay["D_state"])
    Gr_ema = copy.deepcopy(Gr)
    with torch.no_grad():
        for p in Gr_ema.parameters():
            p.mul_(0.5)
    state = {"cur_fid": 12.5, "best_fid": 11.0, "worst_fid": 300.0, "step": 4321}
    d1 = str(tmp_path / "from_reference")
    save_models(d1, {"generator": Gr, "G_ema": Gr_ema, "discriminator": Dr, "state_dict": state}, info_msg="step: 4321")
    assert sorted(os.listdir(d1)) == ["0info.txt", "G_ema.pth", "discriminator.pth", "generator.pth", "state_dict.pth"]
    torch.manual_seed(99)                                   # different initial weights: everything must come from disk
    G = GeneratorNerfINR(**G_CFG, device="cpu"); G_ema = copy.deepcopy(G); D = Discriminator_MultiScale_Aux(**D_CFG)
    st = {}
    load_models(d1, {"generator": G, "G_ema": G_ema, "discriminator": D, "state_dict": st}, strict=True)
    assert st == state
    for a, b in ((G, Gr), (G_ema, Gr_ema), (D, Dr)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    # the other direction, and the single-file loader of gen_images.py:102
    d2 = str(tmp_path / "from_mi355x")
    with torch.no_grad():
        for p in G_ema.parameters():
            p.add_(1.0)
    save_models(d2, {"generator": G, "G_ema": G_ema, "discriminator": D, "state_dict": st})
    torch.manual_seed(7)
    Gr2 = _reference_layout_module(lay["G_state"])
    Checkpointer(Gr2).load_state_dict_from_file(os.path.join(d2, "G_ema.pth"))
    assert all(torch.equal(v, G_ema.state_dict()[k]) for k, v in Gr2.state_dict().items())
    # freeze variant: load_nerf_ema (generator.py:1957-1961) copies the NeRF side of G_ema
    from cips3d_amd import GeneratorNerfINR_freeze_NeRF
    Gf = GeneratorNerfINR_freeze_NeRF(**G_CFG, device="cpu")
    load_models(d2, {"generator": Gf}, strict=True)
    Gf.load_nerf_ema(G_ema)
    assert torch.equal(Gf.siren.network[0].linear.weight, G_ema.siren.network[0].linear.weight)
    # a missing file: skipped with strict=False (train.py:262 loads with strict=False), an error with strict=True
    os.remove(os.path.join(d2, "discriminator.pth"))
    load_models(d2, {"discriminator": D}, strict=False)
    with pytest.raises(FileNotFoundError):
        load_models(d2, {"discriminator": D}, strict=True)


def test_checkpoint_nested_optimizer_state_and_wrapped_payload(tmp_path):
    """save_models maps tensors to the CPU through NESTED containers (an optimiser's state -> index -> exp_avg /
    exp_avg_sq) and the round trip restores the optimiser; Checkpointer also reads a file whose state_dict sits under a
    wrapper key ({'model': sd}) — round-2 advisor items on checkpoint.py."""
    from cips3d_amd.checkpoint import save_models, load_models, Checkpointer, _to_cpu
    torch.manual_seed(3)
    net = torch.nn.Linear(5, 3)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, betas=(0.0, 0.999))
    net(torch.randn(4, 5)).sum().backward()
    opt.step()
    d = str(tmp_path / "ckpt")
    save_models(d, {"net": net, "opt": opt, "state_dict": {"step": 7}})
    raw = torch.load(os.path.join(d, "opt.pth"), weights_only=False)
    assert set(raw) == {"state", "param_groups"} and all(t.device.type == "cpu" for st in raw["state"].values()
                                                          for t in st.values() if torch.is_tensor(t))
    net2 = torch.nn.Linear(5, 3); opt2 = torch.optim.Adam(net2.parameters(), lr=5.0)
    st = {}
    load_models(d, {"net": net2, "opt": opt2, "state_dict": st})
    assert st == {"step": 7} and opt2.param_groups[0]["lr"] == 1e-3
    for a, b in zip(opt.state_dict()["state"].values(), opt2.state_dict()["state"].values()):
        assert torch.equal(a["exp_avg"], b["exp_avg"]) and torch.equal(a["exp_avg_sq"], b["exp_avg_sq"])
    # nested containers keep their types; non-tensors pass through
    x = _to_cpu({"a": [torch.ones(2), (torch.zeros(1), 3)], "b": "s"})
    assert isinstance(x["a"], list) and isinstance(x["a"][1], tuple) and x["a"][1][1] == 3 and x["b"] == "s"
    # wrapped single-network file
    p = str(tmp_path / "wrapped.pth")
    torch.save({"model": net.state_dict(), "epoch": 3}, p)
    net3 = torch.nn.Linear(5, 3)
    Checkpointer(net3).load_state_dict_from_file(p)
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net3.state_dict().values()))
    # a combined file names several networks: ambiguous without `key`, selectable with it
    other = torch.nn.Linear(5, 3)
    p2 = str(tmp_path / "combined.pth")
    torch.save({"generator": other.state_dict(), "G_ema": net.state_dict(), "state_dict": {"step": 7}}, p2)
    net4 = torch.nn.Linear(5, 3)
    with pytest.raises(KeyError, match="key="):
        Checkpointer(net4).load_state_dict_from_file(p2)
    Checkpointer(net4).load_state_dict_from_file(p2, key="G_ema")
    assert all(torch.equal(a, b) for a, b in zip(net.state_dict().values(), net4.state_dict().values()))
    with pytest.raises(KeyError):
        Checkpointer(net4).load_state_dict_from_file(p2, key="discriminator")


def test_graph_capture_and_side_streams_fail_loudly_or_stay_inline_without_a_gpu():
    """No CPU path: the capture helper refuses; the discriminator's side stream is only taken for GPU tensors (module construction
    and the switch itself need no GPU)."""
    import pytest
    import torch
    from cips3d_amd import graph, discriminator
    if torch.cuda.is_available():
        pytest.skip("CPU-side behaviour")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        graph.capture(lambda: None)
    assert discriminator.AUX_SIDE_STREAM is True
    D = discriminator.Discriminator_MultiScale_Aux(diffaug=False, max_size=64, channel_multiplier=2, first_downsample=False, stddev_group=0)
    with pytest.raises(RuntimeError):                       # CPU tensors reach the HIP-only operators in line, and those refuse
        D(torch.zeros(2, 3, 16, 16), alpha=1.0, use_aux_disc=True)
