"""TEST INFRASTRUCTURE — mint the generator_v1 golden fixtures from the UNMODIFIED reference.

Run in a checkout that has the reference next to it (`python scripts/make_golden_v1.py`), like oracle/make_golden.py, whose
import shim and recording helpers it uses: it runs exp.cips3d.models.generator_v1 on CPU with its configuration from
afhq_exp.yaml (G_cfg_3D2D), every torch.rand / randn / randperm draw captured and the CIPS head's LeakyReLU gates recorded, and
writes to tests/golden/:

  reference_layout_v1.pt     the config, state_dict layout (key, shape, dtype), parameter count and module_name_list
  g_v1_r16_hier.pt           full gradient, hierarchical sampling, aux image          (+ gates_g_v1_r16_hier.pt)
  g_v1_r16_part.pt           part_grad_forward through grad_points=96                 (+ gates_g_v1_r16_part.pt)
  g_v1_r8_freeze.pt          GeneratorNerfINR_freeze_NeRF                             (+ gates_g_v1_r8_freeze.pt)
  g_v1_r8_eval_psi_staged.pt psi < 1 (truncation through the mapped nerf_rgb), staged forward_points, no grad

Weights are not stored: the drop-in classes reproduce the reference's initial state_dict under the same torch seed (stored as
per-key checksums).  The camera is the AFHQ recipes' (afhq_exp.yaml:64-77: fov 12, rays 0.8-1.2, h/v stddev 0.5/0.4).
"""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch
import yaml

from oracle import ref_shim
from oracle.make_golden import Capture, HeadGates, checksums, save_gates

ref_shim.install()

from exp.cips3d.models import generator_v1 as ref_v1        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
CFG = yaml.safe_load(open(os.path.join(ref_shim.REFERENCE_ROOT, "exp/cips3d/configs/afhq_exp.yaml")))
KW = dict(fov=12, ray_start=0.8, ray_end=1.2, h_stddev=0.5, v_stddev=0.4, sample_dist="gaussian")


def grad_digest(named_params):
    """oracle.make_golden.grad_digest's format (norm over the whole tensor, every `stride`-th element) with sparser samples,
    so that each fixture stays well under 1 MiB: tensors above 4096 elements keep every 29th, above 70 000 every 197th"""
    d = {}
    for name, p in named_params:
        if p.grad is None:
            d[name] = None
            continue
        g = p.grad.detach().reshape(-1)
        stride = 197 if g.numel() > 70000 else 29 if g.numel() > 4096 else 1
        d[name] = dict(norm=float(g.double().norm()), n=g.numel(), sample=g[::stride].clone(), stride=stride)
    return d


def g_cfg():
    c = dict(CFG["G_cfg_3D2D"])
    c.pop("register_modules"); c.pop("name")
    return c


def _save(tag, fix, imgs):
    path = os.path.join(OUT, f"{tag}.pt")
    torch.save(fix, path)
    print(tag, "->", path, os.path.getsize(path) // 1024, "KiB", "imgs", tuple(imgs.shape))


def make_train_case(tag, seed, b, img_size, S, hier, nerf_noise, aux, freeze=False, grad_points=None):
    """one G forward + backward of (imgs * G0).sum(): whole_grad_forward, or part_grad_forward with `grad_points`"""
    torch.manual_seed(seed)
    cls = ref_v1.GeneratorNerfINR_freeze_NeRF if freeze else ref_v1.GeneratorNerfINR
    G = cls(**g_cfg(), device="cpu")
    sums = checksums(G.state_dict())
    torch.manual_seed(seed + 1)
    zs = G.get_zs(b)
    kw = dict(KW, num_steps=S, hierarchical_sample=hier, psi=1.)
    hg = HeadGates(G)
    try:
        with Capture() as cap:
            imgs, pitch_yaw = G(zs, img_size=img_size, nerf_noise=nerf_noise, return_aux_img=aux, grad_points=grad_points,
                                forward_points=None, **kw)
    finally:
        hg.close()
    per = (["noise_c", "u"] if hier else []) + ["noise_f"]
    if grad_points is None:
        names = ["jitter", "theta", "phi"] + per
    else:
        names = ["jitter", "theta", "phi", "rand_idx"] + [n + "_grad" for n in per] + [n + "_rest" for n in per]
    assert len(cap.draws) == len(names), (len(cap.draws), names)
    rand = {n: t for n, (_, t) in zip(names, cap.draws)}
    torch.manual_seed(4321)
    G0 = torch.randn_like(imgs) / imgs.numel()
    (imgs * G0).sum().backward()
    fix = dict(tag=tag, seed=seed, b=b, img_size=img_size, S=S, hier=hier, nerf_noise=nerf_noise, aux=aux, freeze=freeze,
               grad_points=grad_points, G_kwargs=kw, state_checksums=sums, zs={k: v.clone() for k, v in zs.items()},
               rand=rand, G0=G0, imgs=imgs.detach().clone(), pitch_yaw=pitch_yaw.detach().clone(),
               grads=grad_digest(G.named_parameters()))
    _save(tag, fix, imgs)
    save_gates(tag, hg.gates, "imgs", imgs.detach())


def make_eval_psi_staged_case(tag, seed, b, img_size, S, psi, forward_points, aux):
    """psi < 1 (generate_avg_frequencies over 10 000 latents: the averaged nerf_rgb is nerf_rgb_mapping's output) and the
    staged no-grad forward in chunks of `forward_points` pixels, with its per-image / per-chunk draw order"""
    torch.manual_seed(seed)
    G = ref_v1.GeneratorNerfINR(**g_cfg(), device="cpu")
    G.eval()
    sums = checksums(G.state_dict())
    torch.manual_seed(seed + 1)
    zs = G.get_zs(b)
    n = img_size * img_size
    kw = dict(KW, num_steps=S, hierarchical_sample=True, psi=psi, clamp_mode="relu", last_back=True, white_back=False,
              h_mean=math.pi * 0.5, v_mean=math.pi * 0.5)
    with Capture() as cap, torch.no_grad():
        imgs, pitch_yaw = G(zs, img_size=img_size, nerf_noise=0.0, return_aux_img=aux, grad_points=None,
                            forward_points=forward_points, **kw)
    (_, azn), (_, azi) = cap.draws[0], cap.draws[1]
    assert azn.shape == (10000, 256) and azi.shape == (10000, 512)
    # the 10 000 latents are not stored: they are the next two CPU draws after get_zs(b) under seed + 1
    fix_avg = dict(z_checksums=checksums(dict(z_nerf=azn, z_inr=azi)),
                   styles={k: v.detach().clone() for k, v in G.avg_styles.items()})
    js, ths, phs, ncs, us, nfs = [], [], [], [], [], []
    it = iter(cap.draws[2:])
    for _ in range(b):
        js.append(next(it)[1]); ths.append(next(it)[1]); phs.append(next(it)[1])
        head = 0
        while head < n:
            ncs.append(next(it)[1]); us.append(next(it)[1]); nfs.append(next(it)[1])
            head += forward_points
    assert next(it, None) is None, "unconsumed reference draws"
    rand = dict(jitter=torch.cat(js, 0), theta=torch.cat(ths, 0), phi=torch.cat(phs, 0),
                noise_c=torch.cat(ncs, 1).reshape(b, n, S, 1), u=torch.cat(us, 0),
                noise_f=torch.cat(nfs, 1).reshape(b, n, 2 * S, 1))
    fix = dict(tag=tag, seed=seed, b=b, img_size=img_size, S=S, hier=True, nerf_noise=0.0, aux=aux, freeze=False,
               forward_points=forward_points, camera=None, G_kwargs=kw, state_checksums=sums,
               zs={k: v.clone() for k, v in zs.items()}, avg=fix_avg, rand=rand, imgs=imgs.detach().clone(),
               pitch_yaw=pitch_yaw.detach().clone())
    _save(tag, fix, imgs)


def make_reference_layout_v1():
    from tl2.proj.fvcore import build_model
    torch.manual_seed(0)
    G = build_model(CFG["G_cfg_3D2D"], device="cpu")
    assert type(G) is ref_v1.GeneratorNerfINR
    out = {"G_cfg_3D2D": dict(CFG["G_cfg_3D2D"]),
           "G_state": [(k, tuple(v.shape), str(v.dtype).replace("torch.", "")) for k, v in G.state_dict().items()],
           "num_params": sum(p.numel() for p in G.parameters()), "module_name_list": list(G.module_name_list),
           "mapping_inr_heads": list(G.mapping_network_inr.head_dim_dict), "siren_styles": list(G.siren.style_dim_dict)}
    path = os.path.join(OUT, "reference_layout_v1.pt")
    torch.save(out, path)
    print("reference layout v1 ->", path, os.path.getsize(path) // 1024, "KiB", len(out["G_state"]), "keys",
          out["num_params"], "parameters")


def main():
    os.makedirs(OUT, exist_ok=True)
    make_reference_layout_v1()
    make_train_case("g_v1_r16_hier", seed=1301, b=2, img_size=16, S=6, hier=True, nerf_noise=0.0, aux=True)
    make_train_case("g_v1_r16_part", seed=1302, b=2, img_size=16, S=5, hier=True, nerf_noise=0.2, aux=True, grad_points=96)
    make_train_case("g_v1_r8_freeze", seed=1303, b=2, img_size=8, S=4, hier=True, nerf_noise=0.0, aux=False, freeze=True)
    make_eval_psi_staged_case("g_v1_r8_eval_psi_staged", seed=1304, b=2, img_size=8, S=4, psi=0.7, forward_points=24,
                              aux=True)


if __name__ == "__main__":
    main()
