"""An fp64 yardstick for the feature-volume renderer (csrc/volume.hip, cips_feature_volume_render in include/cips3d_hip.h) BY REUSE
of tests/volume_oracle.py: the rule is the rgb renderer's with 32 channels in place of 3, every channel is treated alike and the
error bars of volume_oracle.render are per channel, so the 32-channel render is eleven calls of volume_oracle.render(case,
bars=True), each carrying three feature channels in the `rgb` slot (the last triple is channels 30, 31 and a plane of zeros).
depth, opacity, near and sees do not depend on the colours: they come from the first call.  Nothing is restated here, and
nothing comes from the code under test.

Cases: the geometry, sigma and flags of volume_oracle.cases() with seeded features, uniform in [-1, 1] and independent per
channel.  NAMES covers partial tiles (5 x 7 images), S = 2, Bv = 1 under b = 3 (turntable), Bv = b = 2 (pairs), the camera inside
the box, and a complete miss.

Two deliberately wrong rules, for tests/test_feature_volume_oracle_cpu.py:
  "wrong_group"  channel c is read from channel c ^ 4 (the neighbouring group's record)
  "top_up_3"     last_back's top-up and white_back's background reach only channels 0..2"""
import functools
import zlib
from types import SimpleNamespace

import torch

import volume_oracle as vo

C = 32
NAMES = ("outside_5x7_s12_relu", "outside_16_s12_softplus_last", "outside_16_s2_relu_white", "inside_16_s12_relu_last_white",
         "miss_5x7_s12_relu_white", "corner_16_s12_relu_last", "turntable_16_s12_relu", "inside_16_s12_relu_last_smooth",
         "pairs_5x7_s12_softplus_last")
VARIANTS = (None, "wrong_group", "top_up_3")


def random_features(seed, Bv, nx, ny, nz):
    """seeded: (Bv,nx,ny,nz,32) uniform in [-1, 1]"""
    return torch.rand(Bv, nx, ny, nz, C, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def with_features(base, feat):
    """a volume_oracle case and features (Bv,nx,ny,nz,32) on its lattice -> the feature case (the base's fields and .feat)"""
    assert feat.shape == (*base.sigma.shape, C)
    return SimpleNamespace(**{**vars(base), "feat": feat})


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for name in NAMES:
        base = vo.cases()[name]
        out[name] = with_features(base, random_features(zlib.crc32(name.encode()), *base.sigma.shape))
    return out


def render(case, dtype=torch.float64, variant=None, bars=False):
    """The rule in `dtype` arithmetic -> SimpleNamespace(fea (b,H*W,32), depth (b,1,H,W), opacity (b,1,H,W), sees (b,H,W)); with
    bars=True (fp64, the right rule) also bar_fea, bar_depth, bar_opacity and near (b,H,W)."""
    assert variant in VARIANTS and not (bars and (variant is not None or dtype != torch.float64))
    feat = case.feat
    if variant == "wrong_group":
        feat = feat[..., torch.arange(C) ^ 4]
    feat = torch.cat([feat, torch.zeros_like(feat[..., :1])], -1)                    # 33 channels: eleven triples
    parts = []
    for t in range(11):
        sub = SimpleNamespace(**{**vars(case), "rgb": feat[..., 3 * t:3 * t + 3].contiguous()})
        wrong = None
        if variant == "top_up_3" and t > 0:
            sub.white_back, wrong = False, ("no_top_up" if case.last_back else None)
        parts.append(vo.render(sub, dtype=dtype, variant=wrong, bars=bars))
    first = parts[0]
    b = case.cam2world.shape[0]
    rows = lambda key: torch.cat([getattr(p, key) for p in parts], 1)[:, :C].reshape(b, C, case.H * case.W).transpose(1, 2).contiguous()
    out = SimpleNamespace(fea=rows("rgb"), depth=first.depth, opacity=first.opacity, sees=first.sees)
    if bars:
        out.bar_fea, out.bar_depth, out.bar_opacity, out.near = rows("bar_rgb"), first.bar_depth, first.bar_opacity, first.near
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the fp64 oracle of a case with its bars: computed once, shared, never modified"""
    return render(cases()[name], bars=True)


def compare(ref, fea, depth, opacity):
    """outputs of any dtype / device against render(bars=True) -> SimpleNamespace(fea, depth, opacity: the largest |err| / bar over
    the pixels that are not near (0 where err and bar are both 0, inf where only the bar is), over (b,H,W): err > bar for any
    output or channel, near pixels False)"""
    b, H, W = ref.near.shape
    keep = ~ref.near
    worst, over = {}, torch.zeros_like(ref.near)
    for name, got, want, bar in (("fea", fea, ref.fea, ref.bar_fea), ("depth", depth, ref.depth, ref.bar_depth),
                                 ("opacity", opacity, ref.opacity, ref.bar_opacity)):
        err = (got.detach().cpu().double() - want).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bar)
        # per pixel, the worst channel: fea is pixel-major (b,H*W,32), the maps are (b,1,H,W)
        ratio = ratio.amax(-1).view(b, H, W) if name == "fea" else ratio.view(b, H, W)
        ratio = torch.where(keep, ratio, torch.zeros_like(ratio))
        worst[name] = float(ratio.max()) if ratio.numel() else 0.0
        over |= ratio > 1
    return SimpleNamespace(over=over, **worst)
