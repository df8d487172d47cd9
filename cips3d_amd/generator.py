"""MI355X-native drop-in for the reference generator API (exp/cips3d/models/generator.py).

Same constructor / forward signatures, attribute names and state_dict layout as
`GeneratorNerfINR` (generator.py:1159-1951) and `GeneratorNerfINR_freeze_NeRF` (:1955-2083), so
checkpoints and `exp/cips3d` scripts work unchanged; the arithmetic runs in the hand-written
HIP kernels of libcips3d_hip.so (see ops.py / include/cips3d_hip.h).  Modules here only HOLD
parameters (same names, shapes and initialisers, created in the reference's order so that the
same torch seed yields the same initial weights) and orchestrate kernel launches.
"""
import math
import os
import random
from collections import OrderedDict
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops


# ------------------------------------------------------------------------------------------
# initialisers (film_layer.py:11-18, inr_network.py:20-27, tl2 init_func.kaiming_leaky_init)
# ------------------------------------------------------------------------------------------
def frequency_init(freq):
    def init(m):
        with torch.no_grad():
            if isinstance(m, nn.Linear):
                num_input = m.weight.size(-1)
                m.weight.uniform_(-np.sqrt(6 / num_input) / freq, np.sqrt(6 / num_input) / freq)
    return init


def kaiming_leaky_init(m):
    if m.__class__.__name__.find('Linear') != -1:
        torch.nn.init.kaiming_normal_(m.weight, a=0.2, mode='fan_in', nonlinearity='leaky_relu')


# ------------------------------------------------------------------------------------------
# parameter holders
# ------------------------------------------------------------------------------------------
class PixelNorm(nn.Module):
    """multi_head_mapping.py:13-19"""

    def forward(self, input):
        assert input.dim() == 2
        return input * torch.rsqrt(torch.mean(input ** 2, dim=1, keepdim=True) + 1e-8)


class MultiHeadMappingNetwork(nn.Module):
    """z -> style MLP (multi_head_mapping.py:28-153).  Tiny (b x 512) GEMMs: stays on
    torch/rocBLAS; must remain differentiable and state-dict compatible."""

    def __init__(self, z_dim, hidden_dim, base_layers, head_layers, head_dim_dict,
                 add_norm=False, norm_out=False, **kwargs):
        super().__init__()
        self.z_dim = z_dim
        self.head_dim_dict = head_dim_dict
        out_dim = z_dim
        self.module_name_list = []
        self.norm = PixelNorm()
        base_net = []
        for i in range(base_layers):
            in_dim = out_dim
            out_dim = hidden_dim
            layer = nn.Linear(in_features=in_dim, out_features=out_dim)
            layer.apply(kaiming_leaky_init)
            base_net.append(layer)
            if head_layers > 0 or i != base_layers - 1:
                if add_norm:
                    base_net.append(nn.LayerNorm(out_dim))
                base_net.append(nn.LeakyReLU(0.2, inplace=True))
        if len(base_net) > 0:
            if norm_out and head_layers <= 0:
                base_net.append(nn.LayerNorm(out_dim))
            self.base_net = nn.Sequential(*base_net)
            self.num_z = 1
            self.module_name_list.append('base_net')
        else:
            self.base_net = None
            self.num_z = len(head_dim_dict)
        head_in_dim = out_dim
        for name, head_dim in head_dim_dict.items():
            if head_layers > 0:
                head_net = []
                out_dim = head_in_dim
                for i in range(head_layers):
                    in_dim = out_dim
                    out_dim = head_dim if i == head_layers - 1 else hidden_dim
                    hl = nn.Linear(in_features=in_dim, out_features=out_dim)
                    hl.apply(kaiming_leaky_init)
                    head_net.append(hl)
                    if i != head_layers - 1:
                        head_net.append(nn.LeakyReLU(0.2, inplace=True))
                    elif norm_out:
                        head_net.append(nn.LayerNorm(out_dim))
                head_net = nn.Sequential(*head_net)
                self.module_name_list.append(name)
            else:
                head_net = nn.Identity()
            self.add_module(name, head_net)

    def _base_hip(self, z):
        """base_net on the HIP kernels: PixelNorm, then per layer the Linear (grouped-linear kernel, one job) and one
        fused LayerNorm / LeakyReLU launch (cips_rownorm_*) instead of three torch modules"""
        x = ops.RowNormFunction.apply(z, None, None, 4)
        mods = list(self.base_net)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, nn.Linear):
                x = ops.grouped_linear([(x, m)])[0]
                i += 1
                ln = mods[i] if i < len(mods) and isinstance(mods[i], nn.LayerNorm) else None
                if ln is not None:
                    i += 1
                act = i < len(mods) and isinstance(mods[i], nn.LeakyReLU)
                if act:
                    i += 1
                if ln is not None or act:
                    x = ops.RowNormFunction.apply(x, ln.weight if ln is not None else None, ln.bias if ln is not None else None,
                                                  (1 if ln is not None else 0) | (2 if act else 0))
            else:               # anything else the constructor could have put here
                x = m(x)
                i += 1
        return x

    def _hip_ok(self, z):
        # (large batches — the 10 000 latents of generate_avg_frequencies — stay on hipBLASLt: the row kernels are built for
        # the few rows of a training batch)
        return (z.is_cuda and z.dim() == 2 and z.dtype == torch.float32 and z.shape[0] <= 256 and z.shape[1] <= 512 and z.shape[1] % 4 == 0
                and all(not isinstance(m, nn.Linear) or (m.in_features <= 512 and m.in_features % 4 == 0 and m.out_features <= 1024)
                        for m in self.base_net))

    def forward(self, z):
        if self.base_net is not None:
            if self._hip_ok(z):
                base_fea = self._base_hip(z)
            else:
                z = self.norm(z)
                base_fea = self.base_net(z)
            head_inputs = {name: base_fea for name in self.head_dim_dict.keys()}
        else:
            head_inputs = {name: self.norm(z[idx]) for idx, name in enumerate(self.head_dim_dict.keys())}
        return {name: getattr(self, name)(head_inputs[name]) for name in self.head_dim_dict.keys()}


class FiLMLayer(nn.Module):
    """Parameters of film_layer.FiLMLayer (film_layer.py:41-107); the sine layer itself is
    evaluated inside the fused SIREN kernel."""

    def __init__(self, in_dim, out_dim, style_dim, use_style_fc=True, **kwargs):
        super().__init__()
        assert use_style_fc
        self.in_dim, self.out_dim, self.style_dim, self.use_style_fc = in_dim, out_dim, style_dim, use_style_fc
        self.linear = nn.Linear(in_dim, out_dim)
        self.linear.apply(frequency_init(25))
        self.gain_fc = nn.Linear(style_dim, out_dim)
        self.bias_fc = nn.Linear(style_dim, out_dim)
        self.gain_fc.weight.data.mul_(0.25)
        self.bias_fc.weight.data.mul_(0.25)

    def film(self, style):
        """gain = 15 * gain_fc(style) + 30 (LinearScale, film_layer.py:21-32, :59), bias = bias_fc(style)."""
        return self.gain_fc(style) * 15 + 30, self.bias_fc(style)


def _film_all(layers, styles):
    """FiLM vectors of several layers in one grouped launch: -> [(gain, bias), ...]"""
    ys = ops.grouped_linear([(st, m) for lay, st in zip(layers, styles) for m in (lay.gain_fc, lay.bias_fc)])
    return [(ys[2 * i] * 15 + 30, ys[2 * i + 1]) for i in range(len(layers))]


class NeRFNetwork(nn.Module):
    """generator.py:151-340.  forward() keeps the reference op boundary ((b,P,3) -> (b,P,33));
    the generator uses `evaluate()` which returns feat / sigma separately (no 33-wide cat)."""

    def __init__(self, in_dim=3, hidden_dim=256, hidden_layers=2, style_dim=512, rgb_dim=3, device=None,
                 name_prefix='nerf', **kwargs):
        super().__init__()
        if not (in_dim == 3 and rgb_dim == 32 and hidden_layers >= 1):
            raise NotImplementedError(
                "the ray set-up produces 3-vectors and the composite / CIPS head take 32 colour features "
                "(in_dim 3, rgb_dim 32: every shipped config, ffhq_exp.yaml:51-58)")
        # the fused SIREN kernels hold exactly the shipped matrices in LDS (hidden 128, two FiLM layers); any other width or depth
        # runs the same arithmetic as plain GPU tensor operations (hipBLASLt linears + elementwise sine, torch autograd) through
        # the unfused rays -> SIREN -> composite path: functional parity with the reference module, not its speed
        self.fused = hidden_dim == 128 and hidden_layers == 2
        self.device = device
        self.in_dim, self.hidden_dim, self.rgb_dim = in_dim, hidden_dim, rgb_dim
        self.style_dim, self.hidden_layers, self.name_prefix = style_dim, hidden_layers, name_prefix
        self.module_name_list = []
        self.style_dim_dict = {}
        self.network = nn.ModuleList()
        self.module_name_list.append('network')
        _out = in_dim
        for idx in range(hidden_layers):
            _in, _out = _out, hidden_dim
            layer = FiLMLayer(in_dim=_in, out_dim=_out, style_dim=style_dim, use_style_fc=True)
            self.network.append(layer)
            self.style_dim_dict[f'{name_prefix}_w{idx}'] = layer.style_dim
        self.final_layer = nn.Linear(hidden_dim, 1)
        self.module_name_list.append('final_layer')
        self.color_layer_sine = FiLMLayer(in_dim=hidden_dim, out_dim=hidden_dim // 2, style_dim=style_dim,
                                          use_style_fc=True)
        self.style_dim_dict[f'{name_prefix}_rgb'] = self.color_layer_sine.style_dim
        self.module_name_list.append('color_layer_sine')
        self.color_layer_linear = nn.Sequential(nn.Linear(hidden_dim // 2, rgb_dim))
        self.color_layer_linear.apply(kaiming_leaky_init)
        self.module_name_list.append('color_layer_linear')
        self.dim_styles = sum(self.style_dim_dict.values())

    def _evaluate_unfused(self, points, style_dict):
        """generator.py:260-317 for any hidden width / depth: UniformBoxWarp (x 2 / 0.24), FiLM sine layers
        (film_layer.py:78-107: sin(gain * linear(x) + bias)), sigma head, colour sine layer, colour linear."""
        if not points.is_cuda:
            raise RuntimeError("NeRFNetwork runs on the GPU only (there is no CPU path)")
        p = self.name_prefix
        x = points * (2.0 / 0.24)
        for idx, layer in enumerate(self.network):
            gain, bias = layer.film(style_dict[f'{p}_w{idx}'])
            x = torch.sin(gain.unsqueeze(1) * layer.linear(x) + bias.unsqueeze(1))
        sigma = self.final_layer(x).squeeze(-1)
        gain, bias = self.color_layer_sine.film(style_dict[f'{p}_rgb'])
        c = torch.sin(gain.unsqueeze(1) * self.color_layer_sine.linear(x) + bias.unsqueeze(1))
        return self.color_layer_linear(c), sigma

    def _siren_args(self, style_dict):
        """the 16 tensors of the fused SIREN Functions in their order (ops._SIREN_NAMES): the FiLM vectors of the three sine
        layers for these styles (one grouped launch), then the ten weights"""
        p = self.name_prefix
        (g0, p0), (g1, p1), (gc, pc) = _film_all([self.network[0], self.network[1], self.color_layer_sine],
                                                 [style_dict[f'{p}_w0'], style_dict[f'{p}_w1'], style_dict[f'{p}_rgb']])
        return (g0, p0, g1, p1, gc, pc,
                self.network[0].linear.weight, self.network[0].linear.bias,
                self.network[1].linear.weight, self.network[1].linear.bias,
                self.final_layer.weight, self.final_layer.bias,
                self.color_layer_sine.linear.weight, self.color_layer_sine.linear.bias,
                self.color_layer_linear[0].weight, self.color_layer_linear[0].bias)

    def evaluate(self, points, style_dict):
        """points (b,P,3) -> feat (b,P,32), sigma (b,P) via the fused HIP kernel (shipped shape) or tensor operations."""
        if not self.fused:
            return self._evaluate_unfused(points, style_dict)
        return ops.SirenFunction.apply(points, *self._siren_args(style_dict))

    def _sigma_args(self, style_dict):
        """_siren_args for the density entry points.  sigma leaves the chain before the colour branch, so it does not depend
        on the colour style: where the styles hold none (generator_v1's NeRF mapping network has no nerf_rgb head) a zero
        style stands in — its FiLM vectors are never read by the sigma-only kernel and do not reach the sigma of the full
        forward either."""
        key = f'{self.name_prefix}_rgb'
        if key not in style_dict:
            b = style_dict[f'{self.name_prefix}_w0'].shape[0]
            style_dict = {**style_dict, key: style_dict[f'{self.name_prefix}_w0'].new_zeros(b, self.color_layer_sine.style_dim)}
        return style_dict

    def _density_call(self, style_dict, fused, unfused):
        """the frame of the density family: no gradient, the styles completed by _sigma_args, then fused(*the 16 SIREN
        tensors) for the shipped shape or unfused(styles) on tensor operations for other widths / depths"""
        with torch.no_grad():
            style_dict = self._sigma_args(style_dict)
            if not self.fused:
                return unfused(style_dict)
            return fused(*self._siren_args(style_dict))

    def density(self, points, style_dict):
        """points (b,P,3) -> sigma (b,P), no gradient: the sigma-only HIP kernel for the shipped shape (the forward's sigma bit
        for bit, without the colour branch), tensor operations for other widths / depths."""
        return self._density_call(style_dict, lambda *siren: ops.siren_sigma(points, *siren),
                                  lambda styles: self._evaluate_unfused(points, styles)[1])

    def density_lattice(self, gx, gy, gz, style_dict):
        """density() over the lattice (gx[i], gy[j], gz[k]) of three 1-D coordinate tensors -> (b, nx, ny, nz); the fused kernel
        reads the coordinates themselves, no points tensor is built"""
        return self._density_call(style_dict, lambda *siren: ops.siren_sigma_grid(gx, gy, gz, *siren),
                                  lambda styles: self._unfused_lattice(gx, gy, gz, styles, False))

    def _unfused_gradient(self, points, style_dict):
        """sigma and d sigma / d points of _evaluate_unfused by autograd (the tensor-operation path of other widths / depths)"""
        with torch.enable_grad():
            pts = points.detach().clone().requires_grad_(True)
            sigma = self._evaluate_unfused(pts, style_dict)[1]
            grad, = torch.autograd.grad(sigma.sum(), pts)
        return sigma.detach(), grad

    def _unfused_lattice(self, gx, gy, gz, style_dict, gradient):
        """the lattice forms on tensor operations: the points are materialised (ops.lattice_points)"""
        b, n = style_dict[f'{self.name_prefix}_w0'].shape[0], (len(gx), len(gy), len(gz))
        pts = ops.lattice_points(gx, gy, gz, b)
        if not gradient:
            return self._evaluate_unfused(pts, style_dict)[1].reshape(b, *n)
        sigma, grad = self._unfused_gradient(pts, style_dict)
        return sigma.reshape(b, *n), grad.reshape(b, *n, 3)

    def density_gradient(self, points, style_dict):
        """points (b,P,3) -> sigma (b,P), d sigma / d points (b,P,3); the outputs carry no grad_fn.  The fused HIP kernel for
        the shipped shape (ops.siren_sigma_grad: sigma is density()'s bit for bit), autograd through the tensor operations for
        other widths / depths."""
        return self._density_call(style_dict, lambda *siren: ops.siren_sigma_grad(points, *siren),
                                  lambda styles: self._unfused_gradient(points, styles))

    def density_gradient_lattice(self, gx, gy, gz, style_dict):
        """density_gradient() over the lattice (gx[i], gy[j], gz[k]) -> (b, nx, ny, nz), (b, nx, ny, nz, 3)"""
        return self._density_call(style_dict, lambda *siren: ops.siren_sigma_grad_grid(gx, gy, gz, *siren),
                                  lambda styles: self._unfused_lattice(gx, gy, gz, styles, True))

    def _unfused_color(self, points, style_dict, proj_w, proj_b, tanh):
        """the colour entry points on tensor operations (other widths / depths) -> rgb (b,P,3), sigma (b,P)"""
        feat, sigma = self._evaluate_unfused(points, style_dict)
        y = F.linear(feat, proj_w, proj_b)
        return (torch.tanh(y) if tanh else y), sigma

    def color(self, points, style_dict, proj_w, proj_b, tanh=True):
        """points (b,P,3) -> rgb (b,P,3) = [tanh](proj_w . feat + proj_b) of evaluate()'s 32 colour features, no gradient: the
        point-colour HIP kernel for the shipped shape (ops.siren_rgb: the projection happens in the forward kernel's registers,
        neither the features nor a second launch exist), tensor operations for other widths / depths.  proj_w (3,32), proj_b
        (3): GeneratorNerfINR's auxiliary RGB layer, or any 32 -> 3 map.  Unlike the density family it needs the colour style."""
        with torch.no_grad():
            if not self.fused:
                return self._unfused_color(points, style_dict, proj_w, proj_b, tanh)[0]
            return ops.siren_rgb(points, proj_w, proj_b, *self._siren_args(style_dict), tanh=tanh)

    def color_lattice(self, gx, gy, gz, style_dict, proj_w, proj_b, tanh=True, sigma=False):
        """color() over the lattice (gx[i], gy[j], gz[k]) of three 1-D coordinate tensors -> rgb (b, nx, ny, nz, 3), with
        sigma=True (rgb, sigma (b, nx, ny, nz)), sigma density_lattice()'s bit for bit; the fused kernel reads the coordinates
        themselves, no points tensor is built"""
        with torch.no_grad():
            if self.fused:
                return ops.siren_rgb_grid(gx, gy, gz, proj_w, proj_b, *self._siren_args(style_dict), tanh=tanh, sigma=sigma)
            b, n = style_dict[f'{self.name_prefix}_w0'].shape[0], (len(gx), len(gy), len(gz))
            rgb, sig = self._unfused_color(ops.lattice_points(gx, gy, gz, b), style_dict, proj_w, proj_b, tanh)
            return (rgb.reshape(b, *n, 3), sig.reshape(b, *n)) if sigma else rgb.reshape(b, *n, 3)

    def surface_rays(self, style_dict, geom, xg, yg, zg, cam2world, level, refine):
        """The iso-surface sigma = level along the unjittered camera rays -> depth (b,n), hit (b,n) uint8, sigma (b,n), points
        (b,n,3), no gradient (the rule: ops.siren_surface).  The ray-cast HIP kernel for the shipped shape on the split-operand
        chain; the same search composed from sigma evaluations (ops.siren_surface_composed) for the exact-fp32 forward
        (CIPS_SIREN_FWD=f32) and, on tensor operations, for other widths / depths."""
        rays = (level, refine, geom, xg, yg, zg, cam2world)
        return self._density_call(
            style_dict,
            lambda *siren: (ops.siren_surface if ops.SIREN_FWD_MODE == "x3" else ops.siren_surface_composed)(*rays, *siren),
            lambda styles: ops.siren_surface_composed(*rays, sigma_fn=lambda p: self._evaluate_unfused(p, styles)[1]))

    def evaluate_rays(self, style_dict, geom, xg, yg, zg, cam2world, jitter=None, zvals=None):
        """evaluate() with the sample points generated in-kernel (coarse: from the jitter draw; fine: from the resampled
        depths `zvals`) -> feat (b,P,32), sigma (b,P), z (b,P)"""
        return ops.SirenRaysFunction.apply(geom, xg, yg, zg, cam2world, jitter, zvals, *self._siren_args(style_dict))

    def march(self, style_dict, geom, xg, yg, zg, cam2world, jitter, noise, geo=False):
        """fused rays + SIREN + composite for non-hierarchical sampling -> pixels_fea (b,n,32), depth (b,n); with `geo` also
        opacity (b,n), and depth and opacity are differentiable (ops.RayMarchGeoFunction)"""
        fn = ops.RayMarchGeoFunction if geo else ops.RayMarchFunction
        return fn.apply(geom, xg, yg, zg, cam2world, jitter, noise, *self._siren_args(style_dict))

    def forward(self, input, style_dict, ray_directions=None, **kwargs):
        feat, sigma = self.evaluate(input, style_dict)
        return torch.cat([feat, sigma.unsqueeze(-1)], dim=-1)

    forward_with_frequencies_phase_shifts = forward


class SinStyleMod(nn.Module):
    """Parameters of mod_conv_fc.SinStyleMod (mod_conv_fc.py:392-450).  `norm` exists in the
    reference state_dict but is never used in forward (:444-445)."""

    def __init__(self, in_channel, out_channel, kernel_size=1, style_dim=None, use_style_fc=False,
                 demodulate=True, eps=1e-8, **kwargs):
        super().__init__()
        assert kernel_size == 1 and use_style_fc and demodulate
        self.eps, self.in_channel, self.out_channel, self.style_dim = eps, in_channel, out_channel, style_dim
        self.weight = nn.Parameter(torch.randn(1, in_channel, out_channel))
        torch.nn.init.kaiming_normal_(self.weight[0], a=0.2, mode='fan_in', nonlinearity='leaky_relu')
        self.modulation = nn.Linear(style_dim, in_channel)
        self.modulation.apply(kaiming_leaky_init)
        self.norm = nn.LayerNorm(in_channel)


class SinBlock(nn.Module):
    """generator.py:893-980 (two modulated FCs + LeakyReLU(0.2), optional skip)."""

    def __init__(self, in_dim, out_dim, style_dim, name_prefix):
        super().__init__()
        self.in_dim, self.out_dim, self.style_dim, self.name_prefix = in_dim, out_dim, style_dim, name_prefix
        self.style_dim_dict = {}
        self.mod1 = SinStyleMod(in_channel=in_dim, out_channel=out_dim, style_dim=style_dim, use_style_fc=True)
        self.style_dim_dict[f'{name_prefix}_0'] = self.mod1.style_dim
        self.mod2 = SinStyleMod(in_channel=out_dim, out_channel=out_dim, style_dim=style_dim, use_style_fc=True)
        self.style_dim_dict[f'{name_prefix}_1'] = self.mod2.style_dim


class ToRGB(nn.Module):
    """generator.py:983-1006"""

    def __init__(self, in_dim, dim_rgb=3, use_equal_fc=False):
        super().__init__()
        assert not use_equal_fc
        self.in_dim, self.dim_rgb = in_dim, dim_rgb
        self.linear = nn.Linear(in_dim, dim_rgb)


class CIPSNet(nn.Module):
    """generator.py:1009-1154.  NOTE (reference behaviour): `points_forward` calls
    `self.inr_net(pixels_fea, style_dict)` WITHOUT img_size (generator.py:1754), so the default
    img_size=1024 applies and ALL nine blocks "4".."1024" run at every resolution."""

    def __init__(self, input_dim, style_dim, hidden_dim=256, pre_rgb_dim=32, device=None, name_prefix='inr',
                 **kwargs):
        super().__init__()
        if pre_rgb_dim != 3:
            raise NotImplementedError("shipped configs use pre_rgb_dim 3 (ffhq_exp.yaml:72)")
        self.device, self.pre_rgb_dim, self.name_prefix = device, pre_rgb_dim, name_prefix
        self.channels = {str(2 ** i): hidden_dim for i in range(2, 11)}
        self.module_name_list = []
        self.style_dim_dict = {}
        _out = input_dim
        network, to_rgbs = OrderedDict(), OrderedDict()
        for name, channel in self.channels.items():
            _in, _out = _out, channel
            blk = SinBlock(in_dim=_in, out_dim=_out, style_dim=style_dim, name_prefix=f'{name_prefix}_w{name}')
            self.style_dim_dict.update(blk.style_dim_dict)
            network[name] = blk
            to_rgbs[name] = ToRGB(in_dim=_out, dim_rgb=pre_rgb_dim, use_equal_fc=False)
        self.network = nn.ModuleDict(network)
        self.to_rgbs = nn.ModuleDict(to_rgbs)
        self.to_rgbs.apply(frequency_init(100))
        self.module_name_list += ['network', 'to_rgbs']
        self.tanh = nn.Sequential(nn.Tanh())
        self.module_name_list.append('tanh')

    def _names(self, img_size):
        img_size = str(2 ** int(np.log2(img_size)))
        names = []
        for name in self.network.keys():
            names.append(name)
            if name == img_size:
                break
        return names

    def _build_params(self, names, style_dict):
        # s = SinStyleMod.modulation(style) of all 18 layers (mod_conv_fc.py:474) in one grouped launch
        mods = ops.grouped_linear([(style_dict[f'{self.network[name].name_prefix}_{j}'], m.modulation)
                                   for name in names for j, m in enumerate((self.network[name].mod1, self.network[name].mod2))])
        params = []
        for k, name in enumerate(names):
            blk = self.network[name]
            # (1, in, out) -> (in, out) as a VIEW: indexing with [0] makes autograd materialise a zero-filled (1, in, out)
            # buffer and copy the gradient into it, 18 x (fill + 1 MiB copy) per step
            w1, w2 = blk.mod1.weight, blk.mod2.weight
            params += [w1.view(w1.shape[1], w1.shape[2]), mods[2 * k], w2.view(w2.shape[1], w2.shape[2]), mods[2 * k + 1]]
        for idx, name in enumerate(names):
            if idx >= 3:
                params += [self.to_rgbs[name].linear.weight, self.to_rgbs[name].linear.bias]
        return mods, params

    def open_tail_ports(self, style_dict, B, n, in0, img_size=1024, join=True):
        """The head's weight-gradient tail behind gradient ports on the side stream (ops.INR_TAIL), opened for the NEXT forward()
        with these styles and (B, n, in0) inputs.  Every autograd node between the ports and the parameters — the modulation
        Linears, the weight views — is created under that stream as well (a node on the caller's stream that consumed a port's
        output would make the caller's stream wait for the whole tail).  GeneratorNerfINR._render calls this first, BEFORE the ray march:
        nodes created earlier run later in the backward pass, so the NeRF backward is issued first and the tail starts behind
        its compositing kernel (ops._TAIL_GATE).  Returns True when ports are pending."""
        self._tail = None
        dev = next(self.parameters()).device
        names = self._names(img_size)
        if not (dev.type == "cuda" and B <= 64 and torch.is_grad_enabled() and ops.INR_TAIL == "side" and len(names) > 3):
            return False
        side = _side_stream(dev)
        main = torch.cuda.current_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            mods, params = self._build_params(names, style_dict)
        for t in mods:
            t.record_stream(main)
        ok = ops.inr_head_ports_ok(len(names), B, n, in0, params, dev)
        ports = ops.inr_head_open_ports(len(names), B, n, params, side) if ok else None
        if join:
            main.wait_stream(side)
        # (not ok: the modulation Linears are kept all the same — forward() takes its parameters from here)
        self._tail = dict(key=(B, n, in0, len(names)), styles=style_dict, params=params, ports=ports)
        return True

    def forward(self, input, style_dict, img_size=1024, **kwargs):
        names = self._names(img_size)
        tail, self._tail = getattr(self, "_tail", None), None
        key = (input.shape[0], input.shape[1], input.shape[2], len(names))
        if (tail is None and torch.is_grad_enabled() and input.is_cuda and input.requires_grad
                and self.open_tail_ports(style_dict, *key[:3], img_size=img_size)):
            tail, self._tail = self._tail, None          # not opened ahead (a direct call): open them now
        if tail is not None and tail["key"] == key and tail["styles"] is style_dict and torch.is_grad_enabled():
            if tail["ports"] is not None:
                rgb = ops.inr_head_with_ports(len(names), input, tail["params"], tail["ports"])
            else:
                rgb = ops.inr_head(len(names), input, *tail["params"])
        else:
            _, params = self._build_params(names, style_dict)
            rgb = ops.inr_head(len(names), input, *params)
        return self.tanh(rgb)


class _ToRGBFunction(torch.autograd.Function):
    """y (M,3) = x (M,K) @ w^T + b on the HIP ToRGB kernels (used for the aux 32->3 head)."""

    @staticmethod
    def forward(ctx, x, w, b):
        x2 = x.detach().contiguous().view(-1, x.shape[-1])
        w, b = w.detach().contiguous(), b.detach().contiguous()
        y = torch.empty(x2.shape[0], 3, device=x.device)
        ops.torgb_fwd(x2, w, b, y, accumulate=False)
        ctx.save_for_backward(x2, w)
        ctx.shape = x.shape
        return y.view(*x.shape[:-1], 3)

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.contiguous().view(-1, 3)
        dw, db = ops.torgb_bwd_w(x2, dy2)
        dx = torch.empty_like(x2)
        ops.torgb_bwd_x(dy2, w, None, None, None, dx)
        return dx.view(ctx.shape), dw, db


# The INR mapping MLP runs on a side stream.  Measured on one box, C2: 17.15 -> 16.79 ms per step (graph replay), 17.22 ->
# 16.88 eager against everything on the caller's stream.
_SIDE_STREAMS = {}


def _side_stream(device):
    key = torch.device(device).index
    s = _SIDE_STREAMS.get(key)
    if s is None:
        s = _SIDE_STREAMS[key] = torch.cuda.Stream(device=device)
    return s


# ------------------------------------------------------------------------------------------
# camera helpers (O(batch) host-side math; comm_utils.py:451-581)
# ------------------------------------------------------------------------------------------
def _normalize(v):
    return v / torch.norm(v, dim=-1, keepdim=True)


def camera_origin_from_angles(theta, phi, r=1.0):
    """comm_utils.py:527-535 (phi already drawn; clamp + spherical -> cartesian)."""
    phi = torch.clamp(phi, 1e-5, math.pi - 1e-5)
    out = torch.zeros((theta.shape[0], 3), device=theta.device)
    out[:, 0:1] = r * torch.sin(phi) * torch.cos(theta)
    out[:, 2:3] = r * torch.sin(phi) * torch.sin(theta)
    out[:, 1:2] = r * torch.cos(phi)
    return out, phi


def _truncated_normal(shape, device):
    """comm_utils.py:441-448: per element the first of four standard-normal draws that lies in (-2, 2) (the first
    draw if none does)."""
    tmp = torch.randn(tuple(shape) + (4,), device=device)      # = empty().normal_(): the same draws
    ok = (tmp < 2) & (tmp > -2)
    first = ok.max(-1, keepdim=True)[1]
    return tmp.gather(-1, first).squeeze(-1)


def sample_camera_positions(device, bs=1, r=1, horizontal_stddev=1, vertical_stddev=1, horizontal_mean=math.pi * 0.5,
                            vertical_mean=math.pi * 0.5, mode='normal'):
    """comm_utils.py:451-535: camera origins on the sphere of radius r -> (origin (bs,3), phi = pitch (bs,1),
    theta = yaw (bs,1)), every distribution of the reference with its draws in the reference's order
    (yaw first; 'hybrid' flips Python's `random.random()` first; anything else is an assertion error)."""
    hs, vs, hm, vm = horizontal_stddev, vertical_stddev, horizontal_mean, vertical_mean
    u = lambda: torch.rand((bs, 1), device=device)
    g = lambda: torch.randn((bs, 1), device=device)
    if mode == 'uniform':
        theta = (u() - 0.5) * 2 * hs + hm
        phi = (u() - 0.5) * 2 * vs + vm
    elif mode in ('normal', 'gaussian'):
        theta = g() * hs + hm
        phi = g() * vs + vm
    elif mode == 'hybrid':
        if random.random() < 0.5:
            theta = (u() - 0.5) * 2 * hs * 2 + hm
            phi = (u() - 0.5) * 2 * vs * 2 + vm
        else:
            theta = g() * hs + hm
            phi = g() * vs + vm
    elif mode == 'truncated_gaussian':
        theta = _truncated_normal((bs, 1), device) * hs + hm
        phi = _truncated_normal((bs, 1), device) * vs + vm
    elif mode == 'spherical_uniform':
        theta = (u() - 0.5) * 2 * hs + hm
        v = (u() - 0.5) * 2 * (vs / math.pi) + vm / math.pi
        phi = torch.arccos(1 - 2 * torch.clamp(v, 1e-5, 1 - 1e-5))
    elif mode == 'mean':
        theta = torch.ones((bs, 1), device=device) * hm
        phi = torch.ones((bs, 1), device=device) * vm
    else:
        assert 0, f"camera distribution {mode!r}"
    origin, phi = camera_origin_from_angles(theta, phi, r)
    return origin, phi, theta


def create_cam2world_matrix(forward_vector, origin, up_vector=None):
    """comm_utils.py:538-581"""
    device = origin.device
    forward_vector = _normalize(forward_vector)
    if up_vector is None:
        # (0, 1, 0) built on the device — no host-to-device copy, so the step can be captured in a hipGraph
        up_vector = (torch.arange(3, device=device) == 1).to(torch.float).expand_as(forward_vector)
    left_vector = _normalize(torch.cross(up_vector, forward_vector, dim=-1))
    up_vector = _normalize(torch.cross(forward_vector, left_vector, dim=-1))
    rot = torch.eye(4, device=device).unsqueeze(0).repeat(forward_vector.shape[0], 1, 1)
    rot[:, :3, :3] = torch.stack((-left_vector, up_vector, -forward_vector), axis=-1)
    trans = torch.eye(4, device=device).unsqueeze(0).repeat(forward_vector.shape[0], 1, 1)
    trans[:, :3, 3] = origin
    return trans @ rot


# ------------------------------------------------------------------------------------------
# the render path's settings, random draws and camera (no kernels of the NeRF path: these run on a CPU device too)
# ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class RenderSettings:
    """What an entry point of GeneratorNerfINR was asked for, built once there (RenderSettings.of) and handed down."""
    img_size: int
    fov: float
    ray_start: float
    ray_end: float
    num_steps: int
    h_stddev: float
    v_stddev: float
    h_mean: float
    v_mean: float
    hierarchical_sample: bool
    sample_dist: str = None
    clamp_mode: str = 'relu'
    nerf_noise: float = 0.
    white_back: bool = False
    last_back: bool = False
    return_aux_img: bool = False
    forward_points: int = None
    grad_points: int = None
    camera_pos: torch.Tensor = None
    camera_lookup: torch.Tensor = None
    up_vector: torch.Tensor = None
    rand_override: dict = None          # any of jitter/theta/phi/noise_c/u/noise_f(/rand_idx): fixed draws for parity tests

    n = property(lambda s: s.img_size ** 2)                                                  # rays per image
    E = property(lambda s: 2 * s.num_steps if s.hierarchical_sample else s.num_steps)        # composited samples per ray
    flags = property(lambda s: (1 if s.last_back else 0) | (2 if s.white_back else 0))
    # generator.py:1325-1347: fewer grad_points than pixels is part_grad_forward, which is not handed forward_points
    part = property(lambda s: s.grad_points is not None and s.grad_points < s.n)
    staged = property(lambda s: s.forward_points is not None and not s.part)

    @classmethod
    def of(cls, args, **fixed):
        """The settings of an entry point: the fields it has a parameter for, picked by name out of `args` (its locals():
        whatever else is in there is not a field and is dropped), then `fixed` on top; a field it has no parameter for keeps
        the default above.  What differs between the entry points, all of it:

          entry point                    camera_pos, camera_lookup, up_vector     rand_override    grad_points, forward_points
          forward                        no parameter: never set                  from **kwargs    passed
          forward_camera_pos_and_lookup  set (generator_v1's drops an up_vector)  from **kwargs    passed
          forward_styles                 optional                                 from **kwargs    passed
          render, render_styles          optional                                 named parameter  any value but None: ValueError
          geometry                       optional                                 named parameter  no parameter
          surface                        optional                                 named parameter  no parameter

        Fixed fields: geometry nerf_noise=0. (and it has no return_aux_img parameter); surface hierarchical_sample=False and
        nerf_noise=0. (and no clamp_mode, white_back, last_back or return_aux_img parameter: the defaults)."""
        return cls(**{**{k: v for k, v in args.items() if k in cls.__dataclass_fields__}, **fixed})


def _grad_ctx(nerf_grad):
    return torch.enable_grad() if nerf_grad else torch.no_grad()


# the two kinds of distribution the training configs use keep their raw camera draws separate (rand_override can inject
# them); the others go through sample_camera_positions as a whole
_SIMPLE_CAMS = ('gaussian', 'normal', 'uniform')


def _draw(ro, kind, fn, shape, device):
    """one draw; an overridden one is still drawn (the generator is consumed), then replaced"""
    t = fn(shape, device=device)
    return ro[kind].to(device).reshape(shape).float() if kind in ro else t


def _draw_cam(s, ro, bs, device):
    """-> the RAW draws (bs,1) x 2, or for the other distributions the finished (theta, phi)"""
    if s.sample_dist not in _SIMPLE_CAMS:
        _, ph, th = sample_camera_positions(device, bs, 1, s.h_stddev, s.v_stddev, s.h_mean, s.v_mean, s.sample_dist)
        return th, ph
    fn = torch.rand if s.sample_dist == 'uniform' else torch.randn
    return _draw(ro, 'theta', fn, (bs, 1), device), _draw(ro, 'phi', fn, (bs, 1), device)


def _draw_noise(s, ro, tag, b, m, device):
    """the draws of points_forward for m rays of b images -> noise_c, u (None without resampling), noise_f"""
    S, hier = s.num_steps, s.hierarchical_sample
    noise_c = _draw(ro, 'noise_c' + tag, torch.randn, (b, m, S, 1), device) if hier else None
    u = _draw(ro, 'u' + tag, torch.rand, (b * m, S), device) if hier else None
    return noise_c, u, _draw(ro, 'noise_f' + tag, torch.randn, (b, m, s.E, 1), device)


def draw_randoms(s, b, device):
    """The random tensors of one forward, drawn with the reference's calls, shapes and order so
    that a same-device, same-seed run consumes the generator identically -> jitter, theta / phi (_draw_cam; None with an
    explicit camera), noise_c, u, noise_f (None in the part mode: draw_part_randoms).
    With `forward_points` the reference evaluates image by image in chunks; the fused kernels need no chunking, so only
    the per-image / per-chunk draw order is reproduced, and an override is taken as given."""
    ro = s.rand_override or {}
    n, S = s.n, s.num_steps
    need_cam = s.camera_pos is None or s.camera_lookup is None
    assert not need_cam or s.sample_dist in _SIMPLE_CAMS + ('hybrid', 'truncated_gaussian', 'spherical_uniform', 'mean'), \
        f"camera distribution {s.sample_dist!r}"          # comm_utils.py:526 (`assert 0`), incl. the default None
    if not s.staged:
        jitter = _draw(ro, 'jitter', torch.rand, (b, n, S, 1), device)
        theta, phi = _draw_cam(s, ro, b, device) if need_cam else (None, None)
        noise_c, u, noise_f = (None, None, None) if s.part else _draw_noise(s, ro, '', b, n, device)
        return SimpleNamespace(jitter=jitter, theta=theta, phi=phi, noise_c=noise_c, u=u, noise_f=noise_f)
    js, cams, chunks = [], [], []
    for _ in range(b):
        js.append(torch.rand((1, n, S, 1), device=device))
        if need_cam:
            cams.append(_draw_cam(s, {}, 1, device))
        for head in range(0, n, s.forward_points):
            chunks.append(_draw_noise(s, {}, '', 1, min(s.forward_points, n - head), device))
    ncs, us, nfs = zip(*chunks)
    d = SimpleNamespace(jitter=ro.get('jitter', torch.cat(js, 0)), theta=None, phi=None, noise_c=None, u=None,
                        noise_f=ro.get('noise_f', torch.cat(nfs, 1).view(b, n, s.E, 1)))
    if need_cam:
        d.theta = ro.get('theta', torch.cat([th for th, _ in cams], 0))
        d.phi = ro.get('phi', torch.cat([ph for _, ph in cams], 0))
    if s.hierarchical_sample:
        d.noise_c = ro.get('noise_c', torch.cat(ncs, 1).view(b, n, S, 1))
        d.u = ro.get('u', torch.cat(us, 0))
    return d


def draw_part_randoms(s, b, device):
    """part_grad_forward's own draws, in its order: the permutation of the pixels, then the noise of the `grad_points`
    pixels rendered with gradients and of the rest -> (idx_grad, (noise_c, u, noise_f)), (idx_rest, (...))"""
    ro = s.rand_override or {}
    rand_idx = ro['rand_idx'].to(device) if 'rand_idx' in ro else torch.randperm(s.n, device=device)
    idx_grad, idx_rest = rand_idx[:s.grad_points], rand_idx[s.grad_points:]
    return ((idx_grad, _draw_noise(s, ro, '_grad', b, idx_grad.numel(), device)),
            (idx_rest, _draw_noise(s, ro, '_rest', b, idx_rest.numel(), device)))


def _wants_grad(*values):
    return any(torch.is_tensor(v) and v.requires_grad for v in values)


def camera_setup(s, theta, phi, b, device):
    """the camera draws of draw_randoms, or the explicit camera (theta is None; pitch / yaw are zeros) -> the origin of
    every ray (b,3), cam2world (b,4,4), pitch_yaw (b,2).  O(b) host math, under no_grad (the GAN step: the reference builds its
    rays there) unless the caller's grad mode is on and camera_pos, camera_lookup, h_mean or v_mean is a tensor that requires
    grad: then cam2world carries the graph to them (fitting a camera to an image)."""
    with torch.set_grad_enabled(torch.is_grad_enabled() and _wants_grad(s.camera_pos, s.camera_lookup, s.h_mean, s.v_mean)):
        return _camera_setup(s, theta, phi, b, device)


def _camera_setup(s, theta, phi, b, device):
    if theta is None:
        origin, forward_vector = s.camera_pos, _normalize(s.camera_lookup)
        pitch = yaw = torch.zeros(b, 1, device=device)
    else:
        if s.sample_dist in _SIMPLE_CAMS:
            # (the one-launch form takes the means as floats: a mean that requires grad goes op by op, which is differentiable,
            # and so does a per-image (b, 1) mean, e.g. the fitted angles of projection.project)
            per_image = any(torch.is_tensor(v) and v.numel() > 1 for v in (s.h_mean, s.v_mean))
            if theta.is_cuda and not (s.staged and s.up_vector is not None) and not _wants_grad(s.h_mean, s.v_mean) and not per_image:
                # draws -> pitch, yaw, origin, cam2world in one launch (the ~45 one-wave torch kernels of the op-by-op form
                # below are 0.2 ms of a captured step)
                pitch_yaw, origin, cam2world = ops.camera_pose(theta, phi, s.sample_dist == 'uniform', s.h_stddev, s.h_mean,
                                                               s.v_stddev, s.v_mean)
                return origin, cam2world, pitch_yaw
            if s.sample_dist == 'uniform':
                theta, phi = (theta - 0.5) * 2, (phi - 0.5) * 2
            theta, phi = theta * s.h_stddev + s.h_mean, phi * s.v_stddev + s.v_mean
        origin, pitch = camera_origin_from_angles(theta, phi)
        yaw = theta
        forward_vector = _normalize(-origin)
    # reference quirk kept: only the staged branch of whole_grad_forward hands `up_vector` on
    # (generator.py:1437 vs :1481-1497); the one-shot branch always uses (0, 1, 0)
    cam2world = create_cam2world_matrix(forward_vector, origin, up_vector=s.up_vector if s.staged else None)
    return cam2world[:, :3, 3].contiguous(), cam2world, torch.cat([pitch, yaw], -1)       # every ray starts at the camera


def _zc(fov):
    """the camera-space z of the image plane for a field of view in degrees (get_initial_rays_trig, comm_utils.py:365-438)"""
    return float((-torch.ones(1) / np.tan((2 * math.pi * fov / 360) / 2)).item())


def _unit_normals(grad, mask=None):
    """-grad / |grad| over the last dimension; exact zeros where the gradient is zero or `mask` (grad's leading shape) is 0"""
    norm = grad.norm(dim=-1, keepdim=True)
    keep = norm > 0 if mask is None else (norm > 0) & (mask != 0).unsqueeze(-1)
    return torch.where(keep, -grad / norm, torch.zeros_like(grad))


def _maps(t, b, H):
    """per-ray values (b, H * H) or (b, H * H, k) -> maps (b, 1 or k, H, H)"""
    return t.reshape(b, H, H, -1).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------------------
# generator
# ------------------------------------------------------------------------------------------
class GeneratorNerfINR(nn.Module):
    """Drop-in for exp.cips3d.models.generator.GeneratorNerfINR."""

    def __init__(self, z_dim, nerf_cfg, mapping_nerf_cfg, inr_cfg, mapping_inr_cfg, device='cuda', **kwargs):
        super().__init__()
        self.epoch = 0
        self.step = 0
        self.z_dim = z_dim
        self.device = device
        self.module_name_list = []
        self.siren = NeRFNetwork(**nerf_cfg)
        self.module_name_list.append('siren')
        self.mapping_network_nerf = MultiHeadMappingNetwork(
            **{**mapping_nerf_cfg, 'head_dim_dict': self.siren.style_dim_dict})
        self.module_name_list.append('mapping_network_nerf')
        self.inr_net = CIPSNet(**{**inr_cfg, "input_dim": self.siren.rgb_dim})
        self.module_name_list.append('inr_net')
        self.mapping_network_inr = MultiHeadMappingNetwork(
            **{**mapping_inr_cfg, 'head_dim_dict': self.inr_net.style_dim_dict})
        self.module_name_list.append('mapping_network_inr')
        self.aux_to_rbg = nn.Sequential(nn.Linear(self.siren.rgb_dim, 3), nn.Tanh())
        self.aux_to_rbg.apply(frequency_init(25))
        self.module_name_list.append('aux_to_rbg')
        self.filters = nn.Identity()

    # ---- latent / style plumbing (generator.py:1764-1826) ----
    def z_sampler(self, shape, device, dist='gaussian'):
        if dist == 'gaussian':
            return torch.randn(shape, device=device)
        return torch.rand(shape, device=device) * 2 - 1

    def get_zs(self, b, batch_split=1):
        z_nerf = self.z_sampler(shape=(b, self.mapping_network_nerf.z_dim), device=self.device)
        z_inr = self.z_sampler(shape=(b, self.mapping_network_inr.z_dim), device=self.device)
        if batch_split > 1:
            return [{'z_nerf': a, 'z_inr': c} for a, c in
                    zip(z_nerf.split(b // batch_split), z_inr.split(b // batch_split))]
        return {'z_nerf': z_nerf, 'z_inr': z_inr}

    def mapping_network(self, z_nerf, z_inr, defer_join=False):
        style_dict = {}
        if z_inr.is_cuda and z_inr.shape[0] <= 256:
            # the two z -> style MLPs are independent chains of latency-bound launches: the INR one runs on a side stream —
            # its forward next to the NeRF mapping (and, with defer_join, next to the ray march: forward() joins right
            # before the INR head, the first consumer of its styles), its backward (autograd keeps a node on its forward's
            # stream) next to the NeRF path's backward.  Fork / join by stream waits, so a captured step records it as
            # parallel branches.
            main = torch.cuda.current_stream(z_inr.device)
            side = _side_stream(z_inr.device)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                inr = self._map_inr(z_inr)
            z_inr.record_stream(side)
            style_dict.update(self._map_nerf(z_nerf))
            for t in inr.values():
                t.record_stream(main)
            style_dict.update(inr)
            self._pending_side = side
            if not defer_join:
                self._join_side()
            return style_dict
        style_dict.update(self._map_nerf(z_nerf))
        style_dict.update(self._map_inr(z_inr))
        return style_dict

    def _map_nerf(self, z_nerf):
        """z_nerf -> the NeRF-side styles (the freeze variant runs it under no_grad)"""
        return self.mapping_network_nerf(z_nerf)

    def _map_inr(self, z_inr):
        """z_inr -> the INR-side styles: the chain mapping_network() runs on the side stream"""
        return self.mapping_network_inr(z_inr)

    def _join_side(self):
        """the caller's stream waits for the INR mapping MLP (no-op when nothing is pending)"""
        side = getattr(self, "_pending_side", None)
        if side is not None:
            torch.cuda.current_stream(side.device).wait_stream(side)
            self._pending_side = None

    def generate_avg_frequencies(self, num_samples=10000, device='cuda'):
        zs = self.get_zs(num_samples)
        with torch.no_grad():
            style_dict = self.mapping_network(**zs)
        self.avg_styles = {name: style.mean(0, keepdim=True) for name, style in style_dict.items()}
        return self.avg_styles

    def get_truncated_freq_phase(self, raw_style_dict, avg_style_dict, raw_lambda):
        """generator_nerf_inr.py:770-782"""
        return {name: avg_style_dict[name].lerp(raw, raw_lambda) for name, raw in raw_style_dict.items()}

    def set_device(self, device):
        pass

    def staged_forward(self, *args, **kwargs):
        raise NotImplementedError        # as in the reference (generator.py:1819-1820: the same two lines)

    # ---- the hot path ----
    nerf_grad = True          # False (the freeze variant): the NeRF path runs under no_grad and hands the head detached features

    def _nerf_styles(self, style_dict):
        return style_dict

    def _ray_geometry(self, s, b, device, origin, cam2world, jitter):
        """The constants of the ray set-up (get_world_points_and_direction, generator.py:1378-1657) and the form the NeRF
        path takes for them, named here once:
          "march"   non-hierarchical sampling of whole images: rays + SIREN + composite fused in one kernel that walks the
                    samples along each ray (ops.RayMarchFunction); no (b,n,S,3) points, no per-sample features in HBM
          "rays"    hierarchical sampling of whole images: both SIREN passes and the resampler regenerate rays / points
                    in-kernel (no rays kernel, no (b,n,S,3) point tensors for either pass)
          "points"  everything else (pixel subsets, other SIREN shapes): the points are materialised here, once"""
        S = s.num_steps
        xg, yg, zg = ops.pixel_grids(s.img_size, s.img_size, S, s.ray_start, s.ray_end, device)
        zc = _zc(s.fov)
        in_kernel = (not s.part) and ops.march_available() and self.siren.fused
        g = SimpleNamespace(form=("rays" if s.hierarchical_sample else "march") if in_kernel else "points", b=b, xg=xg, yg=yg,
                            zg=zg, zc=zc, origin=origin, cam2world=cam2world, jitter=jitter.reshape(b, s.n, S))
        # a camera that is being fitted: cam2world carries a graph and the NeRF path runs with gradients.  The in-kernel forms
        # take the matrix as an input of their Functions; the "points" form applies it in torch
        g.cam_grad = self.nerf_grad and torch.is_grad_enabled() and cam2world.requires_grad
        if g.form == "points" and g.cam_grad:
            with torch.no_grad():
                # the camera-space samples and directions: the rays of the identity camera
                eye = torch.eye(4, device=device).expand(b, 4, 4).contiguous()
                q, g.z_vals, d_cam = ops.rays_fwd(xg, yg, zg, zc, eye, g.jitter, b, s.img_size, s.img_size, S)
            Rt = cam2world[:, :3, :3].transpose(1, 2)
            g.points = (q.view(b, s.n * S, 3) @ Rt + cam2world[:, None, :3, 3]).view(b, s.n, S, 3)
            g.dirs = d_cam @ Rt
        elif g.form == "points":
            with torch.no_grad():
                g.points, g.z_vals, g.dirs = ops.rays_fwd(xg, yg, zg, zc, cam2world, g.jitter, b, s.img_size, s.img_size, S)
        return g

    def _nerf_stage(self, s, g, nerf_styles, noise_c, u, noise_f, nerf_grad, idx=None, geo=False):
        """points_forward (generator.py:1659-1746) up to the composite, for all n rays of every image or for the subset
        `idx` of them (form "points" only): -> pixels_fea (b, m, 32), the per-ray depth (b, m) the march / composite kernels
        compute next to the features, opacity.  opacity is None unless `geo`: then it is (b, m), the sum of the ray's weights
        before the last_back top-up, and depth and opacity carry gradients like the features (the Functions' Geo counterparts)"""
        b, S, E, H, W = g.b, s.num_steps, s.E, s.img_size, s.img_size
        m = s.n if idx is None else idx.numel()
        clamp = ops._CLAMP[s.clamp_mode]

        def along_rays(dirs, z):        # origin + direction * depth (generator_nerf_inr.py:537-598) -> points (b, m * S, 3)
            return (g.origin.view(b, 1, 1, 3) + dirs.reshape(b, m, 1, 3) * z.view(b, m, S, 1)).reshape(b, m * S, 3)

        with _grad_ctx(nerf_grad):
            if g.form == "march":
                # (live_fwd: the lists of the backward's live samples may be made in the forward — _head and _render_styles
                # join their stream, ops.live_forward_join)
                geom = ops.MarchGeom(b, H, W, S, g.zc, float(s.nerf_noise), clamp, s.flags, torch.is_grad_enabled(), live_fwd=True)
                out = self.siren.march(nerf_styles, geom, g.xg, g.yg, g.zg, g.cam2world, g.jitter,
                                       noise_f.reshape(b, m, S) if s.nerf_noise != 0 else None, geo=geo)
                return out[0], out[1], out[2] if geo else None
            if g.form == "rays":
                rays = (nerf_styles, ops.RayGeom(b, H, W, S, g.zc), g.xg, g.yg, g.zg, g.cam2world)
                feat_c, sig_c, z_c = self.siren.evaluate_rays(*rays, jitter=g.jitter)
                dirs = None
            else:
                points, z_c, dirs = g.points, g.z_vals, g.dirs
                if idx is not None:
                    points, z_c, dirs = (t.index_select(1, idx).contiguous() for t in (points, z_c, dirs))
                feat_c, sig_c = self.siren.evaluate(points.reshape(b, m * S, 3), nerf_styles)
            feat_c, sig_c, z_c = feat_c.view(b * m, S, 32), sig_c.view(b * m, S), z_c.reshape(b * m, S)
            feat_f = sig_f = fine_z = None
            if s.hierarchical_sample:
                with torch.no_grad():
                    rp = ops._ray_params(g.xg, g.yg, g.zg, g.zc, g.cam2world, None, H, W, S) if g.form == "rays" else None
                    drawn_z, fine_pts = ops.resample_fwd(
                        sig_c, z_c, noise_c.reshape(b * m, S) if s.nerf_noise != 0 else None, s.nerf_noise, u, g.origin,
                        dirs.reshape(b * m, 3) if dirs is not None else None, b, m, S, clamp, rays=rp)
                    fine_z = ops.fine_z_debug(drawn_z)
                    if fine_z is not drawn_z and g.form == "points":
                        fine_pts = along_rays(dirs, fine_z)        # pinned depths, materialised points
                if g.form == "rays":
                    feat_f, sig_f, _ = self.siren.evaluate_rays(*rays, zvals=fine_z.view(b, m * S))
                else:
                    if g.cam_grad and torch.is_grad_enabled():
                        # again outside no_grad: the depths are constants (as in the reference), the origin and the
                        # directions carry the camera's graph
                        fine_pts = along_rays(dirs, fine_z)
                    feat_f, sig_f = self.siren.evaluate(fine_pts.view(b, m * S, 3), nerf_styles)
                feat_f, sig_f = feat_f.view(b * m, S, 32), sig_f.view(b * m, S)
            out = (ops.CompositeGeoFunction if geo else ops.CompositeFunction).apply(
                feat_c, sig_c, z_c, feat_f, sig_f, fine_z, noise_f.reshape(b * m, E) if s.nerf_noise != 0 else None,
                s.nerf_noise, clamp, s.flags)
            return out[0].view(b, m, 32), out[1].view(b, m), out[2].view(b, m) if geo else None

    def _head(self, s, pixels_fea, style_dict, nerf_grad):
        """the tail of points_forward (generator.py:1747-1762) on features of any form: -> inr rgb (b,m,3), aux rgb or None.
        The INR head is called WITHOUT img_size, as the reference does (see CIPSNet)."""
        aux = None
        if s.return_aux_img:
            with _grad_ctx(nerf_grad):
                aux = torch.tanh(_ToRGBFunction.apply(pixels_fea, self.aux_to_rbg[0].weight, self.aux_to_rbg[0].bias))
        if not nerf_grad:
            pixels_fea = pixels_fea.detach()
        self._join_side()
        rgb = self.inr_net(pixels_fea, style_dict)
        # the ray march's forward-time lists (ops.live_plan_forward) ran beside the head on a stream of their own: joined
        # here, behind the head — in front of it the caller's stream would wait for them with nothing else to do
        ops.live_forward_join(pixels_fea.device)
        return rgb, aux

    def _part_grad(self, s, g, nerf_styles, style_dict, device):
        """part_grad_forward (generator.py:1536-1657): a `randperm(n)` splits the pixels of every image into `grad_points`
        rendered with gradients and a rest rendered under no_grad, each with its own noise draws; the two are scattered
        back (int64 bookkeeping of comm_utils.py:240-282) -> inr rgb (b,n,3), aux rgb or None"""
        (idx_grad, noise_grad), (idx_rest, noise_rest) = draw_part_randoms(s, g.b, device)
        fea, _, _ = self._nerf_stage(s, g, nerf_styles, *noise_grad, self.nerf_grad, idx_grad)
        inr_g, aux_g = self._head(s, fea, style_dict, self.nerf_grad)
        with torch.no_grad():
            fea, _, _ = self._nerf_stage(s, g, nerf_styles, *noise_rest, False, idx_rest)
            inr_r, aux_r = self._head(s, fea, style_dict, False)

        def scatter(pg, pr):       # comm_utils.scatter_points: rows idx_grad <- pg (with grad), idx_rest <- pr
            out = torch.zeros(g.b, s.n, pg.shape[-1], device=device, dtype=pg.dtype)
            return out.index_copy(1, idx_grad, pg).index_copy(1, idx_rest, pr)

        return scatter(inr_g, inr_r), scatter(aux_g, aux_r) if s.return_aux_img else None

    def _images(self, inr_rows, aux_rows, b, H):
        """_head's pixel rows (b, H*H, 3) -> images (b,3,H,H): the INR one through self.filters, the auxiliary one (or None) as
        it is; views, made contiguous by the caller.  _render's tail, shared with evaluation.render_feature_volume."""
        inr_img = self.filters(inr_rows.view(b, H, H, 3).permute(0, 3, 1, 2))
        return inr_img, aux_rows.view(b, H, H, 3).permute(0, 3, 1, 2) if aux_rows is not None else None

    def _render(self, style_dict, s, geo=False):
        """whole_grad_forward / part_grad_forward + points_forward (generator.py:1378-1657, 1659-1762) on the HIP path:
        draws (draw_randoms) -> camera (camera_setup) -> NeRF features (_ray_geometry, _nerf_stage) -> head (_head), or
        the last two per pixel subset (_part_grad).  -> imgs, pitch_yaw; with `geo` (render(): whole images in one shot)
        -> SimpleNamespace(imgs, depth, opacity, pitch_yaw, cam2world), the same launches plus the opacity store of the NeRF
        path; cam2world is camera_setup's matrix of this call."""
        device = next(self.parameters()).device
        b = list(style_dict.values())[0].shape[0]
        if not s.part and not s.staged and self.nerf_grad and torch.is_grad_enabled():
            # the INR head's gradient ports, opened before the NeRF path so that its backward is issued first
            # (CIPSNet.open_tail_ports); they sit on the INR mapping network's side stream, joined right before the head.
            # Only where a NeRF backward follows the head's: with a frozen NeRF there is nothing to run beside, and the
            # side-stream form measured 0.4 ms slower than the plain one at the r256 stages (profiles/r6_tail_ab.txt)
            if self.inr_net.open_tail_ports(style_dict, b, s.n, self.siren.rgb_dim, join=False):
                self._pending_side = _side_stream(device)
        d = draw_randoms(s, b, device)
        origin, cam2world, pitch_yaw = camera_setup(s, d.theta, d.phi, b, device)
        g = self._ray_geometry(s, b, device, origin, cam2world, d.jitter)
        nerf_styles = self._nerf_styles(style_dict)
        if s.part:
            inr_img, aux_img = self._part_grad(s, g, nerf_styles, style_dict, device)
        else:
            fea, depth, opacity = self._nerf_stage(s, g, nerf_styles, d.noise_c, d.u, d.noise_f, self.nerf_grad, geo=geo)
            inr_img, aux_img = self._head(s, fea, style_dict, self.nerf_grad)
        inr_img, aux_img = self._images(inr_img, aux_img, b, s.img_size)
        if s.return_aux_img:
            imgs, pitch_yaw = torch.cat([inr_img, aux_img]), torch.cat([pitch_yaw, pitch_yaw])
        else:
            imgs = inr_img.contiguous()
        if not geo:
            return imgs, pitch_yaw
        depth, opacity = (t.view(b, 1, s.img_size, s.img_size) for t in (depth, opacity))
        return SimpleNamespace(imgs=imgs, depth=depth, opacity=opacity, pitch_yaw=pitch_yaw, cam2world=cam2world)

    def forward(self, zs, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, hierarchical_sample,
                h_mean=math.pi * 0.5, v_mean=math.pi * 0.5, psi=1, sample_dist=None, lock_view_dependence=False,
                clamp_mode='relu', nerf_noise=0., white_back=False, last_back=False, return_aux_img=False,
                grad_points=None, forward_points=None, **kwargs):
        """generator.py:1256-1370.  Returns (imgs (b or 2b,3,H,W), pitch_yaw (b or 2b,2))."""
        return self._forward_styles(zs, psi, RenderSettings.of(locals(), rand_override=kwargs.get('rand_override')))

    def render(self, zs, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, hierarchical_sample,
               h_mean=math.pi * 0.5, v_mean=math.pi * 0.5, psi=1, sample_dist=None, clamp_mode='relu', nerf_noise=0.,
               white_back=False, last_back=False, return_aux_img=False, camera_pos=None, camera_lookup=None, up_vector=None,
               rand_override=None, grad_points=None, forward_points=None):
        """forward() (or, with camera_pos / camera_lookup, forward_camera_pos_and_lookup()) that also returns the geometry the
        image is rendered from, differentiable -> SimpleNamespace of
          imgs, pitch_yaw    what that call returns for the same arguments, seed and grad mode: the same bits and the same
                             random draws (batch 2b with return_aux_img), from the same launches except that the NeRF
                             forward runs its opacity-storing instantiation and one more (b, n) tensor is allocated
          depth   (b,1,H,W)  the expected ray depth sum_k w_k z_k of the compositing kernel (under last_back with the topped-up
                             last weight); for nerf_noise = 0 it is geometry().depth bit for bit
          opacity (b,1,H,W)  sum_k w_k, taken BEFORE the last_back top-up (the reference's weights_sum, the soft foreground
                             matte): under last_back it is not the constant 1
          cam2world (b,4,4)  the camera matrix camera_setup returned for this call (b rows with return_aux_img too): what
                             relates this view to another one (evaluation.relative_pose, warp_view)
        depth and opacity carry a grad_fn whenever the NeRF path runs with gradients, as in the reference, where fancy_integration
        returns them as autograd tensors: a depth-supervised inversion, a silhouette loss or a geometric regulariser reaches
        the SIREN weights, the NeRF mapping network, zs['z_nerf'] and a camera that requires grad (camera_pos, camera_lookup,
        tensor h_mean / v_mean) on the native path (ops.RayMarchGeoFunction / ops.CompositeGeoFunction).
        What gets no gradient: the sample depths z (constants, as in the reference: the coarse depths are inputs, the fine ones
        are drawn under no_grad); and on GeneratorNerfINR_freeze_NeRF the whole NeRF path runs under no_grad, so depth and
        opacity have no grad_fn there (imgs keeps the head's).  Whole images in one shot only, as in geometry(): the partial
        (grad_points) and staged (forward_points) forms are refused.  Any value but None is: unlike forward(), which takes
        grad_points >= n pixels as a whole-image render, render() refuses that too."""
        self._whole_images_only('render', 'forward', grad_points, forward_points)
        self._gpu_only('render')
        return self._forward_styles(zs, psi, RenderSettings.of(locals()), geo=True)

    def _whole_images_only(self, name, other, grad_points, forward_points):
        """the refusal of render() / render_styles(): any value but None, unlike `other`, the entry point that takes them"""
        if grad_points is not None or forward_points is not None:
            raise ValueError(f"GeneratorNerfINR.{name} renders whole images in one shot: grad_points / forward_points are not "
                             f"supported (use {other}() for the partial and staged forms; they return no depth or opacity)")

    def _gpu_only(self, name):
        """the refusal of the entry points that have no CPU path -> the parameters' device"""
        device = next(self.parameters()).device
        if device.type != 'cuda':
            raise RuntimeError(f"GeneratorNerfINR.{name} runs on the GPU only (there is no CPU path)")
        return device

    def _truncate(self, style_dict, psi, avg_styles=None):
        """styles -> the same, for psi < 1 lerped towards the average styles: avg_styles(), by default the average of 10 000
        draws through both mapping networks (generate_avg_frequencies), made only then"""
        if psi < 1:
            avg = avg_styles() if avg_styles is not None else self.generate_avg_frequencies(device=self.device)
            style_dict = self.get_truncated_freq_phase(raw_style_dict=style_dict, avg_style_dict=avg, raw_lambda=psi)
        return style_dict

    def _forward_styles(self, zs, psi, s, geo=False):
        """the entry points' common path: latents -> styles (truncated towards the average for psi < 1) -> _render"""
        # (defer_join: joined right before the INR head, _head)
        return self._render_styles(self._truncate(self.mapping_network(**zs, defer_join=not psi < 1), psi), s, geo)

    # ---- style-space entry points: what fitting, interpolation and per-layer mixing work on ----
    def _style_dims(self):
        """name -> width of every style forward() renders from, in the order of its style dictionary (mapping_network: the
        NeRF mapping network's heads, then the INR one's).  The width is the consumer's: the FiLM layers' resp. the modulated
        FCs' style_dim."""
        dims = {f'{self.siren.name_prefix}_w{i}': lay.style_dim for i, lay in enumerate(self.siren.network)}
        dims[f'{self.siren.name_prefix}_rgb'] = self.siren.color_layer_sine.style_dim
        dims.update(self.inr_net.style_dim_dict)
        names = tuple(self.mapping_network_nerf.head_dim_dict) + tuple(self.mapping_network_inr.head_dim_dict)
        return OrderedDict((name, dims[name]) for name in names)

    @property
    def style_names(self):
        """the keys of the style dictionary forward() renders from, in its order"""
        return tuple(self._style_dims())

    def styles(self, zs, psi=1.0):
        """zs -> {name: (b, dim)}: the dictionary forward(zs, psi=psi) renders from — both mapping networks, and for psi < 1
        the truncation towards the average of the same 10 000 draws.  Returned joined: the INR mapping network's side stream
        is not pending.  Under grad mode it is differentiable with respect to zs and the mapping networks."""
        return self._truncate(self.mapping_network(**zs), psi)

    def _check_styles(self, styles, what):
        """the style dictionary of a caller -> a dict in forward()'s order (the same tensors), or ValueError"""
        dims = self._style_dims()
        missing = [name for name in dims if name not in styles]
        unknown = [name for name in styles if name not in dims]
        if missing or unknown:
            raise ValueError(f"{what}: styles must hold exactly G.style_names; missing {missing}, unknown {unknown}")
        b = styles[next(iter(dims))].shape[0] if styles[next(iter(dims))].dim() == 2 else None
        for name, dim in dims.items():
            t = styles[name]
            if t.dim() != 2 or t.shape[0] != b or t.shape[1] != dim:
                raise ValueError(f"{what}: style {name!r} must be ({b if b is not None else 'b'}, {dim}), got {tuple(t.shape)}")
        self._gpu_only(what)
        return {name: styles[name] for name in dims}

    def _render_styles(self, style_dict, s, geo=False):
        """the entry points' common path behind the mapping networks: styles (the latent entry points', possibly with the INR
        mapping network's side stream still pending, or a caller's) -> _render, with the clean-up every exit needs"""
        try:
            # with forward_points the reference evaluates image by image in chunks under no_grad (generator.py:1325-1347)
            with torch.set_grad_enabled(torch.is_grad_enabled() and not s.staged):
                return self._render(style_dict, s, geo)
        finally:
            # a deferred INR-mapping side stream is joined on EVERY exit (no-op after _head's own join): an exception
            # before the INR head must not leave the fork open — the main stream would never wait for it, and a
            # hipGraph capture would end with an unjoined stream.  Nor may it leave the gradient ports _render opened
            # for the head pending: they hold the modulation graph, and the next forward() must not find them
            self._join_side()
            ops.live_forward_join()         # likewise the ray march's list stream (no-op after _head's join)
            self.inr_net._tail = None

    def forward_styles(self, styles, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, hierarchical_sample,
                       h_mean=math.pi * 0.5, v_mean=math.pi * 0.5, sample_dist=None, lock_view_dependence=False,
                       clamp_mode='relu', nerf_noise=0., white_back=False, last_back=False, return_aux_img=False,
                       grad_points=None, forward_points=None, camera_pos=None, camera_lookup=None, up_vector=None, **kwargs):
        """forward() (or, with camera_pos / camera_lookup, forward_camera_pos_and_lookup()) from a style dictionary instead of
        latents: `styles` holds one (b, dim) tensor per name of G.style_names — styles(zs, psi), or anything made from such
        dictionaries (a fitted offset, an interpolation, a per-layer mix).  The other arguments are forward()'s without zs
        and psi; forward_styles(styles(zs, psi), ...) returns what forward(zs, psi=psi, ...) returns for the same seed, bit
        for bit, and the same parameter gradients.  Every key may be its own tensor, and a leaf: the gradient of an image loss
        reaches it (on the freeze variant only the INR-side keys, the NeRF path runs under no_grad there)."""
        return self._render_styles(self._check_styles(styles, "forward_styles"),
                                   RenderSettings.of(locals(), rand_override=kwargs.get('rand_override')))

    def render_styles(self, styles, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, hierarchical_sample,
                      h_mean=math.pi * 0.5, v_mean=math.pi * 0.5, sample_dist=None, clamp_mode='relu', nerf_noise=0.,
                      white_back=False, last_back=False, return_aux_img=False, camera_pos=None, camera_lookup=None,
                      up_vector=None, rand_override=None, grad_points=None, forward_points=None):
        """render() from a style dictionary (forward_styles' `styles`): -> SimpleNamespace(imgs, depth, opacity, pitch_yaw, cam2world),
        what render(zs, psi=psi, ...) returns for styles(zs, psi).  Whole images in one shot only, as render()."""
        self._whole_images_only('render_styles', 'forward_styles', grad_points, forward_points)
        return self._render_styles(self._check_styles(styles, "render_styles"), RenderSettings.of(locals()), geo=True)

    def _density_styles(self, z_nerf, psi):
        """z_nerf -> the NeRF styles of the density entry points: only the NeRF mapping network runs; for psi < 1 the styles are
        truncated towards the average of 10 000 draws as in forward() (the same draws from the RNG as
        generate_avg_frequencies: get_zs draws both latents), an average of its own that leaves self.avg_styles alone"""
        def avg_styles():
            return {name: style.mean(0, keepdim=True) for name, style in self._map_nerf(self.get_zs(10000)['z_nerf']).items()}

        return self._truncate(self._map_nerf(z_nerf), psi, avg_styles)

    @torch.no_grad()
    def density_gradient(self, zs, points, psi=1.0):
        """sigma (b,P) and d sigma / d point (b,P,3) of zs['z_nerf'] at arbitrary world-space points (b,P,3), no grad_fn:
        density_grid's style handling and truncation, NeRFNetwork.density_gradient's kernel."""
        return self.siren.density_gradient(points, self._nerf_styles(self._density_styles(zs['z_nerf'], psi)))

    # ---- the colour of the shape ----
    # False: the styles of an 'aux' colour come from the NeRF mapping network alone (_density_styles).  generator_v1 sets it: its
    # colour style nerf_rgb is a head of the INR mapping network, so both networks run for any colour
    _color_style_from_inr = False
    _COLOR_MODES = ('aux', 'head')

    def _check_color_mode(self, who, mode, img_size, none_ok=False):
        if not ((none_ok and mode is None) or mode in self._COLOR_MODES):
            raise ValueError(f"GeneratorNerfINR.{who}: colours are {'None, ' if none_ok else ''}'aux' or 'head', got {mode!r}")
        if mode == 'head' and img_size is None:
            raise ValueError(f"GeneratorNerfINR.{who}: 'head' colours need img_size (it selects the depth of the INR head)")
        if mode == 'head' and img_size < 32:
            raise ValueError(f"GeneratorNerfINR.{who}: 'head' colours need img_size >= 32 (block \"32\" is the first of the INR "
                             f"head with a ToRGB layer: a shallower head has no colour), got {img_size}")

    def _color_styles(self, zs, psi, mode):
        """zs -> the styles of a colour query.  'aux': the density entry points' (_density_styles: only the NeRF mapping network,
        for psi < 1 an average of its own over 10 000 draws) unless _color_style_from_inr; 'head', or that flag: forward()'s —
        both mapping networks, joined, for psi < 1 truncated towards generate_avg_frequencies' average (which it stores)"""
        if mode == 'head' or self._color_style_from_inr:
            return self._nerf_styles(self._truncate(self.mapping_network(**zs), psi))
        return self._nerf_styles(self._density_styles(zs['z_nerf'], psi))

    def _colors_at(self, points, style_dict, mode, img_size):
        """rgb (b,P,3) in [-1, 1] at world-space points (b,P,3) for styles of _color_styles: 'aux' the point-colour kernel with
        the auxiliary RGB layer's Linear (its Tanh is the kernel's), 'head' the SIREN's features as pixels through the INR head"""
        if mode == 'aux':
            return self.siren.color(points, style_dict, self.aux_to_rbg[0].weight, self.aux_to_rbg[0].bias, tanh=True)
        feat, _ = self.siren.evaluate(points, style_dict)
        return self.inr_net(feat, style_dict, img_size=img_size)

    @torch.no_grad()
    def point_colors(self, zs, points, psi=1.0, mode='aux', img_size=None):
        """The colour of the generator's radiance field at arbitrary world-space points (b,P,3) -> (b,P,3) fp32 in [-1, 1], no
        grad_fn.
          'aux'   tanh(W_a f(x) + b_a) with the SIREN's 32 colour features f and aux_to_rbg's Linear, from the point-colour
                  kernel (NeRFNetwork.color).  The auxiliary image is tanh(W_a sum_k w_k f_k + b_a); the map is affine and under
                  last_back a ray's weights sum to one, so that image is the volume rendering of this per-point field.  Only
                  the NeRF mapping network runs (generator_v1: both, its colour style comes from the INR one); psi < 1
                  truncates as density_grid does, with the same draws.
          'head'  the features of the points as (b,P,32) "pixels" through the CIPS head with the styles of zs['z_inr'], for
                  checkpoints trained without the auxiliary image.  img_size is required: it selects the head's depth (forward()
                  runs all nine blocks, img_size=1024) and must be at least 32, the first block with a ToRGB layer.  Both mapping networks run; psi < 1 truncates both towards
                  generate_avg_frequencies' average, as forward() does, with its draws.  Any P."""
        self._gpu_only('point_colors')
        self._check_color_mode('point_colors', mode, img_size)
        return self._colors_at(points, self._color_styles(zs, psi, mode), mode, img_size)

    @torch.no_grad()
    def color_grid(self, zs, resolution=256, cube_length=0.3, center=(0., 0., 0.), psi=1.0, return_sigma=False):
        """The 'aux' point colour (point_colors) on density_grid's N^3 lattice -> (b, N, N, N, 3) fp32 in [-1, 1]; with
        return_sigma=True -> (rgb, sigma (b, N, N, N)), sigma density_grid's bit for bit from the same launch.  The lattice
        kernel reads the three coordinate arrays: no points tensor and no (b, N^3, 32) feature tensor exist.  Auxiliary colours
        only: the INR head over 16.7 M points per image is out of scope (colour a mesh's vertices with extract_mesh(colors=
        'head') or point_colors instead).  Styles, truncation and RNG draws: density_grid's (generator_v1: forward()'s)."""
        from .evaluation import density_lattice
        self._gpu_only('color_grid')
        style_dict = self._color_styles(zs, psi, 'aux')
        gx, gy, gz = (g.to(zs['z_nerf'].device) for g in density_lattice(resolution, cube_length, center))
        return self.siren.color_lattice(gx, gy, gz, style_dict, self.aux_to_rbg[0].weight, self.aux_to_rbg[0].bias, tanh=True,
                                        sigma=return_sigma)

    @torch.no_grad()
    def bake(self, zs, resolution=128, cube_length=0.3, center=(0., 0., 0.), psi=1.0):
        """The radiance field of zs baked onto density_grid's N^3 lattice, for evaluation.render_volume: one launch of
        color_grid(return_sigma=True) and ops.bake_volume -> SimpleNamespace
          rgbs       (b, N, N, N, 4)  r, g, b, sigma per node: rgbs[..., :3] is color_grid's and rgbs[..., 3] density_grid's
                                      output for the same arguments, bit for bit ('aux' colours)
          occupancy  (b, ceil((N-1)/8),) * 3  the brick maxima of sigma that the renderer's empty-space skip reads
          lo, hi     three floats each: the first and last coordinate of evaluation.density_lattice per axis, the box the
                     renderer spreads the N nodes over uniformly
          resolution N
        The network runs here once; every view of the volume afterwards is a gather-and-composite pass.  A volume costs
        16 N^3 bytes per image (33.5 MB at N = 128, 268 MB at N = 256).  No gradient."""
        from . import ops
        from .evaluation import density_lattice
        rgb, sigma = self.color_grid(zs, resolution=resolution, cube_length=cube_length, center=center, psi=psi, return_sigma=True)
        packed, occ = ops.bake_volume(sigma, rgb)
        grids = density_lattice(resolution, cube_length, center)
        return SimpleNamespace(rgbs=packed, occupancy=occ, lo=tuple(float(g[0]) for g in grids),
                               hi=tuple(float(g[-1]) for g in grids), resolution=int(resolution))

    @torch.no_grad()
    def bake_features(self, zs, resolution=64, cube_length=0.3, center=(0., 0., 0.), psi=1.0, slab=None):
        """The SIREN's 32 colour features and sigma of zs baked onto density_grid's N^3 lattice, for
        evaluation.render_feature_volume, which composites them per ray and runs the INR head on the result: forward()'s
        picture (not the auxiliary one bake() holds) with the SIREN out of the loop -> SimpleNamespace
          sigma      (b, N, N, N)        the density per node
          features   (b, 8, N, N, N, 4)  channel-group-major planes: features[:, g, i, j, k] holds channels 4g .. 4g+3 of node
                                         (i, j, k) (ops.bake_feature_volume's layout)
          occupancy  (b, ceil((N-1)/8),) * 3  the brick maxima of sigma, bake()'s
          lo, hi     three floats each, bake()'s box
          resolution N
          styles     the full style dictionary the volume was baked with, NeRF and INR keys (b rows each): the renderer needs
                     no zs
        Styles: forward()'s — both mapping networks, joined; psi < 1 truncates both towards generate_avg_frequencies' average
        with its draws (_color_styles(zs, psi, 'head')).  density_grid's default style path is another one (_density_styles:
        the NeRF mapping network alone, for psi < 1 an average of its own), so for psi < 1 sigma is not density_grid(zs)'s; it
        is NeRFNetwork.density_lattice's on the same lattice with volume.styles, bit for bit, and for psi = 1 density_grid's.
        The lattice is evaluated by NeRFNetwork.evaluate a slab of x-planes at a time and packed slab by slab, so that the
        (b, slab N^2, 32) temporary stays bounded: `slab` x-planes per pass, by default as many as keep it under 256 MB.  The
        result does not depend on it.  A volume costs 132 N^3 bytes per image: 34.6 MB at N = 64, 277 MB at N = 128.
        No gradient; GPU only."""
        from . import ops
        from .evaluation import density_lattice
        device = self._gpu_only('bake_features')
        N = int(resolution)
        style_dict = self._color_styles(zs, psi, 'head')
        b = zs['z_nerf'].shape[0]
        grids = density_lattice(N, cube_length, center)
        gx, gy, gz = (g.to(device) for g in grids)
        if slab is None:
            slab = max(1, (256 << 20) // max(1, b * N * N * 128))
        slab = int(slab)
        if slab < 1:
            raise ValueError(f"GeneratorNerfINR.bake_features: slab must be at least 1 x-plane, got {slab}")
        sigma, planes, occ = ops.feature_volume_buffers(b, N, N, N, device)
        for x0 in range(0, N, slab):
            feat, sig = self.siren.evaluate(ops.lattice_points(gx[x0:x0 + slab], gy, gz, b).contiguous(), style_dict)
            sigma[:, x0:x0 + slab] = sig.view(b, -1, N, N)
            ops._bake_feature_slab(sigma, feat.contiguous(), planes, occ, x0)
        return SimpleNamespace(sigma=sigma, features=planes, occupancy=occ, lo=tuple(float(g[0]) for g in grids),
                               hi=tuple(float(g[-1]) for g in grids), resolution=N, styles=dict(style_dict))

    @torch.no_grad()
    def geometry(self, zs, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, hierarchical_sample,
                 h_mean=math.pi * 0.5, v_mean=math.pi * 0.5, psi=1, sample_dist=None, clamp_mode='relu', white_back=False,
                 last_back=False, camera_pos=None, camera_lookup=None, up_vector=None, rand_override=None):
        """The geometry of the image forward() (or, with camera_pos / camera_lookup, forward_camera_pos_and_lookup()) renders
        for the same arguments under no_grad with nerf_noise = 0 -> SimpleNamespace of
          depth   (b,1,H,W)  the expected ray depth the march / composite kernels compute next to the features
          points  (b,3,H,W)  origin + direction * depth, world space (directions: ops.rays_fwd)
          sigma   (b,1,H,W)  the density at those points
          normals (b,3,H,W)  -grad sigma / |grad sigma| there (ops.siren_sigma_grad); exact zeros where the gradient is zero
          pitch_yaw (b,2)
          cam2world (b,4,4)  the camera matrix camera_setup returned for this call
        Only the NeRF mapping network runs: neither the INR mapping network nor the head.
        Random numbers: the draws and the camera are draw_randoms / camera_setup on the RenderSettings of those calls, so a
        seed gives the geometry of the image it renders, and the generator is left in the state forward() leaves it in — with
        whole images in one shot (no grad_points / forward_points), which is all this entry point offers: every draw of a
        forward, the noise tensors included, is made before the NeRF path starts and nothing after it draws.  For psi < 1 the
        10 000 latents of the average styles are drawn as get_zs draws them (both z_nerf and z_inr), as in forward()."""
        device = self._gpu_only('geometry')
        s, b, H = RenderSettings.of(locals(), nerf_noise=0.), zs['z_nerf'].shape[0], img_size
        nerf_styles, d, origin, cam2world, pitch_yaw = self._density_camera(s, zs, psi, device)
        g = self._ray_geometry(s, b, device, origin, cam2world, d.jitter)
        _, depth, _ = self._nerf_stage(s, g, nerf_styles, d.noise_c, d.u, d.noise_f, False)
        dirs = g.dirs if g.form == "points" else ops.rays_fwd(g.xg, g.yg, g.zg, g.zc, cam2world, g.jitter, b, H, H, s.num_steps)[2]
        points = origin.view(b, 1, 3) + dirs * depth.view(b, s.n, 1)
        sigma, grad = self.siren.density_gradient(points, nerf_styles)
        normals = _unit_normals(grad)
        return SimpleNamespace(depth=_maps(depth, b, H), points=_maps(points, b, H), sigma=_maps(sigma, b, H),
                               normals=_maps(normals, b, H), pitch_yaw=pitch_yaw, cam2world=cam2world)

    def _density_camera(self, s, zs, psi, device):
        """what geometry() and surface() start from, in the order forward() consumes the generator in: the NeRF styles of the
        density entry points (for psi < 1 the 10 000 latents are drawn here, before the draws of the forward), then the draws
        and the camera of settings s -> nerf_styles, draws, origin, cam2world, pitch_yaw"""
        nerf_styles = self._nerf_styles(self.siren._sigma_args(self._density_styles(zs['z_nerf'], psi)))
        b = zs['z_nerf'].shape[0]
        d = draw_randoms(s, b, device)
        return (nerf_styles, d) + camera_setup(s, d.theta, d.phi, b, device)

    @torch.no_grad()
    def surface(self, zs, level, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean=math.pi * 0.5,
                v_mean=math.pi * 0.5, psi=1, sample_dist=None, camera_pos=None, camera_lookup=None, up_vector=None, refine=8,
                normals=True, rand_override=None):
        """The surface sigma = level as the camera of forward() (or, with camera_pos / camera_lookup, of
        forward_camera_pos_and_lookup()) sees it: every ray is walked through the density at the `num_steps` unjittered depths
        from ray_start to ray_end, stopped at the first crossing of `level` and refined by `refine` bisection steps and a secant
        step (NeRFNetwork.surface_rays; the rule: include/cips3d_hip.h, cips_siren_surface_x3) -> SimpleNamespace of
          depth   (b,1,H,W)  the depth of the crossing — geometry()'s quantity; ray_start where the ray starts inside the
                             surface, ray_end where it crosses nothing
          mask    (b,1,H,W)  uint8: 1 crossing, 0 none (background), 2 the ray starts inside
          points  (b,3,H,W)  origin + direction * depth, world space
          sigma   (b,1,H,W)  the density at those points: level up to the residual of the refinement where mask == 1
          normals (b,3,H,W)  -grad sigma / |grad sigma| at the points (NeRFNetwork.density_gradient); exact zeros where
                             mask == 0 or the gradient is zero; None with normals=False
          pitch_yaw (b,2)
          cam2world (b,4,4)  the camera matrix camera_setup returned for this call
        `level` has no default (as in extract_mesh, whose mesh this is a view of).  Only the NeRF mapping network runs.  Random
        numbers: as geometry() — the draws and the camera are draw_randoms / camera_setup on the RenderSettings of a
        non-hierarchical forward() with nerf_noise = 0, so a seed gives the camera of the image it renders and the generators
        are left where forward() leaves them; the jitter is drawn and not used.  surface_colored() is this call with the colour
        of the surface points next to it."""
        return self._surface('surface', None, zs, level, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean,
                             v_mean, psi, sample_dist, camera_pos, camera_lookup, up_vector, refine, normals, rand_override)

    @torch.no_grad()
    def surface_colored(self, zs, level, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean=math.pi * 0.5,
                        v_mean=math.pi * 0.5, psi=1, sample_dist=None, camera_pos=None, camera_lookup=None, up_vector=None,
                        refine=8, normals=True, rand_override=None, colors='aux'):
        """surface() with the colour of the surface: its arguments and `colors` ('aux' or 'head'; None is surface() itself) ->
        surface()'s SimpleNamespace and
          rgb     (b,3,H,W)  point_colors' colour of that mode at `points` (for 'head' the INR head at depth img_size, which
                             must be at least 32), exactly -1 where mask == 0; evaluation.shade_surface(albedo=True) shades it
        An entry point of its own because surface()'s signature is part of the public contract (it is listed parameter by
        parameter in tests/test_render_settings_cpu.py).  Random numbers and styles: 'aux' makes surface()'s draws, runs only the
        NeRF mapping network and returns surface()'s other fields bit for bit.  'head' — and 'aux' on generator_v1, whose colour
        style is a head of the INR mapping network — takes forward()'s styles instead: both mapping networks run, and psi < 1
        draws the 10 000 latents as generate_avg_frequencies does (storing its average) and truncates the NeRF and the INR
        styles alike, before the draws of the camera; the other fields are then those of the truncated shape forward() renders
        (for psi = 1: surface()'s)."""
        return self._surface('surface_colored', colors, zs, level, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev,
                             h_mean, v_mean, psi, sample_dist, camera_pos, camera_lookup, up_vector, refine, normals, rand_override)

    def _surface(self, who, colors, zs, level, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean, v_mean, psi,
                 sample_dist, camera_pos, camera_lookup, up_vector, refine, normals, rand_override):
        """surface() (colors None) and surface_colored(): the settings, the styles and the camera in forward()'s order, the ray
        cast, the normals and, when asked for, the colours at the surface points"""
        device = self._gpu_only(who)
        self._check_color_mode(who, colors, img_size, none_ok=True)
        s, b, H = RenderSettings.of(locals(), hierarchical_sample=False, nerf_noise=0.), zs['z_nerf'].shape[0], img_size
        if colors is None:
            nerf_styles, _, _, cam2world, pitch_yaw = self._density_camera(s, zs, psi, device)
        else:
            nerf_styles = self._color_styles(zs, psi, colors)
            d = draw_randoms(s, b, device)
            _, cam2world, pitch_yaw = camera_setup(s, d.theta, d.phi, b, device)
        xg, yg, zg = ops.pixel_grids(H, H, num_steps, ray_start, ray_end, device)
        depth, hit, sigma, points = self.siren.surface_rays(nerf_styles, ops.RayGeom(b, H, H, num_steps, _zc(fov)), xg, yg, zg,
                                                            cam2world, level, refine)
        nrm = _unit_normals(self.siren.density_gradient(points, nerf_styles)[1], hit) if normals else None
        out = SimpleNamespace(depth=_maps(depth, b, H), mask=_maps(hit, b, H), points=_maps(points, b, H),
                              sigma=_maps(sigma, b, H), normals=_maps(nrm, b, H) if normals else None, pitch_yaw=pitch_yaw,
                              cam2world=cam2world)
        if colors is not None:
            rgb = self._colors_at(points, nerf_styles, colors, img_size)
            out.rgb = _maps(torch.where(hit.unsqueeze(-1) != 0, rgb, rgb.new_full((), -1.)), b, H)
        return out

    @torch.no_grad()
    def density_grid(self, zs, resolution=256, cube_length=0.3, center=(0., 0., 0.), psi=1.0, return_gradient=False):
        """The density sigma of zs['z_nerf'] on an N^3 lattice -> (b, N, N, N) fp32, no gradient: the volume that
        exp/pigan/scripts/extract_shapes.py feeds to marching cubes (sample_generator, :38-60), from the sigma-only SIREN
        kernel — only the NeRF mapping network runs, the INR one does not, and no points tensor is built.

        Axis a in {x, y, z} has the coordinates  arange(N) * (L / (N - 1)) + (center[a] - L / 2)  (evaluation.density_lattice,
        fp32 on the host; the kernel reads them and computes none), and element [b, i, j, k] is sigma at (x_i, y_j, z_k).
        This is the integer lattice ON PURPOSE.  The reference's create_samples (:18-31) divides a float index by N without
        flooring, which shears two of the axes by up to one voxel across the faster-running index, and pairs
        voxel_origin[2] with x (and [0] with z); neither is reproduced.  For psi < 1 the NeRF styles are truncated towards
        the average of 10 000 draws as in forward() (the same draws from the RNG as generate_avg_frequencies).
        return_gradient: -> (sigma (b, N, N, N), d sigma / d (x, y, z) (b, N, N, N, 3)) from the gradient lattice kernel
        (NeRFNetwork.density_gradient_lattice); sigma is the default call's bit for bit."""
        from .evaluation import density_lattice
        style_dict = self._density_styles(zs['z_nerf'], psi)
        gx, gy, gz = (g.to(zs['z_nerf'].device) for g in density_lattice(resolution, cube_length, center))
        if return_gradient:
            return self.siren.density_gradient_lattice(gx, gy, gz, self._nerf_styles(style_dict))
        return self.siren.density_lattice(gx, gy, gz, self._nerf_styles(style_dict))

    @torch.no_grad()
    def extract_mesh(self, zs, level, resolution=256, cube_length=0.3, center=(0., 0., 0.), psi=1.0, normals=True, colors=None,
                     img_size=None):
        """The surface sigma = level of density_grid's volume as one indexed triangle mesh per image -> a list of
        SimpleNamespace(vertices (V, 3) fp32, faces (T, 3) int32, normals (V, 3) fp32 or None), all on the GPU; the volume never
        leaves it (ops.mesh_from_volume: marching tetrahedra, one host synchronisation for the mesh sizes).  `level` has no
        default: the right iso-value depends on the checkpoint.  The volume is density_grid's for the same arguments — same
        styles, truncation and RNG draws (psi < 1 draws the 10 000 latents once).  Triangles are wound so that their geometric
        normal points towards lower density; `normals` are -grad sigma / |grad sigma| at the vertices from
        NeRFNetwork.density_gradient with that image's styles, exact zeros where the gradient is zero (as in geometry).
        colors: None, 'aux' or 'head' — each mesh also gets .colors (V, 3) fp32 in [-1, 1], point_colors' colour of that mode at
        its vertices with that image's latents ((0, 3) for an empty mesh; 'head' needs img_size, see point_colors;
        evaluation.save_ply writes them).  With colors=None the result and the RNG draws are unchanged, and there is no .colors.
        'aux' changes neither geometry nor draws (generator_v1 excepted: its colour style needs the INR mapping network, so
        there, as with 'head' everywhere, the styles are forward()'s — both mapping networks, and psi < 1 draws and truncates as
        forward() does, the shape's styles included)."""
        from .evaluation import density_lattice
        device = zs['z_nerf'].device
        self._check_color_mode('extract_mesh', colors, img_size, none_ok=True)
        if colors is None:
            nerf_styles = self._nerf_styles(self._density_styles(zs['z_nerf'], psi))
        else:
            nerf_styles = self._color_styles(zs, psi, colors)
        gx, gy, gz = (g.to(device) for g in density_lattice(resolution, cube_length, center))
        sigma = self.siren.density_lattice(gx, gy, gz, nerf_styles)
        meshes = []
        for b, (vertices, faces) in enumerate(ops.mesh_from_volume(sigma.contiguous(), gx, gy, gz, level)):
            n = None
            styles_b = {name: style[b:b + 1] for name, style in nerf_styles.items()}
            if normals:
                n = torch.zeros_like(vertices)
                if vertices.shape[0]:
                    n = _unit_normals(self.siren.density_gradient(vertices.unsqueeze(0), styles_b)[1][0])
            mesh = SimpleNamespace(vertices=vertices, faces=faces, normals=n)
            if colors is not None:
                mesh.colors = torch.zeros_like(vertices)
                if vertices.shape[0]:
                    mesh.colors = self._colors_at(vertices.unsqueeze(0), styles_b, colors, img_size)[0]
            meshes.append(mesh)
        return meshes

    def forward_camera_pos_and_lookup(self, zs, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev,
                                      h_mean, v_mean, hierarchical_sample, camera_pos, camera_lookup, psi=1,
                                      sample_dist=None, lock_view_dependence=False, clamp_mode='relu',
                                      nerf_noise=0., white_back=False, last_back=False, return_aux_img=False,
                                      grad_points=None, forward_points=None, up_vector=None, **kwargs):
        """generator.py:1828-1951 (explicit camera; pitch/yaw are zeros)."""
        return self._forward_styles(zs, psi, RenderSettings.of(locals(), rand_override=kwargs.get('rand_override')))


class GeneratorNerfINR_freeze_NeRF(GeneratorNerfINR):
    """generator.py:1955-2083: mapping_nerf, both SIREN passes, the composite and aux_to_rbg run
    under no_grad; gradients flow only through the CIPS INR head and mapping_inr."""
    nerf_grad = False

    def load_nerf_ema(self, G_ema):
        self.siren.load_state_dict(G_ema.siren.state_dict())
        self.mapping_network_nerf.load_state_dict(G_ema.mapping_network_nerf.state_dict())
        self.aux_to_rbg.load_state_dict(G_ema.aux_to_rbg.state_dict())

    def _map_nerf(self, z_nerf):
        with torch.no_grad():
            return super()._map_nerf(z_nerf)
