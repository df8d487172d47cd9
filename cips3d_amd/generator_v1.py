"""MI355X-native drop-in for the reference's second generator layout (exp/cips3d/models/generator_v1.py), the one the AFHQ
recipes (exp/cips3d/configs/afhq_exp.yaml) and ffhq_exp_v1.yaml build.

It differs from generator.py in one place: the colour FiLM style of the SIREN, `nerf_rgb`, is no longer a head of the NeRF
mapping network.  It is the first head of the INR mapping network, turned into a 128-wide style by a new Linear,
`nerf_rgb_mapping` (generator_v1.py:1192-1212, 1794-1819).  Everything else — rays, SIREN, hierarchical sampling, compositing,
the CIPS head, part_grad_forward — is the v0 code, so these classes are the v0 drop-ins with the v1 constructor (174 state_dict
keys, the reference's initialisation draw order) and three overrides:

  _map_inr       the INR mapping network followed by nerf_rgb_mapping on the grouped-linear kernel: both run on the INR
                 mapping side stream, their backward next to the NeRF path's;
  _nerf_styles   _render calls it ahead of its NeRF stage (_nerf_stage): the caller's stream joins that side stream before
                 the first SIREN launch, whose colour FiLM reads nerf_rgb (v0 joins in _head, right before the INR head;
                 DESIGN.md §3, "generator_v1");
  forward_camera_pos_and_lookup   takes no up_vector (generator_v1.py:1845): the keyword lands in **kwargs and is ignored,
                 on the staged path too.
"""
import torch
import torch.nn as nn

from . import generator, ops
from .generator import CIPSNet, MultiHeadMappingNetwork, NeRFNetwork, frequency_init


class GeneratorNerfINR(generator.GeneratorNerfINR):
    """Drop-in for exp.cips3d.models.generator_v1.GeneratorNerfINR (generator_v1.py:1159-1967)."""

    def __init__(self, z_dim, nerf_cfg, mapping_nerf_cfg, inr_cfg, mapping_inr_cfg, device='cuda', **kwargs):
        nn.Module.__init__(self)
        self.epoch = 0
        self.step = 0
        self.z_dim = z_dim
        self.device = device
        self.module_name_list = []
        self.siren = NeRFNetwork(**nerf_cfg)
        self.module_name_list.append('siren')
        # (the reference pops the colour style out of the SIREN's own style_dim_dict)
        shape_style_dict = self.siren.style_dim_dict
        color_style_dict = {'nerf_rgb': shape_style_dict.pop('nerf_rgb')}
        self.mapping_network_nerf = MultiHeadMappingNetwork(**{**mapping_nerf_cfg, 'head_dim_dict': shape_style_dict})
        self.module_name_list.append('mapping_network_nerf')
        self.inr_net = CIPSNet(**{**inr_cfg, "input_dim": self.siren.rgb_dim})
        self.module_name_list.append('inr_net')
        color_style_dict.update(self.inr_net.style_dim_dict)
        self.mapping_network_inr = MultiHeadMappingNetwork(**{**mapping_inr_cfg, 'head_dim_dict': color_style_dict})
        self.module_name_list.append('mapping_network_inr')
        self.nerf_rgb_mapping = nn.Linear(in_features=mapping_inr_cfg['hidden_dim'], out_features=color_style_dict['nerf_rgb'])
        self.module_name_list.append('nerf_rgb_mapping')
        self.aux_to_rbg = nn.Sequential(nn.Linear(self.siren.rgb_dim, 3), nn.Tanh())
        self.aux_to_rbg.apply(frequency_init(25))
        self.module_name_list.append('aux_to_rbg')
        self.filters = nn.Identity()

    # the colour entry points (point_colors, color_grid, extract_mesh with colors, surface_colored): nerf_rgb, which every colour of the
    # SIREN depends on, leaves the INR mapping chain here, so an 'aux' colour too runs both mapping networks on forward()'s styles
    _color_style_from_inr = True

    def _map_inr(self, z_inr):
        """generator_v1.py:1808-1818: style_dict['nerf_rgb'] = nerf_rgb_mapping(<INR mapping output>), on the grouped-linear
        kernel (the 10 000 latents of generate_avg_frequencies take the Linear itself, like the mapping network's layers)"""
        inr = self.mapping_network_inr(z_inr)
        inr['nerf_rgb'] = ops.grouped_linear([(inr['nerf_rgb'], self.nerf_rgb_mapping)])[0]
        return inr

    def _nerf_styles(self, style_dict):
        # every SIREN launch runs the colour FiLM layer on nerf_rgb, the end of the INR mapping chain: join its side stream
        # here, before the first one (this also waits for the head's modulation Linears, which open_tail_ports queued there)
        self._join_side()
        return style_dict

    def forward_camera_pos_and_lookup(self, zs, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev,
                                      h_mean, v_mean, hierarchical_sample, camera_pos, camera_lookup, psi=1,
                                      sample_dist=None, lock_view_dependence=False, clamp_mode='relu',
                                      nerf_noise=0., white_back=False, last_back=False, return_aux_img=False,
                                      grad_points=None, forward_points=None, **kwargs):
        """generator_v1.py:1845-1967: no up_vector parameter; one given by keyword is ignored, also where v0 honours it"""
        kwargs.pop('up_vector', None)
        return super().forward_camera_pos_and_lookup(
            zs, img_size, fov, ray_start, ray_end, num_steps, h_stddev, v_stddev, h_mean, v_mean, hierarchical_sample,
            camera_pos, camera_lookup, psi=psi, sample_dist=sample_dist, lock_view_dependence=lock_view_dependence,
            clamp_mode=clamp_mode, nerf_noise=nerf_noise, white_back=white_back, last_back=last_back,
            return_aux_img=return_aux_img, grad_points=grad_points, forward_points=forward_points, **kwargs)


class GeneratorNerfINR_freeze_NeRF(GeneratorNerfINR, generator.GeneratorNerfINR_freeze_NeRF):
    """generator_v1.py:1970-1990: as v0's freeze variant (NeRF mapping, SIREN, composite and aux_to_rbg under no_grad), and
    the whole INR-side mapping — mapping_network_inr and nerf_rgb_mapping — runs under no_grad too: unlike v0, neither gets a
    gradient; only the CIPS head trains."""

    def load_nerf_ema(self, G_ema):
        super().load_nerf_ema(G_ema)
        self.mapping_network_inr.load_state_dict(G_ema.mapping_network_inr.state_dict())
        self.nerf_rgb_mapping.load_state_dict(G_ema.nerf_rgb_mapping.state_dict())

    def _map_inr(self, z_inr):
        with torch.no_grad():
            return super()._map_inr(z_inr)
