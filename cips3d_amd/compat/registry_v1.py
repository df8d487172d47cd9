"""Registration of the generator_v1 drop-in models in the reference's model registry.

The AFHQ recipes (exp/cips3d/configs/afhq_exp.yaml:24-27) and ffhq_exp_v1.yaml build
`exp.cips3d.models.generator_v1.GeneratorNerfINR` / `..._freeze_NeRF` (generator_v1.py:1158, 1970), not the classes of
generator.py that `registry` serves.  Importing THIS module registers the MI355X versions of those two classes under its own
name, so the reference-side change is again only in the YAML:

    G_cfg_3D2D:
      register_modules: [cips3d_amd.compat.registry_v1]
      name: cips3d_amd.compat.registry_v1.GeneratorNerfINR         # or ...GeneratorNerfINR_freeze_NeRF

The discriminator of those recipes is the v0 one: select it through `cips3d_amd.compat.registry`.
"""
from ..generator_v1 import GeneratorNerfINR, GeneratorNerfINR_freeze_NeRF

CLASSES = (GeneratorNerfINR, GeneratorNerfINR_freeze_NeRF)


def register(registry=None, name_prefix=__name__):
    """Register the two classes in `registry` (default: tl2.proj.fvcore.MODEL_REGISTRY) -> list of registered names."""
    if registry is None:
        from tl2.proj.fvcore import MODEL_REGISTRY as registry
    for cls in CLASSES:
        registry.register(name_prefix=name_prefix)(cls)
    return [f"{name_prefix}.{cls.__name__}" for cls in CLASSES]


try:                                   # `register_modules: [cips3d_amd.compat.registry_v1]` -> registered on import
    REGISTERED = register()
except ImportError:                    # tl2 not installed (this repo's own tests / bench): call register(registry) yourself
    REGISTERED = []
