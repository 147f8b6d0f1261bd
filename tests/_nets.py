"""Small models and their weights for the GPU tests: a deterministic state whose BatchNorm running statistics are off the identity, and
the small PHISeg3D the volume tests run.  Plain helpers: the device is touched only when a model is built."""
import torch

import oracle
from tests import _golden as G


def off_identity_state(spec_or_meta, seed=91):
    """oracle.deterministic_state_dict of a spec (or of the spec in a golden meta) with eval-mode BatchNorm far from the identity"""
    spec = G.spec_of(spec_or_meta) if isinstance(spec_or_meta, dict) else spec_or_meta
    sd = oracle.deterministic_state_dict(spec, seed=seed)
    for k, v in sd.items():
        n = torch.arange(v.numel(), dtype=torch.float32).reshape(v.shape)
        if k.endswith("running_mean"):
            v += 0.3 * torch.cos(1.7 * n + 0.3)
        elif k.endswith("running_var"):
            v *= 1.0 + 0.6 * torch.sin(2.3 * n + 1.1)
    return sd


def small_phiseg3d(meta, sd=None, graphs=False, reversible=False):
    """PHISeg3D of a golden meta (input_channels, num_classes, filters, latent_levels, dhw) in eval mode, with `sd` loaded if given"""
    from unet_zoo_amd.models.phiseg3D import PHISeg3D
    net = PHISeg3D(meta["input_channels"], meta["num_classes"], meta["filters"], latent_levels=meta["latent_levels"], reversible=reversible,
                   image_size=(meta["input_channels"], *meta["dhw"]))
    if sd is not None:
        res = net.load_state_dict(sd)
        assert not res.missing_keys and not res.unexpected_keys
    net.eval()
    net.enable_graphs(graphs)
    return net
