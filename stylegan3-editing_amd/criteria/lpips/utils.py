"""Helpers of the LPIPS criterion (reference criteria/lpips/utils.py).  Nothing is downloaded here: weights come from the caller."""
from collections import OrderedDict

import torch


def normalize_activation(x, eps=1e-10):
    """Unit-normalise every pixel over its channels."""
    norm_factor = torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True))
    return x / (norm_factor + eps)


def load_state(source):
    """A state dict, given as one or as the path of a `torch.save`d one (optionally wrapped as {'state_dict': ...})."""
    if isinstance(source, dict):
        state = source
    else:
        state = torch.load(source, map_location='cpu')
    if isinstance(state, dict) and isinstance(state.get('state_dict'), dict):
        state = state['state_dict']
    return state


def get_state_dict(source):
    """The state dict of `LinLayers` from the published linear-layer weights: keys `lin0.model.1.weight` become `0.1.weight`
    (the reference's renaming); already renamed keys pass through."""
    new_state_dict = OrderedDict()
    for key, val in load_state(source).items():
        new_key = key.replace('lin', '').replace('model.', '')
        new_state_dict[new_key] = val
    return new_state_dict


def alexnet_features_state(source):
    """The `layers.*` entries of `AlexNet` from a torchvision AlexNet state dict: `features.N.*` kept, `classifier.*` ignored."""
    out = OrderedDict()
    for key, val in load_state(source).items():
        if key.startswith('features.'):
            out[key[len('features.'):]] = val
    return out
