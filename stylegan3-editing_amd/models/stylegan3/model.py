"""`SG3Generator`: loads / builds the StyleGAN3 decoder used by the encoders, PTI and the editing tools
(API of reference models/stylegan3/model.py:19-65).

Weight-layout contract kept from the reference: a `.pkl` is `pickle.load(f)['G_ema']`, a persistent object that carries
the source of the module it was defined in; anything else is a plain `Generator.state_dict()` loaded strictly, or --
if that fails -- without the `synthesis.input.transform` entry (:59-65).  `config="landscape"` selects the config-T
sizes (:29-40), everything else config-R (:42-54).  `device=` replaces the reference's hard-coded `.cuda()` on the
pickle branch; a generator built from a state dict stays on the CPU until the caller moves it, as in the reference.

Which entry point reaches which kernels:

    .pkl, adopted         this package's `Generator` with the pickle's weights: the native graph (batch-wide HIP modulated
                          convolution, batched weight preparation, fused ToRGB, `GraphedSynthesis`, the PTI backward)
    .pkl, not adopted     the pickled module source, exec'd against this package's `torch_utils` / `dnnlib`: `filtered_lrelu`
                          and `bias_act` run on HIP, the convolutions are the library's grouped convolution
    .pt / state dict      this package's `Generator`: the native graph

A pickle written by another code base (an official checkpoint) unpickles into a class rebuilt from ITS source.
`adopt_generator` replaces such an object by this package's `Generator(**init_kwargs)` holding the same parameters and
buffers when the two are the same network by construction arguments, names and shapes; otherwise the unpickled object is
returned as it is, with one warning that names the reason.  The snapshot layout `{G, D, G_ema, augment_pipe,
training_set_kwargs}` unpickles whole (torch_utils.ops has the operator modules a discriminator / augmentation source
imports); no official weight file is available offline, so that layout is taken from the reference's copy of the upstream
modules (models/styleganxl/training/networks_stylegan2.py:16-21), not from a real checkpoint.
"""
import pickle
import warnings
from enum import Enum
from pathlib import Path
from typing import Optional

import torch

from models.stylegan3.networks_stylegan3 import Generator
from torch_utils import misc

_COMMON = dict(z_dim=512, c_dim=0, w_dim=512, img_channels=3, magnitude_ema_beta=0.5 ** (32 / (20 * 1e3)))
# translation-equivariant config: 3x3 convs, separable 12-tap filters, two mapping layers in the landscape checkpoints
CONFIG_T = dict(_COMMON, channel_base=32768, channel_max=512, mapping_kwargs={'num_layers': 2})
# rotation-equivariant config: 1x1 convs, radial 6-tap filters, twice the channels at a quarter of the output scale
CONFIG_R = dict(_COMMON, channel_base=65536, channel_max=1024, conv_kernel=1, filter_size=6, output_scale=0.25,
                use_radial_filters=True)
_SHAPE_DEPENDENT = 'synthesis.input.transform'


class GeneratorType(str, Enum):
    ALIGNED = "aligned"
    UNALIGNED = "unaligned"

    def __str__(self):
        return str(self.value)


def _adoption_obstacle(obj):
    """None when `obj` is a foreign generator this package's `Generator` can stand in for; else the reason it is not."""
    if not hasattr(obj, 'init_kwargs'):
        return 'it is not a persistent object (no init_kwargs)'
    if type(obj).__name__ != 'Generator':
        return f'its class is {type(obj).__name__}, not Generator'
    if not isinstance(obj, torch.nn.Module):
        return 'it is not a torch.nn.Module'
    return None


def adopt_generator(obj, adopt=True):
    """A generator unpickled from another code base's source -> this package's `Generator` with the same weights.

    Applies to a persistent object of a foreign class named `Generator` whose constructor arguments build this package's
    `Generator` and whose parameters and buffers match the native ones one to one (names and shapes, checked in both
    directions).  The native object takes over the values, each tensor's dtype, `requires_grad` of every parameter, the
    train / eval mode and `init_kwargs`; it stays on the CPU.  An object that is already native is returned untouched, and so
    is everything with `adopt=False`.  Anything else is returned as it is after one warning naming the reason."""
    if not adopt or isinstance(obj, Generator):
        return obj
    reason = _adoption_obstacle(obj)
    native = None
    if reason is None:
        try:
            native = Generator(*getattr(obj, 'init_args', ()), **obj.init_kwargs)
        except Exception as err:  # pylint: disable=broad-except
            reason = f'Generator(**init_kwargs) failed: {type(err).__name__}: {err}'
    if reason is None:
        theirs, ours = dict(misc.named_params_and_buffers(obj)), dict(misc.named_params_and_buffers(native))
        extra, missing = sorted(set(theirs) - set(ours)), sorted(set(ours) - set(theirs))
        shapes = [k for k in ours if k in theirs and ours[k].shape != theirs[k].shape]
        kinds = [k for k in ours if k in theirs and isinstance(ours[k], torch.nn.Parameter) != isinstance(theirs[k], torch.nn.Parameter)]
        if extra:
            reason = f'it has parameters / buffers this package does not: {extra[:3]}'
        elif missing:
            reason = f'it lacks parameters / buffers this package has: {missing[:3]}'
        elif shapes:
            k = shapes[0]
            reason = f'shape of {k} is {list(theirs[k].shape)}, expected {list(ours[k].shape)}'
        elif kinds:
            reason = f'{kinds[0]} is a parameter on one side and a buffer on the other'
    if reason is not None:
        warnings.warn(f'generator not adopted, running its own pickled graph (convolutions on the library): {reason}')
        return obj
    for name, tensor in ours.items():
        tensor.data = tensor.data.to(theirs[name].dtype)
        if isinstance(tensor, torch.nn.Parameter):
            tensor.requires_grad_(theirs[name].requires_grad)
    misc.copy_params_and_buffers(obj, native, require_all=True)
    return native.train(obj.training)


def load_generator_pickle(path, device='cuda', adopt=True):
    """`pickle.load(path)['G_ema']`, adopted onto the native graph (see `adopt_generator`), on `device`."""
    with open(path, 'rb') as fh:
        return adopt_generator(pickle.load(fh)['G_ema'], adopt=adopt).to(device)


def _from_state_dict(net, path):
    state = torch.load(path, map_location='cpu')
    try:
        net.load_state_dict(state, strict=True)
    except RuntimeError:
        # checkpoints saved after a batched call carry a [B,3,3] transform buffer
        net.load_state_dict({k: v for k, v in state.items() if _SHAPE_DEPENDENT not in k}, strict=False)
    return net


class SG3Generator(torch.nn.Module):
    def __init__(self, checkpoint_path: Optional[Path] = None, res: int = 1024, config: str = None, device='cuda',
                 adopt: bool = True):
        super().__init__()
        print(f"Loading StyleGAN3 generator from path: {checkpoint_path}")
        if str(checkpoint_path).endswith("pkl"):
            self.decoder = load_generator_pickle(checkpoint_path, device, adopt=adopt)
        else:
            self.decoder = Generator(img_resolution=res, **(CONFIG_T if config == "landscape" else CONFIG_R))
            if checkpoint_path is not None:
                _from_state_dict(self.decoder, checkpoint_path)
        print('Done!')
