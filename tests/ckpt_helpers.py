"""Helpers shared by the checkpoint-loading tests: stand-in "foreign" generators / discriminators rebuilt from source
text the way torch_utils.persistence rebuilds the classes of an official pickle, with the synthetic weights."""
import contextlib
import os
import pickle

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
EXTRA_BUFFER_HOOK = '# EXTRA_BUFFER_HOOK'


def source_text(name='foreign_generator_src.py'):
    with open(os.path.join(HERE, name)) as fh:
        return fh.read()


def foreign_module(text):
    """The module torch_utils.persistence execs for `text` (one per distinct text, as for a pickle's module_src)."""
    from torch_utils import persistence
    return persistence._src_to_module(text)


def load_synth(G, seed=0):
    from synth_weights import synth_state_dict
    man = {k: list(v.shape) for k, v in G.state_dict().items() if not k.endswith('extra_stat')}    # a variant's own buffer
    sd = synth_state_dict(man, seed=seed, input_bandwidth=float(G.synthesis.input.bandwidth))
    missing, unexpected = G.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith(('_filter', 'extra_stat')) for k in missing), (missing, unexpected)
    return G


def standin_generator(cfg, text=None, class_name='Generator', **extra_kwargs):
    """A generator of the stand-in source's class with the synthetic weights, in eval mode, gradients off."""
    from synth_weights import CONFIGS
    cls = getattr(foreign_module(source_text() if text is None else text), class_name)
    return load_synth(cls(**CONFIGS[cfg], **extra_kwargs)).eval().requires_grad_(False)


def standin_discriminator(res=64):
    return foreign_module(source_text('foreign_discriminator_src.py')).Discriminator(c_dim=0, img_resolution=res, img_channels=3)


def write_pickle(path, **entries):
    with open(path, 'wb') as fh:
        pickle.dump(entries, fh)
    return str(path)


def write_state_dict(path, G):
    torch.save(G.state_dict(), path)
    return str(path)


@contextlib.contextmanager
def _tiny_sizes(cfg):
    """`SG3Generator`'s state-dict branch builds CONFIG_T / CONFIG_R at full width; shrink that table to the tiny network's
    sizes for the duration of one load (as tests/test_product_cpu.py does)."""
    from models.stylegan3 import model as m
    from synth_weights import CONFIGS
    table = m.CONFIG_T if cfg.startswith('T') else m.CONFIG_R
    saved = dict(table)
    table.update({k: CONFIGS[cfg][k] for k in ('z_dim', 'w_dim', 'channel_base', 'channel_max')})
    try:
        yield
    finally:
        table.clear()
        table.update(saved)


def sg3_from_state_dict(path, cfg, device='cpu'):
    """The decoder `SG3Generator` builds from a `.pt` state dict of the tiny configuration `cfg`."""
    from models.stylegan3 import model as m
    from synth_weights import CONFIGS
    with _tiny_sizes(cfg):
        wrapper = m.SG3Generator(checkpoint_path=path, res=CONFIGS[cfg]['img_resolution'], config='landscape' if cfg.startswith('T') else None)
    return wrapper.decoder.eval().requires_grad_(False).to(device)
