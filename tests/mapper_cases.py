"""Cases shared by the StyleCLIP latent mapper tests and tests/golden/make_golden_styleclip_mapper.py: options, seeded weights
(non-zero biases, one RandomState per tensor so a group's weights do not depend on which other groups exist), seeded inputs and
an fp64 numpy restatement of the mapper (reference editing/styleclip_mapper/latent_mappers.py)."""
import math
import types
import zlib

import numpy as np

LEVELS = {'course_mapping': (0, 5), 'medium_mapping': (5, 8), 'fine_mapping': (8, 16)}
CASES = {
    'levels_all': dict(mapper_type='LevelsMapper', no_coarse_mapper=False, no_medium_mapper=False, no_fine_mapper=False),
    'levels_no_coarse': dict(mapper_type='LevelsMapper', no_coarse_mapper=True, no_medium_mapper=False, no_fine_mapper=False),
    'levels_coarse_only': dict(mapper_type='LevelsMapper', no_coarse_mapper=False, no_medium_mapper=True, no_fine_mapper=True),
    'single': dict(mapper_type='SingleMapper', no_coarse_mapper=False, no_medium_mapper=False, no_fine_mapper=False),
}
LR_MUL = 0.01


def opts(case, **kw):
    o = dict(CASES[case])
    o.update(kw)
    return types.SimpleNamespace(**o)


def groups(o):
    """[(state-dict prefix, (level_begin, level_end))] of the enabled groups."""
    if o.mapper_type == 'SingleMapper':
        return [('mapping', (0, 16))]
    flags = {'course_mapping': o.no_coarse_mapper, 'medium_mapping': o.no_medium_mapper, 'fine_mapping': o.no_fine_mapper}
    return [(name, LEVELS[name]) for name in LEVELS if not flags[name]]


def _rs(key, seed):
    return np.random.RandomState((zlib.crc32(key.encode()) + 7919 * int(seed)) % (2 ** 32))


def state_dict(o, seed=0, w_scale=1.0):
    """Mapper state dict (numpy float32): stored weights ~ N(0, 1) / lr_mul (EqualLinear's own init) times w_scale, biases
    ~ N(0, 1) / lr_mul / 10 (so b * lr_mul ~ 0.1: non-zero)."""
    sd = {}
    for prefix, _ in groups(o):
        for i in range(1, 5):
            k = f'{prefix}.mapping.{i}'
            sd[k + '.weight'] = (_rs(k + '.weight', seed).randn(512, 512) / LR_MUL * w_scale).astype(np.float32)
            sd[k + '.bias'] = (_rs(k + '.bias', seed).randn(512) / LR_MUL / 10).astype(np.float32)
    return sd


def inputs(seed=1):
    """[6, 16, 512] float32: three seeded latents, an all-zero latent (the 1e-8 of PixelNorm), latent 0 x 1e3 and x 1e-3."""
    x = _rs('latents', seed).randn(3, 16, 512).astype(np.float32)
    return np.concatenate([x, np.zeros_like(x[:1]), x[:1] * np.float32(1e3), x[:1] * np.float32(1e-3)]).astype(np.float32)


def latents(n, seed=1, scale=1.0):
    return (_rs(f'latents{n}', seed).randn(n, 16, 512) * scale).astype(np.float32)


def mapper_fp64(sd, o, x, per_feature_norm=False):
    """delta = mapper(x) in float64.  per_feature_norm=True normalises over the feature axis instead of the level axis (the
    wrong reading of PixelNorm(dim=1), for the test that must tell them apart)."""
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    scale = LR_MUL / math.sqrt(512)
    for prefix, (b, e) in groups(o):
        h = x[:, b:e, :]
        h = h / np.sqrt(np.mean(h ** 2, axis=2 if per_feature_norm else 1, keepdims=True) + 1e-8)
        for i in range(1, 5):
            w = sd[f'{prefix}.mapping.{i}.weight'].astype(np.float64) * scale
            bias = sd[f'{prefix}.mapping.{i}.bias'].astype(np.float64) * LR_MUL
            h = h @ w.T + bias
            h = np.where(h > 0, h, 0.2 * h) * math.sqrt(2)
        out[:, b:e, :] = h
    return out


def build_mapper(o, sd, device='cpu'):
    """The package's mapper module for options `o` with the numpy state dict `sd`, in eval mode."""
    import torch
    from editing.styleclip_mapper import latent_mappers
    m = latent_mappers.SingleMapper(o) if o.mapper_type == 'SingleMapper' else latent_mappers.LevelsMapper(o)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m.eval().to(device)
