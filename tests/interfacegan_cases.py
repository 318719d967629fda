"""Shared case builders of the InterFaceGAN editing tests and their fixture (tests/golden/make_golden_interfacegan.py): seeded
latents, synthetic directions (the pretrained boundaries are not available offline) and per-image landmark transforms.

The case sequence runs on ONE generator, in order, because the reference's editor leaves its user transform in the generator:
  A  'age',   factor_range (-2, 2), the [N,3,3] landmark transforms
  B  np.random.seed(5), 'smile', factor_range (-1, 2), no transforms given  -> one random draw reused for all factors
  C  np.random.seed(7), 'pose', factor 3 (single mode)                       -> one random draw
  D  'Male',  factor_range (0, 2), apply_user_transformations=False          -> the generator's transform (C's) as it is
  anim: the reference's animation loop over case A's latents of image 0, N_ANIM transitions per segment."""
import numpy as np

from synth_weights import make_user_transform, synth_ws

NAMES = ('age', 'smile', 'pose', 'Male')
N_ANIM = 3


def directions(w_dim, scale=0.15):
    return {name: (np.random.RandomState(40 + i).randn(1, w_dim) * scale).astype(np.float32) for i, name in enumerate(NAMES)}


def latents(num_ws, w_dim, n=2):
    return synth_ws(n, num_ws, w_dim, seed=31)


def landmarks(n=2):
    return np.stack([make_user_transform((0.03 * (i + 1), -0.02 * i), 7.0 - 12.0 * i) for i in range(n)]).astype(np.float32)


CASES = [
    dict(key='A', direction='age', factor_range=(-2, 2), transforms=True, apply=True, seed=None),
    dict(key='B', direction='smile', factor_range=(-1, 2), transforms=False, apply=True, seed=5),
    dict(key='C', direction='pose', factor=3, transforms=False, apply=True, seed=7),
    dict(key='D', direction='Male', factor_range=(0, 2), transforms=False, apply=False, seed=None),
]


def edit_kwargs(case, landmark_tensor):
    kw = dict(direction=case['direction'], apply_user_transformations=case['apply'])
    if 'factor_range' in case:
        kw['factor_range'] = case['factor_range']
    else:
        kw['factor'] = case['factor']
    if case['transforms']:
        kw['user_transforms'] = landmark_tensor
    return kw
