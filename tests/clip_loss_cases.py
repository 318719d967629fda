"""Cases shared by the CLIP loss tests and tests/golden/make_golden_clip_loss.py: the seeded `small` tower of tests/clip_cases.py at
w_scale 1 and 3, three token rows, and seeded images at the StyleGAN sizes 64 (pooling window 2) and 32 (window 1: pure
upsampling)."""
import types

import numpy as np

import clip_cases as cases

CFG = 'small'
W_SCALES = (1, 3)
N_TEXT = 3
GOLDEN_IMAGES = {64: 2, 32: 1}            # stylegan_size -> batch


def images(size, n, seed=1):
    """float32 [n, 3, size, size] ~ N(0, 0.5^2)."""
    return (0.5 * cases._rs(f'clip_loss_images{size}', seed).randn(n, 3, size, size)).astype(np.float32)


def tokens():
    return cases.tokens(CFG, N_TEXT)


def opts(size):
    return types.SimpleNamespace(stylegan_size=int(size), clip_checkpoint_path=None)
