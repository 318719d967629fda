"""Case tables shared by tests/golden/make_golden_ckpt_ops.py (which runs the reference) and the tests of the operator
modules that upstream snapshot sources import (`conv2d_resample`, `fma`, `grid_sample_gradfix`).

Inputs are regenerated from seeds; tests/golden/ckpt_ops.npz holds the reference's outputs only."""
import itertools

import numpy as np

from golden_cases import rand

RESAMPLE_FILTER = [1, 3, 3, 1]
N, C_IN, C_OUT = 2, 4, 6

# name -> dict(up, down, k, groups, flip_weight, padding): the full product of the values an upstream discriminator /
# synthesis block can ask for
CONV2D_RESAMPLE_CASES = {
    f'u{up}d{down}k{k}g{groups}{"corr" if flip_weight else "conv"}p{padding}':
        dict(up=up, down=down, k=k, groups=groups, flip_weight=flip_weight, padding=padding)
    for up, down, k, groups, flip_weight, padding in itertools.product([1, 2], [1, 2], [1, 3], [1, 2], [True, False], [0, 1])
}


def conv2d_resample_inputs(c, h=9, w=11, dtype=np.float32):
    """(x [N, C_IN, h, w], weight [C_OUT, C_IN / groups, k, k]).  The weight carries the 1 / sqrt(fan_in) gain every caller of
    this op applies and x ~ N(0, 1/16): with the up^2 gain of the upsampling cases the outputs then stay below 2 in magnitude,
    where one float32 ulp is 1.2e-7 -- the 1e-6 absolute tolerance of the operator tests is then several ulps for every case
    (at |y| in [4, 8), reached with unit-variance x, it would be two)."""
    fan_in = (C_IN // c['groups']) * c['k'] ** 2
    x = rand(51, N, C_IN, h, w) * 0.25
    wt = rand(52, C_OUT, C_IN // c['groups'], c['k'], c['k']) / np.sqrt(fan_in)
    return x.astype(dtype), wt.astype(dtype)


def fma_inputs(dtype=np.float32, spatial=(4, 5)):
    """a [2,3,h,w] * b [3,1,w] + c [h,1]: b and c are broadcast along leading, inner and trailing axes."""
    h, w = spatial
    return rand(61, 2, 3, h, w).astype(dtype), rand(62, 3, 1, w).astype(dtype), rand(63, h, 1).astype(dtype)


def grid_sample_inputs(dtype=np.float32, hw=(7, 9), grid_hw=(8, 8)):
    """image [2,3,h,w] and a sampling grid reaching 20 % beyond the image on every side (zero padding is exercised)."""
    image = rand(71, 2, 3, *hw)
    grid = np.random.RandomState(72).uniform(-1.2, 1.2, size=(2, *grid_hw, 2))
    return image.astype(dtype), grid.astype(dtype)
