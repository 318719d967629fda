"""Cases shared by the StyleCLIP mapper training tests and tests/golden/make_golden_styleclip_mapper_train.py: an fp64 numpy
restatement of the mapper's gradients (with respect to the input and to the STORED weights and biases), seeded upstream gradients
dDelta / dOut, and the seeded gradient sequence of the Ranger trajectory.  Options, weights and latents are tests/mapper_cases.py."""
import math

import numpy as np

import mapper_cases as cases

ALPHA = 0.1
GOLDEN_CASES = ('levels_all', 'levels_no_coarse', 'single')
W_LATTICE = (slice(None, None, 37), slice(None, None, 41))     # weight gradients are stored on this lattice in the golden file
RANGER_STEPS = 13
RANGER_LR = 0.5
RANGER_SHAPES = {'w': (8, 8), 'b': (8,)}


def upstream(n, which, seed=3):
    """(dDelta, dOut) float32 [n, 16, 512] ~ N(0, 1), either None when `which` ('delta', 'out', 'both') leaves it out."""
    d = cases._rs(f'dDelta{n}', seed).randn(n, 16, 512).astype(np.float32) if which in ('delta', 'both') else None
    o = cases._rs(f'dOut{n}', seed).randn(n, 16, 512).astype(np.float32) if which in ('out', 'both') else None
    return d, o


def mapper_grads_fp64(sd, o, x, d_delta=None, d_out=None, alpha=ALPHA):
    """(dx [N, 16, 512], {state-dict key: gradient}) in float64 of  sum(dDelta * delta) + sum(dOut * (x + alpha * delta))."""
    x = np.asarray(x, np.float64)
    dx = np.zeros_like(x) if d_out is None else np.asarray(d_out, np.float64).copy()
    dd = np.zeros_like(x)
    if d_delta is not None:
        dd = dd + np.asarray(d_delta, np.float64)
    if d_out is not None:
        dd = dd + alpha * np.asarray(d_out, np.float64)
    grads = {}
    scale = cases.LR_MUL / math.sqrt(512)
    s2 = math.sqrt(2)
    for prefix, (b, e) in cases.groups(o):
        xg = x[:, b:e, :]
        lg = e - b
        r = 1.0 / np.sqrt(np.mean(xg ** 2, axis=1, keepdims=True) + 1e-8)
        hs, zs = [xg * r], []
        for i in range(1, 5):
            w = sd[f'{prefix}.mapping.{i}.weight'].astype(np.float64) * scale
            z = hs[-1] @ w.T + sd[f'{prefix}.mapping.{i}.bias'].astype(np.float64) * cases.LR_MUL
            zs.append(z)
            hs.append(np.where(z > 0, z, 0.2 * z) * s2)
        dh = dd[:, b:e, :]
        for i in range(4, 0, -1):
            dz = dh * np.where(zs[i - 1] > 0, s2, 0.2 * s2)
            w = sd[f'{prefix}.mapping.{i}.weight'].astype(np.float64) * scale
            grads[f'{prefix}.mapping.{i}.weight'] = (dz.reshape(-1, 512).T @ hs[i - 1].reshape(-1, 512)) * scale
            grads[f'{prefix}.mapping.{i}.bias'] = dz.reshape(-1, 512).sum(0) * cases.LR_MUL
            dh = dz @ w
        dx[:, b:e, :] += r * dh - xg * r ** 3 * (1.0 / lg) * np.sum(dh * xg, axis=1, keepdims=True)
    return dx, grads


def ranger_init():
    """Initial parameters of the Ranger trajectory, float32."""
    return {k: cases._rs(f'ranger_p_{k}', 0).randn(*s).astype(np.float32) for k, s in RANGER_SHAPES.items()}


def ranger_grads(step, shapes=None, seed=0):
    """The gradients of 1-based `step`, float32 ~ N(0, 1) + 0.3 (a non-zero row mean, so centralisation shows)."""
    shapes = RANGER_SHAPES if shapes is None else shapes
    return {k: (cases._rs(f'ranger_g_{k}_{step}', seed).randn(*s) + 0.3).astype(np.float32) for k, s in shapes.items()}
