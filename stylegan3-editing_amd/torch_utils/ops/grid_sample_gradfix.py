"""`grid_sample(input, grid)`: bilinear, zero padding, `align_corners=False`, 2-D only
(operator API of reference torch_utils/ops/grid_sample_gradfix.py: `enabled` :22, `grid_sample` :26).

Imported by name from the module source embedded in upstream training snapshots (the augmentation pipeline); the
generator graph of this package does not use it.

With `enabled = False` (the default, as in the reference) the call is `torch.nn.functional.grid_sample`, whose backward
has no derivative of its own.  With `enabled = True` the same interpolation is written out with gathers and elementwise
ops: output = sum over the four neighbouring texels of (bilinear weight) * (texel, or 0 outside the image).  Every step
is an ordinary differentiable torch op, so gradients of any order exist, w.r.t. the image and w.r.t. the grid (the
reference's custom op stops at the image).  The texel indices are piecewise constant in the grid and carry no gradient.
"""
import torch

enabled = False     # True: the arbitrarily differentiable formulation below


def grid_sample(input, grid):  # pylint: disable=redefined-builtin
    if _should_use_custom_op():
        return _bilinear_zero_padded(input, grid)
    return torch.nn.functional.grid_sample(input=input, grid=grid, mode='bilinear', padding_mode='zeros', align_corners=False)


def _should_use_custom_op():
    return bool(enabled)


def _bilinear_zero_padded(image, grid):
    assert image.ndim == 4 and grid.ndim == 4 and grid.shape[0] == image.shape[0] and grid.shape[3] == 2
    n, c, h, w = image.shape
    ho, wo = grid.shape[1:3]
    # [-1, 1] spans the image from the outer edge of the first texel to the outer edge of the last one
    px = ((grid[..., 0] + 1) * w - 1) / 2
    py = ((grid[..., 1] + 1) * h - 1) / 2
    x0, y0 = px.detach().floor(), py.detach().floor()
    fx, fy = px - x0, py - y0
    flat = image.reshape(n, c, h * w)
    out = None
    for dy, wy in ((0, 1 - fy), (1, fy)):
        for dx, wx in ((0, 1 - fx), (1, fx)):
            xi, yi = x0 + dx, y0 + dy
            inside = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
            index = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).to(torch.int64).reshape(n, 1, ho * wo).expand(n, c, ho * wo)
            texel = flat.gather(2, index).reshape(n, c, ho, wo)
            term = texel * (wx * wy * inside.to(image.dtype)).unsqueeze(1)
            out = term if out is None else out + term
    return out
