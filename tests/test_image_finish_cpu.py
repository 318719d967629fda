"""CPU: the host half of the image-finishing kernel (csrc/sg3_image_finish.hip).  The fixed-point bicubic tables that
libsg3hip exports, applied with numpy integer arithmetic in the kernel's order (horizontal pass into uint8, then vertical),
give exactly what PIL's Image.resize gives; the tensor2im arithmetic restated in float32 numpy equals utils.common.tensor2im
on values that land on k/255 boundaries; the ctypes parameter block has the header's field order."""
import ctypes
import os
import re

import numpy as np
import pytest

from helpers import HERE

ROOT = os.path.dirname(HERE)

# (in_w, in_h) -> (out_w, out_h), PIL order
SIZES = [((1024, 1024), (256, 256)), ((1024, 1024), (1024, 1024)), ((256, 256), (1024, 1024)), ((1000, 1000), (256, 256)),
         ((257, 257), (256, 256)), ((512, 384), (256, 192)), ((3, 3), (1, 1))]


def tables(n_in, n_out):
    from torch_utils import _sg3abi
    lib = _sg3abi.load()
    k = lib.sg3_resample_coeffs(n_in, n_out, None, None)
    assert k > 0
    bounds = np.zeros([n_out, 2], np.int32)
    coeffs = np.zeros([n_out, k], np.int32)
    assert lib.sg3_resample_coeffs(n_in, n_out, bounds.ctypes.data, coeffs.ctypes.data) == k
    return bounds, coeffs


def resample_axis(u8, n_out, axis):
    """One pass of the kernel along `axis` of an [H, W, 3] uint8 array: (1 << 21) + sum_t u8[xmin + t] * k[t], >> 22, clamped."""
    bounds, coeffs = tables(u8.shape[axis], n_out)
    a = np.moveaxis(u8.astype(np.int64), axis, 0)
    out = np.empty((n_out,) + a.shape[1:], np.int64)
    for o in range(n_out):
        xmin, n = bounds[o]
        ss = np.full(a.shape[1:], 1 << 21, np.int64)
        for t in range(n):
            ss += a[xmin + t] * int(coeffs[o, t])
        assert np.abs(ss).max() < 2 ** 31                     # the kernel accumulates in int32, as PIL does
        out[o] = np.clip(ss >> 22, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def finish_numpy(u8, size):
    w, h = size
    out = u8
    if w != u8.shape[1]:
        out = resample_axis(out, w, 1)
    if h != u8.shape[0]:
        out = resample_axis(out, h, 0)
    return out


@pytest.mark.parametrize('src,dst', SIZES)
def test_tables_reproduce_pil_resize(src, dst):
    from PIL import Image
    rng = np.random.RandomState(src[0] + 7 * dst[0] + dst[1])
    u8 = rng.randint(0, 256, size=(src[1], src[0], 3)).astype(np.uint8)
    # sharp edges and saturated blocks push the taps' overshoot into the clamps
    u8[: src[1] // 3, : src[0] // 2] = 255
    u8[src[1] // 2:, src[0] // 3: src[0] // 2] = 0
    ref = np.array(Image.fromarray(u8).resize(dst))
    got = finish_numpy(u8, dst)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), int(np.abs(got.astype(int) - ref).max())


def test_table_shape_and_bad_sizes():
    from torch_utils import _sg3abi
    lib = _sg3abi.load()
    assert lib.sg3_resample_coeffs(1024, 256, None, None) == 17        # support 2 * 4 -> 2 * 8 + 1 taps
    assert lib.sg3_resample_coeffs(256, 1024, None, None) == 5
    bounds, coeffs = tables(1024, 256)
    assert (bounds[:, 0] >= 0).all() and (bounds.sum(axis=1) <= 1024).all()
    assert (np.abs(coeffs.sum(axis=1) - (1 << 22)) <= 17).all()        # each row is a partition of unity in fixed point
    assert lib.sg3_resample_coeffs(0, 4, None, None) == _sg3abi.SG3_BAD_ARG


def tensor2im_numpy(x):
    """utils/common.py tensor2im restated: float32 (x + 1) / 2, clip to [0, 1], * 255, truncation."""
    x = np.asarray(x, np.float32)
    return (np.clip((x + np.float32(1)) / np.float32(2), 0, 1) * np.float32(255)).astype(np.uint8)


def test_tensor2im_arithmetic_on_boundaries():
    import torch
    from utils.common import tensor2im
    k = np.arange(256, dtype=np.float64)
    base = (k / 255.0) * 2 - 1                                       # x whose image lands on k / 255 exactly (in real arithmetic)
    vals = np.concatenate([base, np.nextafter(base.astype(np.float32), np.float32(2)), np.nextafter(base.astype(np.float32), np.float32(-2)),
                           [-1.3, -1.0, -0.0, 0.0, 1.0, 1.3, 0.999999, -0.999999]]).astype(np.float32)
    n = 32 * 32
    vals = np.resize(vals, 3 * n).reshape(3, 32, 32)
    ref = np.array(tensor2im(torch.from_numpy(vals)))
    assert np.array_equal(tensor2im_numpy(vals.transpose(1, 2, 0)), ref)


def test_image_finish_struct_matches_header():
    from torch_utils import _sg3abi
    with open(os.path.join(ROOT, 'include', 'sg3_ops.h')) as f:
        src = f.read()
    cname = 'sg3_image_finish_params'
    body = re.search(r'typedef struct ' + cname + r' \{(.*?)\} ' + cname + ';', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            parts = decl.split(',')
            for nm in [parts[0].split()[-1]] + [q.strip() for q in parts[1:]]:
                names.append(re.sub(r'\[\d+\]|\*', '', nm))
    assert names == [n for n, _ in _sg3abi.ImageFinishParams._fields_]
    assert ctypes.sizeof(_sg3abi.ImageFinishParams) == 8 + 32 + 8 + 32 + 5 * 4 + 4 + 8 + 8 + 4 + 4 + 8 + 8 + 4 + 4
