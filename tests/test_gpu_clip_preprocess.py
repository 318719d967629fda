"""GPU: the fused CLIP preprocessing kernel (csrc/sg3_clip_preprocess.hip) against the fp64 restatement in
tests/delta_i_c_cases.py, with the error model of DESIGN.md 3.7 / 3.8: the kernel may miss the restatement by at most twice what
torch's own float32 composite misses it by on the same input, plus 1e-7 of the largest reference value."""
import numpy as np
import pytest
import torch

import delta_i_c_cases as cases
from helpers import maxabs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_refs = {}


def case(shape, scale):
    """(input on the device, fp64 reference), computed once per (shape, scale) and left unchanged."""
    key = (shape, scale)
    if key not in _refs:
        b, hh, ww, h, w = shape
        x = cases.noise((b, 3, hh, ww), scale)
        _refs[key] = (torch.from_numpy(x).to(DEV), cases.preprocess_ref64(x, (h, w)))
    return _refs[key]


def check(got, x, ref, size):
    from torch_utils.ops.clip_preprocess import composite
    torch32 = composite(x, size).cpu().numpy()
    err, err32 = maxabs(got.cpu().numpy(), ref), maxabs(torch32, ref)
    bound = 2 * err32 + 1e-7 * float(np.abs(ref).max())
    print(f'clip_preprocess {tuple(x.shape)} -> {size}: max|hip - ref| = {err:.3e}, max|torch32 - ref| = {err32:.3e}, bound {bound:.3e}')
    assert err <= bound
    return torch32


@pytest.mark.parametrize('scale', [1.0, 3.0])
@pytest.mark.parametrize('shape', cases.SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_kernel_matches_fp64_restatement(shape, scale):
    from torch_utils import _sg3abi
    from torch_utils.ops.clip_preprocess import clip_preprocess
    b, hh, ww, h, w = shape
    x, ref = case(shape, scale)
    before = _sg3abi.launch_count
    got = clip_preprocess(x, size=(h, w))
    assert _sg3abi.launch_count - before == 1                                # one forward per call
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (b, 3, h, w)
    torch32 = check(got, x, ref, (h, w))
    if (hh, ww) == (h, w):
        assert np.array_equal(got.cpu().numpy(), torch32)                     # identity scale: t = 0 everywhere
    if scale == 3.0:
        lo, hi = float(got[:, 0].min()), float(got[:, 0].max())
        assert lo == (0 - np.float32(cases.CLIP_MEAN[0])) / np.float32(cases.CLIP_STD[0])
        assert hi == (1 - np.float32(cases.CLIP_MEAN[0])) / np.float32(cases.CLIP_STD[0])


def test_strided_views():
    from torch_utils.ops.clip_preprocess import clip_preprocess
    x, _ = case((2, 256, 256, 224, 224), 1.0)
    view = x[:, :, 4:-4, 4:-4]
    assert not view.is_contiguous()
    check(clip_preprocess(view), view, cases.preprocess_ref64(view.cpu().numpy()), (224, 224))
    assert torch.equal(clip_preprocess(view), clip_preprocess(view.contiguous()))
    cl = x.contiguous(memory_format=torch.channels_last)
    assert cl.stride() != x.stride()
    assert torch.equal(clip_preprocess(cl), clip_preprocess(x))
    # a strided destination, and constants other than CLIP's
    out = torch.zeros([2, 3, 31, 2 * 47], device=DEV)
    m, s = (0.1, 0.2, 0.3), (0.5, 2.0, 4.0)
    ret = clip_preprocess(x, (31, 47), m, s, out=out[:, :, :, ::2])
    assert ret.data_ptr() == out.data_ptr() and float(out[:, :, :, 1::2].abs().max()) == 0
    ref = cases.preprocess_ref64(x.cpu().numpy(), (31, 47), m, s)
    assert maxabs(out[:, :, :, ::2].cpu().numpy(), ref) <= 2e-5


@pytest.mark.parametrize('shape', [(3, 37, 53, 224, 224), (2, 224, 224, 224, 224), (1, 224, 100, 224, 224)], ids=['resize', 'identity', 'one-axis'])
def test_nan_pixel_mask_equals_composite(shape):
    from torch_utils.ops.clip_preprocess import clip_preprocess, composite
    b, hh, ww, h, w = shape
    x = torch.from_numpy(cases.noise((b, 3, hh, ww), 1.0)).to(DEV)
    x[b - 1, 1, hh // 3, ww // 2] = float('nan')
    got, want = torch.isnan(clip_preprocess(x, (h, w))), torch.isnan(composite(x, (h, w)))
    assert int(want.sum()) > 0 and int(want[:, 0].sum()) == 0 and int(want[:, 2].sum()) == 0
    assert torch.equal(got, want)


def test_gradient_takes_the_composite():
    from torch_utils import _sg3abi
    from torch_utils.ops.clip_preprocess import clip_preprocess
    x = torch.from_numpy(cases.noise((1, 3, 37, 53), 1.0)).to(DEV).requires_grad_(True)
    before = _sg3abi.launch_count
    y = clip_preprocess(x)
    assert _sg3abi.launch_count == before and y.requires_grad
    y.square().sum().backward()
    assert x.grad is not None and float(x.grad.abs().sum()) > 0
    with torch.no_grad():                                                     # the same tensor with no gradient recorded: the kernel
        clip_preprocess(x)
    assert _sg3abi.launch_count == before + 1
    y64 = clip_preprocess(x.detach().double())
    assert y64.dtype == torch.float64 and _sg3abi.launch_count == before + 1
