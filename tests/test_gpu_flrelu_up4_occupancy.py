"""GPU: the up-4 separable plain forward of the streaming filtered_lrelu kernel has two forms -- the default, whose up taps sit in
scalar registers and single vector register pairs (at most 128 VGPRs: four waves per SIMD), and the earlier, wider one (three waves),
which sg3_filtered_lrelu_force_up4_wide(1) selects.  Both form every output from the same products in the same order, so their
outputs must be equal bit for bit: at every up-4 layer geometry of T-1024 (L2, L4, L5, L7, L9, L10; channels, sizes, filters and
padding from the built generator) at batch 1 and 2, with a non-finite sample, and with samples above the fast-activation threshold
(the redo pass)."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
UP4_LAYERS = ['L2', 'L4', 'L5', 'L7', 'L9', 'L10']


@functools.lru_cache(maxsize=None)
def _layers():
    """{Lk: (channels, x side, call arguments, fu, fd)} of the full-size T generator (filters as the product designs them)."""
    from helpers import build_product_generator
    G = build_product_generator('T1024')
    out = {}
    for name in G.synthesis.layer_names:
        L = getattr(G.synthesis, name)
        if not L.is_torgb:
            kw = dict(up=int(L.up_factor), down=int(L.down_factor), padding=[int(v) for v in L.padding], gain=float(np.sqrt(2)), slope=0.2,
                      clamp=L.conv_clamp, flip_filter=False)               # as SynthesisLayer.forward calls the op
            out[name.split('_')[0]] = (int(L.out_channels), int(L.in_size[0]) + L.conv_kernel - 1, kw, L.up_filter.to(DEV), L.down_filter.to(DEV))
    return out


def test_the_up4_layers_are_the_six_of_the_flagship():
    assert [k for k, v in _layers().items() if v[2]['up'] == 4] == UP4_LAYERS


@contextlib.contextmanager
def _wide_form():
    from torch_utils import _sg3abi as abi
    lib = abi.load()
    prev = lib.sg3_filtered_lrelu_force_up4_wide(1)
    try:
        yield
    finally:
        lib.sg3_filtered_lrelu_force_up4_wide(prev)


def _both(x, b, fu, fd, kw):
    """(default form, wide form) outputs of one call."""
    from torch_utils.ops import filtered_lrelu as fl
    y = fl.filtered_lrelu(x, fu=fu, fd=fd, b=b, **kw)
    with _wide_form():
        ref = fl.filtered_lrelu(x, fu=fu, fd=fd, b=b, **kw)
    torch.cuda.synchronize()
    return y, ref


def _bit_equal(a, b):
    ints = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(ints), b.view(ints))


def _inputs(layer, n, seed, dtype=torch.float32):
    """Seeded inputs at the magnitudes the layers see: the convolution before the op is demodulated and its input normalised to
    unit RMS, so samples are of order 1 with a tail of a few units; biases of order 0.5."""
    c, side, kw, fu, fd = _layers()[layer]
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = (torch.randn([n, c, side, side], device=DEV, generator=gen) * 1.5).to(dtype)
    b = (torch.randn([c], device=DEV, generator=gen) * 0.5).to(dtype)
    return x, b, fu, fd, kw


def _threshold(fu, kw):
    from torch_utils import _sg3abi as abi
    fu_host = fu.cpu().contiguous()
    return float(abi.load().sg3_filtered_lrelu_fast_threshold(fu_host.data_ptr(), int(fu_host.shape[0]), kw['up'], ctypes.c_float(kw['gain']),
                                                              ctypes.c_float(kw['slope']), ctypes.c_float(kw['clamp'])))


@pytest.mark.parametrize('n', [1, 2])
@pytest.mark.parametrize('layer', UP4_LAYERS)
def test_default_form_equals_wide_form_bit_for_bit(layer, n):
    x, b, fu, fd, kw = _inputs(layer, n, seed=1000 * n + int(layer[1:]))
    assert kw['up'] == 4 and kw['down'] == 2 and fu.ndim == 1 and fd.ndim == 1
    y, ref = _both(x, b, fu, fd, kw)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert _bit_equal(y, ref)


def test_force_call_returns_the_previous_setting():
    from torch_utils import _sg3abi as abi
    lib = abi.load()
    first = lib.sg3_filtered_lrelu_force_up4_wide(1)
    assert lib.sg3_filtered_lrelu_force_up4_wide(0) == 1
    assert lib.sg3_filtered_lrelu_force_up4_wide(first) == 0


@pytest.mark.parametrize('layer', ['L5'])
def test_non_finite_sample(layer):
    """A NaN in plane 0 and an infinity in plane 1: the same NaN footprint and the same finite outputs in both forms."""
    x, b, fu, fd, kw = _inputs(layer, 1, seed=77)
    side = x.shape[-1]
    x[0, 0, side // 2, side // 5] = float('nan')
    x[0, 1, side // 3, side - 2] = float('inf')
    y, ref = _both(x, b, fu, fd, kw)
    assert bool(torch.isnan(ref[0, 0]).any()) and bool(torch.isnan(ref[0, 1]).any()) and bool(torch.isfinite(ref[0, 2:]).all())
    assert _bit_equal(y, ref)


@pytest.mark.parametrize('layer', ['L7', 'L2'])
def test_samples_above_the_fast_activation_threshold(layer):
    """A block of rows at the left of plane 0 and one sample of the last plane far above the threshold: those waves run their chunk
    again with lrelu + clamp (L7: one plane per wave and the two-plane remainder strip; L2: two planes per wave)."""
    x, b, fu, fd, kw = _inputs(layer, 2, seed=78)
    t = _threshold(fu, kw)
    assert t > 0
    h, w = x.shape[-2:]
    assert float((x[1] + b[:, None, None]).abs().max()) < t                   # elsewhere the fast form stands
    x[0, 0, h // 3: h // 3 + 7, : max(4, w // 10)] *= 4.0 * t
    x[-1, -1, h // 2, w // 2] = -3.0 * t
    assert float((x[0, 0] + b[0]).abs().max()) > t and float((x[-1, -1] + b[-1]).abs().max()) > t    # those waves run the redo pass
    y, ref = _both(x, b, fu, fd, kw)
    assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0
    assert _bit_equal(y, ref)


def test_fp16_io_comes_along():
    x, b, fu, fd, kw = _inputs('L4', 1, seed=79, dtype=torch.float16)
    y, ref = _both(x, b, fu, fd, kw)
    assert bool(torch.isfinite(ref.float()).all()) and _bit_equal(y, ref)
