"""GPU: the plain forward of the streaming filtered_lrelu kernel runs a row chunk with the one-instruction activation
med3(u, slope*u, clamp/gain) while every staged sample stays within the threshold, and runs the chunk again with lrelu + clamp
(and the NaN guard) where one does not.  Its outputs must be bit-for-bit those of the second form alone, which
SG3_FLRELU_SLOWACT=1 forces: at the T-1024 and R-1024 layer geometries, on typical inputs, on inputs that trip some strips only,
at the special activation settings, and with NaN / infinity in the input."""
import contextlib
import os

import numpy as np
import pytest
import torch

from golden_cases import rand

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (shape, up, taps, padding, radial): output sizes of the synthesis layers
GEOMETRIES = [
    ((2, 6, 38, 38), 2, 12, [9, 8, 9, 8], False),              # T L0 / L1: 36 columns, two planes per wave
    ((2, 4, 38, 38), 4, 24, [-6, -9, -6, -9], False),          # T L2: up 4, 52 columns, two planes per wave
    ((1, 4, 150, 150), 2, 12, [9, 8, 9, 8], False),            # T L6: 148 = 120 + 28, full strip + packed remainder
    ((1, 4, 86, 86), 4, 24, [-6, -9, -6, -9], False),          # T L5: up 4, 148 columns
    ((1, 2, 1046, 1046), 2, 12, [9, 8, 9, 8], False),          # T L10-L13: 1044 columns, nine strips
    ((2, 4, 36, 36), 2, 12, [11, 10, 11, 10], True),           # R: radial down filter, two planes per wave
    ((1, 2, 148, 148), 2, 12, [11, 10, 11, 10], True),         # R: radial, up 2, 148 columns (two launches)
    ((1, 3, 84, 84), 4, 24, [-2, -5, -2, -5], True),           # R: radial, up 4, 148 columns (one launch), odd plane count
]
GEOMETRY_IDS = ['T36', 'T52up4', 'T148', 'T148up4', 'T1044', 'R36', 'R148', 'R148up4']


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@contextlib.contextmanager
def _slow_activation():
    old = os.environ.get('SG3_FLRELU_SLOWACT')
    os.environ['SG3_FLRELU_SLOWACT'] = '1'
    try:
        yield
    finally:
        if old is None:
            del os.environ['SG3_FLRELU_SLOWACT']
        else:
            os.environ['SG3_FLRELU_SLOWACT'] = old


def _filters(up, taps, radial, mirror=True):
    from oracle import oracle as O
    fu = O.design_lowpass_filter(taps, 4.0, 8.0, 64.0 * up / 2).astype(np.float32)
    fd = O.design_lowpass_filter(12, 5.0, 9.0, 64.0, radial=radial).astype(np.float32)
    if radial and not mirror:
        fd = (fd + 0.01 * np.random.RandomState(8).rand(12, 12)).astype(np.float32)
    return fu, fd


def _threshold(fu, up, gain, slope, clamp):
    import ctypes
    from torch_utils import _sg3abi
    return float(_sg3abi.load().sg3_filtered_lrelu_fast_threshold(fu.ctypes.data_as(ctypes.c_void_p), fu.size, up, gain, slope,
                                                                   float('inf') if clamp is None else clamp))


def _both(x, b, fu, fd, up, pad, slope=0.2, clamp=256.0, dtype=None):
    """(default, forced-slow) outputs as numpy arrays."""
    from torch_utils.ops import filtered_lrelu as fl
    kw = dict(up=up, down=2, padding=pad, gain=float(np.sqrt(2)), slope=slope, clamp=clamp, flip_filter=False)
    xt, bt, fut, fdt = T(x, dtype), T(b, dtype), T(fu), T(fd)
    fast = fl.filtered_lrelu(xt, fut, fdt, bt, **kw)
    with _slow_activation():
        slow = fl.filtered_lrelu(xt, fut, fdt, bt, **kw)
    return fast.cpu().numpy(), slow.cpu().numpy()


def _bit_equal(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype
    ints = np.uint32 if a.dtype == np.float32 else np.uint16
    return np.array_equal(a.view(ints), b.view(ints))


@pytest.mark.parametrize('shape,up,taps,pad,radial', GEOMETRIES, ids=GEOMETRY_IDS)
@pytest.mark.parametrize('clamp,slope', [(256.0, 0.2), (4.0, 0.2), (None, 0.2), (256.0, 0.0), (8.0, 1.0)],
                         ids=['typical', 'clamp4', 'noclamp', 'slope0', 'slope1'])
def test_fast_activation_is_bit_identical(shape, up, taps, pad, radial, clamp, slope):
    fu, fd = _filters(up, taps, radial)
    x = rand(3, *shape); b = rand(4, shape[1])
    y, ref = _both(x, b, fu, fd, up, pad, slope, clamp)
    assert np.isfinite(ref).all() and _bit_equal(y, ref)
    if (clamp, slope) == (256.0, 0.2):
        # typical activations: every staged sample is under the threshold, so the fast form is what produced y
        assert float(np.abs(x + b[None, :, None, None]).max()) < _threshold(fu, up, float(np.sqrt(2)), slope, clamp)


@pytest.mark.parametrize('shape,up,taps,pad,radial', GEOMETRIES, ids=GEOMETRY_IDS)
def test_fast_activation_redo_where_the_threshold_trips(shape, up, taps, pad, radial):
    """A block of rows in the first columns of plane 0 (strip 0 of one row chunk) and one sample of the last plane far above the
    threshold: those waves run their chunk again, everything is bit-for-bit the forced-slow output -- on both sides of the
    clamp, since the scaled samples drive the activation far beyond +-clamp."""
    fu, fd = _filters(up, taps, radial, mirror=False)
    x = rand(5, *shape); b = rand(6, shape[1])
    h, w = shape[2], shape[3]
    t = _threshold(fu, up, float(np.sqrt(2)), 0.2, 256.0)
    x[0, 0, h // 3: h // 3 + 7, : max(4, w // 10)] *= 4.0 * t
    x[-1, -1, h // 2, w // 2] = -3.0 * t
    y, ref = _both(x, b, fu, fd, up, pad)
    assert np.isfinite(ref).all() and _bit_equal(y, ref)
    assert float(np.abs(ref).max()) > 0


@pytest.mark.parametrize('shape,up,taps,pad,radial', GEOMETRIES, ids=GEOMETRY_IDS)
def test_fast_activation_non_finite_input(shape, up, taps, pad, radial):
    """NaN in one strip of plane 0, an infinity in plane 1 (the second plane of a two-plane wave where the planes pack): the NaN
    footprint of the NaN guard and every finite output, bit for bit."""
    fu, fd = _filters(up, taps, radial)
    x = rand(7, *shape); b = rand(8, shape[1])
    h, w = shape[2], shape[3]
    x[0, 0, h // 2, w // 5] = np.nan
    x[0, 1, h // 3, w - 2] = np.inf
    y, ref = _both(x, b, fu, fd, up, pad)
    assert np.isnan(ref[0, 0]).any() and np.isnan(ref[0, 1]).any()
    assert _bit_equal(y, ref)


@pytest.mark.parametrize('shape,up,taps,pad,radial', [GEOMETRIES[2], GEOMETRIES[5]], ids=['T148', 'R36'])
def test_fast_activation_fp16_io(shape, up, taps, pad, radial):
    fu, fd = _filters(up, taps, radial)
    x = rand(9, *shape); b = rand(10, shape[1])
    x[0, 0, 5: 9, :6] *= 3e3                                   # trips strip 0 of plane 0 (fp16 still holds it)
    y, ref = _both(x, b, fu, fd, up, pad, dtype=torch.float16)
    assert _bit_equal(y, ref)
