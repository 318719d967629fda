"""CPU: the threshold under which the plain forward of the streaming filtered_lrelu kernel evaluates lrelu + clamp as one
med3(u, slope*u, clamp/gain) is conservative.  The library computes it with the same code on the host as each wave does on the
device (sg3_filtered_lrelu_fast_threshold); here it is checked against the exact bound in float64 and against a float32 worst
case of the kernel's own up-filter arithmetic."""
import ctypes

import numpy as np
import pytest


def _lib():
    import torch  # noqa: F401  (loads torch's HIP runtime before ours)
    from torch_utils import _sg3abi
    return _sg3abi.load()


def _threshold(fu, up, gain, slope, clamp):
    fu = np.ascontiguousarray(fu, dtype=np.float32)
    return float(_lib().sg3_filtered_lrelu_fast_threshold(fu.ctypes.data_as(ctypes.c_void_p), fu.size, up, gain, slope, clamp))


def _phase_bound(fu, up):
    """up * max over phases of sum |taps|: the gain of one direction of the up filter as the kernel applies it (float64)."""
    f = np.abs(fu.astype(np.float64))
    return up * max(f[p::up].sum() for p in range(up))


def _clampv(gain, clamp):
    return float(np.float32(clamp) / np.float32(gain))         # the kernel's clamp / gain, in float32


@pytest.mark.parametrize('up,taps', [(2, 12), (4, 24)])
def test_fast_threshold_is_conservative_for_random_filters(up, taps):
    rng = np.random.RandomState(7 + up)
    for _ in range(400):
        fu = (rng.randn(taps) * rng.choice([1e-3, 0.1, 1.0, 30.0])).astype(np.float32)
        gain = float(np.float32(rng.choice([1.0, np.sqrt(2), rng.uniform(0.05, 20.0)])))
        slope = float(np.float32(rng.choice([0.0, 0.2, 1.0, rng.uniform(0.0, 1.0)])))
        clamp = float(np.float32(rng.choice([256.0, 4.0, np.inf, rng.uniform(1e-3, 1e3)])))
        t = _threshold(fu, up, gain, slope, clamp)
        hv = _phase_bound(fu, up) ** 2
        assert 0.0 < t < np.inf                                # an infinity in the input always fails |x| <= T
        assert t * hv <= 2.0 ** 124                            # |u| stays far below overflow
        if np.isfinite(clamp) and slope > 0:
            assert t * hv * slope <= _clampv(gain, clamp)


def test_fast_threshold_is_tight_enough_for_stylegan3():
    """At the synthesis layers' settings (clamp 256, gain sqrt 2, slope 0.2) and their low-pass up filters the threshold leaves
    typical activations on the fast path: within 1e-3 of the exact bound clamp / (gain slope hv)."""
    from oracle import oracle as O
    for up, taps in ((2, 12), (4, 24)):
        fu = O.design_lowpass_filter(taps, 4.0, 8.0, 64.0 * up / 2).astype(np.float32)
        t = _threshold(fu, up, float(np.float32(np.sqrt(2))), 0.2, 256.0)
        exact = _clampv(np.float32(np.sqrt(2)), 256.0) / (0.2 * _phase_bound(fu, up) ** 2)
        assert exact * (1 - 1e-3) <= t <= exact


def test_fast_threshold_none_without_a_positive_clamp():
    fu = np.full(12, 0.1, np.float32)
    assert _threshold(fu, 2, 1.0, 0.2, 0.0) == -1.0
    assert _threshold(fu, 2, -1.0, 0.2, 256.0) == -1.0


@pytest.mark.parametrize('up,taps', [(2, 12), (4, 24)])
def test_fast_threshold_holds_in_the_kernels_float32_arithmetic(up, taps):
    """Worst case of the kernel's fp32 FMA chains: every staged sample at +-T with the sign of its tap, both directions --
    slope * |u| stays within clamp / gain (the condition under which med3(u, slope u, c) equals med3(max(u, slope u), -c, c))."""
    rng = np.random.RandomState(3 + up)
    for _ in range(200):
        fu = rng.randn(taps).astype(np.float32)
        gain, slope, clamp = np.float32(np.sqrt(2)), np.float32(rng.uniform(0.01, 1.0)), np.float32(rng.uniform(0.1, 300.0))
        t = np.float32(_threshold(fu, up, float(gain), float(slope), float(clamp)))
        g = (fu * np.float32(up)).astype(np.float32)
        for p in range(up):
            taps_p = g[p::up]
            w = np.float32(0)
            for tap in taps_p:                                 # H-up: |w| at its largest
                w = np.float32(np.float32(np.abs(tap)) * t + w)
            wmax = max(np.float32(0), w)
            for q in range(up):
                u = np.float32(0)
                for tap in g[q::up]:                           # V-up over rows that all hold wmax
                    u = np.float32(np.float32(np.abs(tap)) * wmax + u)
                assert np.float32(u * slope) <= clamp / gain
