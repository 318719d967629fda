"""CPU: the per-operand error contract of the split-precision (fp16 hi + lo) encoder kernels, on the bit-level model of
tests/split_model.py.  The GPU tests (test_gpu_encoder_numerics.py) take their bounds from the constants checked here."""
import numpy as np
import pytest

import split_model as M


def _logu(r, lo, hi, n):
    return (np.exp2(r.uniform(lo, hi, n)) * r.choice([-1.0, 1.0], n)).astype(np.float32)


def test_rtz_conversion_matches_definition():
    v = np.array([1.0, 1 + 2 ** -11, 1 + 3 * 2 ** -11, -(1 + 3 * 2 ** -11), 7e4, -7e4, 2 ** -25, 2 ** -24 * 1.5, np.inf, 65504.0],
                 np.float32)
    got = M.f16_rtz(v).astype(np.float64)
    want = [1.0, 1.0, 1 + 2 ** -10, -(1 + 2 ** -10), 65504.0, -65504.0, 0.0, 2 ** -24, np.inf, 65504.0]
    assert got.tolist() == want
    assert np.isnan(M.f16_rtz(np.float32(np.nan)))


def test_split2_halves():
    x = np.array([1 + 2 ** -10 + 2 ** -11 + 2 ** -22 + 2 ** -23, 3.0, -0.1], np.float32)
    hi, lo = M.split2(x)
    assert hi[0] == np.float16(1 + 2 ** -10) and lo[0] == np.float16(2 ** -11)     # the two lowest bits of lo are cut off
    assert hi[1] == 3 and lo[1] == 0
    assert np.all(np.abs(hi.astype(np.float64)) <= np.abs(x.astype(np.float64)))   # truncation: never rounds up


def test_activation_contract():
    r = np.random.RandomState(0)
    x = _logu(r, -40, 15.98, 1 << 21)
    err = np.abs(M.activations_effective(x) - x.astype(np.float64))
    big = np.abs(x) >= 2 ** -3
    assert np.all(err[big] <= M.ACT_REL * np.abs(x[big]))                             # relative 2^-21 for |x| >= 2^-3
    assert np.all(err <= M.act_error_bound(x))                                        # + ~2^-23 absolute below
    # both constants are needed: the bounds are reached within a factor of two
    assert np.max(err[big] / np.abs(x[big])) > M.ACT_REL / 2
    assert np.max(err[~big]) > M.ACT_ABS / 4
    assert np.max(err[~big] / np.abs(x[~big]).astype(np.float64)) > 2 ** -10       # small activations: no relative bound at all


def test_pow2_lift():
    peaks = np.array([0.0, 1.0, 2 ** 14 - 1, 2 ** 14, 3e4, 7e4, np.inf, np.nan, 1e-30, 1e-45, 0.015], np.float32)
    s = M.pow2_lift(peaks)
    assert s.tolist()[:1] == [1.0] and s[3:8].tolist() == [1.0] * 5                   # scale up only; zero / inf / NaN untouched
    lifted = peaks[[1, 2, 8, 10]] * s[[1, 2, 8, 10]]
    assert np.all((lifted >= M.LIFT_LO) & (lifted < M.LIFT_HI))
    assert np.all(np.log2(s) == np.round(np.log2(s))) and s.max() <= 2.0 ** 126        # exact powers of two with exact inverses
    assert s[9] == 2.0 ** 126                                                          # a subnormal peak: the largest lift


@pytest.mark.parametrize('bn', [1.0, 0.05, 'sweep'])
def test_conv_weight_contract_after_lift(bn):
    """Realistic folded weights (fan-in 4608, folded BatchNorm scales from 2^-12 to 2^4): relative 2^-22 within 2^-17 of the
    channel maximum and 2^-25 lifted units below it.  Without the lift (the pack before the fix) the same weights lose up to all
    of their bits."""
    r = np.random.RandomState(1)
    o = 64
    w = (r.randn(o, 512, 3, 3) / np.sqrt(4608)).astype(np.float32)
    w[:, :, 0, 0] *= np.float32(2 ** -20)                                             # some weights far below the window
    sc = np.exp2(r.uniform(-12, 4, o)).astype(np.float32) if bn == 'sweep' else np.full(o, bn, np.float32)
    v = (w * sc[:, None, None, None]).astype(np.float64)
    hi, lo, ws = M.conv_pack(w, sc)
    lifted_max = np.abs(M.joined(hi, lo)).reshape(o, -1).max(1)
    assert np.all((lifted_max >= M.LIFT_LO) & (lifted_max <= M.LIFT_HI))
    err = np.abs(M.conv_weights_effective(w, sc) - v)
    mx = np.abs(v).reshape(o, -1).max(1)[:, None, None, None]
    win = np.abs(v) >= mx * M.WEIGHT_WINDOW
    assert (~win).any()
    assert np.all(err[win] <= M.CONV_W_REL * np.abs(v[win]))
    assert np.all(err <= M.CONV_W_REL * np.abs(v) + M.CONV_W_ABS_LIFTED * ws.astype(np.float64)[:, None, None, None])
    old = np.abs(M.conv_weights_effective(w, sc, lift=False) - v)
    assert np.max(old[win] / np.abs(v[win])) > 2 ** 8 * M.CONV_W_REL


def test_head_weight_contract_after_lift():
    r = np.random.RandomState(2)
    w = (r.randn(3, 512, 96) / np.sqrt(512) * np.exp2(r.uniform(-12, 4, (1, 1, 96)))).astype(np.float32)
    err = np.abs(M.head_weights_effective(w) - w.astype(np.float64))
    _, _, cs = M.head_pack(w)
    mx = np.abs(w).max(axis=1, keepdims=True).astype(np.float64)
    win = np.abs(w) >= mx * M.WEIGHT_WINDOW
    assert np.all(err[win] <= M.HEAD_W_REL * np.abs(w[win]))
    assert np.all(err <= M.HEAD_W_REL * np.abs(w) + M.HEAD_W_ABS_LIFTED * cs.astype(np.float64)[:, None, :])
    old = np.abs(M.head_weights_effective(w, lift=False) - w.astype(np.float64))
    assert np.max(old[win] / np.abs(w[win]).astype(np.float64)) > 2 ** 8 * M.HEAD_W_REL


def test_product_contract():
    """One split product ah*bh + ah*bl + al*bh (al*bl dropped) of operands in their relative regime."""
    r = np.random.RandomState(3)
    a, b = _logu(r, -3, 15.9, 1 << 20), _logu(r, -3, 15.9, 1 << 20)
    exact = np.abs(a.astype(np.float64) * b)
    ah, al = M.split2(a)
    bh, bl = M.pack_round(b)
    rel = np.abs(M.product(ah, al, bh, bl) - a.astype(np.float64) * b) / exact
    assert rel.max() <= M.PROD_REL_CONV and rel.max() > M.PROD_REL_CONV / 2
    bh, bl = M.split2(b)
    rel = np.abs(M.product(ah, al, bh, bl) - a.astype(np.float64) * b) / exact
    assert rel.max() <= M.PROD_REL_HEAD and rel.max() > M.PROD_REL_HEAD / 2


def test_gemm_error_of_the_issue_table():
    """K = 4608 dot products of realistic operands (64 x 256 outputs), fp64 sums of the split operands: with a folded BatchNorm
    scale of 0.05 the unlifted pack is off by ~2e-5 of max|ref|; the lifted one stays at the operand contract."""
    r = np.random.RandomState(4)
    w = (r.randn(64, 4608) / np.sqrt(4608)).astype(np.float32)
    x = r.randn(4608, 256).astype(np.float32)
    sc = np.full(64, 0.05, np.float32)
    ref = (w.astype(np.float64) * 0.05) @ x.astype(np.float64)
    xe = M.activations_effective(x)
    new = M.conv_weights_effective(w, sc) @ xe
    old = M.conv_weights_effective(w, sc, lift=False) @ xe
    scale = np.abs(ref).max()
    assert np.abs(old - ref).max() / scale > 1e-5
    assert np.abs(new - ref).max() / scale < 1e-6
