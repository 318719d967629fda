"""Bit-level numpy model of the fp16 hi + lo operand splits of the encoder's split-precision kernels (csrc/sg3_split.h,
csrc/sg3_conv2d.hip, csrc/sg3_head_gemm.hip), and the per-operand error contract they give.  The GPU tests take their bounds
from the constants here; tests/test_split_numerics_cpu.py checks the constants against the model.

  split2       (activations of both kernels, head-GEMM weights): hi = fp16_rtz(x with its low 13 significand bits cleared),
               lo = fp16_rtz(x - that truncated value) -- the subtraction uses the fp32 truncation, not the converted hi;
  pack_round   (conv2d weights): hi = fp16_rne(v), lo = fp16_rne(v - hi);
  pow2_lift    the power of two both packs multiply a weight channel / column by first (max |w| into [2^14, 2^15), scale up only).

A product of two split operands is ah*bh + ah*bl + al*bh (al*bl is dropped), each term exact in fp32.
"""
import numpy as np

# per-operand contract: |x - (hi + lo)| <= REL * |x| + ABS
ACT_REL = 2.0 ** -21          # split2: 13 bits of lo rounded toward zero to 11
ACT_ABS = 2.0 ** -23          # split2 below |x| = 2^-3: lo on fp16's 2^-24 grid, and a hi below 2^-14 loses what lo cannot recover
CONV_W_REL = 2.0 ** -22       # pack_round, for weights within 2^-17 of their (lifted) channel maximum
CONV_W_ABS_LIFTED = 2.0 ** -25  # pack_round below that, in lifted units (multiply by the channel's inverse lift, wScale)
HEAD_W_REL = ACT_REL          # split2 on lifted weights
HEAD_W_ABS_LIFTED = ACT_ABS
# relative error of one product ah*bh + ah*bl + al*bh of two operands inside their relative regime (al*bl dropped)
PROD_REL_CONV = 2.0 ** -20    # split2 activation x pack_round weight
PROD_REL_HEAD = 2.0 ** -19    # split2 x split2
LIFT_LO, LIFT_HI = 2.0 ** 14, 2.0 ** 15
WEIGHT_WINDOW = 2.0 ** -17    # weights this far below their channel's maximum keep the relative bound
FP16_GUARD = 65000.0          # the kernels' range flag threshold on |operand|


def f16_rtz(v):
    """fp32 -> fp16 rounding toward zero (v_cvt_pkrtz_f16_f32): overflow saturates to +-65504, NaN / inf pass."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        r = v.astype(np.float16)
        away = np.isfinite(v) & (np.abs(r.astype(np.float64)) > np.abs(v.astype(np.float64)))
        r = np.where(away, np.nextafter(r, np.float16(0)), r)
    return r.astype(np.float16)


def split2(x):
    x = np.asarray(x, dtype=np.float32)
    h = (x.view(np.uint32) & np.uint32(0xffffe000)).view(np.float32)
    with np.errstate(invalid='ignore'):
        return f16_rtz(h), f16_rtz(x - h)


def pack_round(v):
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over='ignore', invalid='ignore'):
        h = v.astype(np.float16)
        return h, (v - h.astype(np.float32)).astype(np.float16)


def pow2_lift(peak):
    """Elementwise 2^e, e = min(15 - exponent, 126) for 0 < peak < 2^14, else 1 (pow2_lift in csrc/sg3_split.h)."""
    peak = np.asarray(peak, dtype=np.float32)
    _, ex = np.frexp(peak)
    ok = (peak > 0) & (peak < LIFT_LO)
    return np.where(ok, np.ldexp(np.float32(1), np.minimum(15 - ex, 126)), np.float32(1)).astype(np.float32)


def joined(hi, lo):
    return hi.astype(np.float64) + lo.astype(np.float64)


def conv_pack(w, out_scale=None, lift=True):
    """Folded [O, ...] fp32 weights -> (hi, lo, wScale) of conv2d_pack_f16x3_kernel; hi / lo in lifted units."""
    w = np.asarray(w, dtype=np.float32)
    sc = np.ones(w.shape[0], np.float32) if out_scale is None else np.asarray(out_scale, np.float32)
    v = (w * sc.reshape((-1,) + (1,) * (w.ndim - 1))).astype(np.float32)
    s = pow2_lift(np.abs(v).reshape(v.shape[0], -1).max(axis=1)) if lift else np.ones(v.shape[0], np.float32)
    hi, lo = pack_round(v * s.reshape((-1,) + (1,) * (w.ndim - 1)))
    return hi, lo, (1.0 / s).astype(np.float32)


def conv_weights_effective(w, out_scale=None, lift=True):
    """The folded weights as the split kernel multiplies them (float64): (hi + lo) * wScale."""
    hi, lo, ws = conv_pack(w, out_scale, lift)
    return joined(hi, lo) * ws.astype(np.float64).reshape((-1,) + (1,) * (hi.ndim - 1))


def head_pack(w, lift=True):
    """[G, K, N] weights -> (hi, lo, colScale [G, N]) of head_gemm_colscale_kernel + head_gemm_pack_kernel."""
    w = np.asarray(w, dtype=np.float32)
    s = pow2_lift(np.abs(w).max(axis=1)) if lift else np.ones((w.shape[0], w.shape[2]), np.float32)
    hi, lo = split2(w * s[:, None, :])
    return hi, lo, (1.0 / s).astype(np.float32)


def head_weights_effective(w, lift=True):
    hi, lo, cs = head_pack(w, lift)
    return joined(hi, lo) * cs.astype(np.float64)[:, None, :]


def activations_effective(x):
    hi, lo = split2(x)
    return joined(hi, lo)


def product(a_hi, a_lo, b_hi, b_lo):
    """ah*bh + ah*bl + al*bh in float64 (each fp16 x fp16 product is exact in fp32)."""
    A = lambda t: t.astype(np.float64)  # noqa: E731
    return A(a_hi) * A(b_hi) + A(a_hi) * A(b_lo) + A(a_lo) * A(b_hi)


def act_error_bound(x):
    """Per-activation contract |x - split(x)| <= ACT_REL |x| + ACT_ABS."""
    return ACT_REL * np.abs(np.asarray(x, np.float64)) + ACT_ABS
