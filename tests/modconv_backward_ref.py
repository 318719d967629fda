"""float64 references of the modulated convolution's backward, and the error model its HIP kernels are held to.

Plain torch, no libsg3hip call: the references run wherever their inputs live (the GPU tests keep them on the device, in
float64, sample by sample).  With the per-sample effective weights w_eff[n,o,i,ky,kx] of the reference formulation
(`modulated_conv._effective_weights`, networks_stylegan3.py:39-56) the forward is out[n] = conv(x[n], w_eff[n], pad), so

    dW_eff[n,o,i,ky,kx] = sum_{y,x} dy[n,o,y,x] * xp[n,i,y+ky,x+kx]                 (xp: x zero-padded by `pad`)
    dx[n,i,y+ky-pad,x+kx-pad] += sum_o dy[n,o,y,x] * w_eff[n,o,i,ky,kx]

one GEMM per sample and tap.  dw, ds follow from dW_eff by the chain rule through `_effective_weights` (autograd in float64).

Error model (what the bound functions below return, element by element:  |got - ref| <= c_rel * abs_scale + c_abs).
u = 2^-24 is the fp32 unit roundoff.

  split:  an fp32 operand a (already multiplied by its power-of-two scale) is held as hi + lo: hi = a with the low 13
          significand bits cleared, lo = fp16(a - hi) rounded toward zero (v_cvt_pkrtz).  |a - hi| < 2^-10 |a|; lo keeps 11 of
          the at most 13 bits of a - hi, so |lo - (a - hi)| < 2^-20 |a|.  The kernels form ah*bh + ah*bl + al*bh (exact fp16
          products): the dropped al*bl is < 2^-20 |ab|, the two rounded lo's add < 2^-20 |ab| each.  Per product: 3 * 2^-20 |ab|.
  floor:  a scaled operand below fp16's normal range (2^-14) sits on the absolute 2^-24 grid; hi and lo are each converted
          once, so |delta a_scaled| < 2^-23 on top of the relative part.  In unscaled units that is 2^-23 / scale, where the
          scale is the power of two that puts the operand's bound just below 2^15 (`pow2_scale` of sg3_wgrad.hip, `prep_s_body`
          of sg3_modconv.hip).  Summed over a dot product: 2^-23 * (sum|b| / scale_a + sum|a| / scale_b).
  accumulation:  fp32, in MFMA steps of 16 products; a product passes through at most 16 roundings inside its MFMA, one per
          later MFMA on the same accumulator (three per 16-element K step), one per workgroup partial added after it.  With n
          such roundings the probabilistic bound of Higham & Mary (SIAM J. Sci. Comput. 41 (2019) A2815) gives
          lambda * sqrt(n) * u * sum|ab|, failing with probability below 2 n exp(-lambda^2 / 2): lambda = 10 makes that < 1e-18
          per element.  (The worst-case n * u is 30 - 100x larger at the 1044^2 layers and would hide a dropped row.)
  prep:   the scale vectors come from fp32 reductions on the device: the pre-normalisation rsqrt(mean w^2) over I k^2 terms,
          computed twice (the forward's prep, and the transposed weights of the data gradient) and the demodulation
          coefficient over I k^2 terms; the style normalisation cancels between s_in and dcoef.  lambda * sqrt(I k^2) * u each
          (half of it after the rsqrt), plus a handful of single roundings (operand x scale, coefficient products, epilogue).
  F(2,3): the transform-domain kernel multiplies (d_a +- d_b) by (g_0 +- g_1 + g_2) / 2; every |d_a| |g_b| with a - b within
          three columns of the output appears with weight <= 2 in sum|m|, so its relative terms apply to twice the sum of
          abs_scale over the seven columns around the output; its operands carry one more fp32 rounding and the input scale is
          one power of two lower (the transform adds two samples).
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24                 # fp32 unit roundoff
LAMBDA = 10.0                  # probabilistic rounding-error bound, see the module docstring
C_SPLIT = 3.0 * 2.0 ** -20     # hi/lo split, per product
FLOOR = 2.0 ** -23             # fp16 subnormal grid (2^-24) for hi and for lo, in scaled units


def _acc(n):
    return LAMBDA * math.sqrt(n) * U


def pow2_scale(amax):
    """The operand scale of the weight-gradient kernel: 2^-ceil(log2(amax / 2^15)) (sg3_wgrad.hip: pow2_scale)."""
    return 2.0 ** -math.ceil(math.log2(max(float(amax), 1e-30) / 32768.0))


# ---------------------------------------------------------------------------------------------------------------- references

def wgrad_ref(x, dy, k, pad):
    """dW_eff [N,O,I,k,k] float64: one [O,P] x [P,I] GEMM per sample and tap."""
    n, ci, h, w = x.shape
    co, oh, ow = dy.shape[1], dy.shape[2], dy.shape[3]
    out = torch.empty([n, co, ci, k, k], dtype=torch.float64, device=x.device)
    for s in range(n):
        xp = F.pad(x[s].to(torch.float64), (pad, pad, pad, pad))
        d = dy[s].to(torch.float64).reshape(co, -1)
        for ky in range(k):
            for kx in range(k):
                out[s, :, :, ky, kx] = d @ xp[:, ky:ky + oh, kx:kx + ow].reshape(ci, -1).T
    return out


def dgrad_ref(dy, w_eff, k, pad, extra_cols=0):
    """dx [N,I,H,W] float64 from the per-sample effective weights: one [I,O] x [O,P] GEMM per sample and tap, scattered into
    the padded plane.  `extra_cols`: also return that many columns beyond each side of the plane (the F(2,3) bound's window)."""
    n, co, oh, ow = dy.shape
    ci = w_eff.shape[2]
    h, w = oh + k - 1 - 2 * pad, ow + k - 1 - 2 * pad
    e = extra_cols
    out = torch.empty([n, ci, h, w + 2 * e], dtype=torch.float64, device=dy.device)
    for s in range(n):
        d = dy[s].to(torch.float64).reshape(co, -1)
        acc = torch.zeros([ci, oh + k - 1, ow + k - 1 + 2 * e], dtype=torch.float64, device=dy.device)
        for ky in range(k):
            for kx in range(k):
                acc[:, ky:ky + oh, e + kx:e + kx + ow] += (w_eff[s, :, :, ky, kx].to(torch.float64).T @ d).reshape(ci, oh, ow)
        out[s] = acc[:, pad:pad + h, pad:pad + w + 2 * e]
    return out


def effective_weights64(w, s, demodulate, input_gain):
    from torch_utils.ops import modulated_conv as mc
    g = None if input_gain is None else input_gain.to(torch.float64)
    return mc._effective_weights(w.to(torch.float64), s.to(torch.float64), demodulate, g, int(s.shape[0]))


def modgrad_ref(dw_eff, w, s, demodulate, input_gain):
    """(dw [O,I,k,k], ds [N,I]) float64: autograd of `_effective_weights` in float64 applied to dW_eff (input_gain constant)."""
    w64 = w.detach().to(torch.float64).requires_grad_(True)
    s64 = s.detach().to(torch.float64).requires_grad_(True)
    with torch.enable_grad():
        we = effective_weights64(w64, s64, demodulate, None if input_gain is None else input_gain.detach())
        dw, ds = torch.autograd.grad(we, [w64, s64], dw_eff.to(torch.float64))
    return dw, ds


# ------------------------------------------------------------------------------------------------------------ abs scales

def abs_scale(x=None, dy=None, w_eff=None, k=3, pad=0, extra_cols=0):
    """sum |a| |b| of every output element: the weight gradient's GEMMs on |x|, |dy| (given x and dy) or the data gradient's on
    |dy|, |w_eff| (given dy and w_eff)."""
    if x is not None:
        return wgrad_ref(x.abs(), dy.abs(), k, pad)
    return dgrad_ref(dy.abs(), w_eff.abs(), k, pad, extra_cols)


def _gain_nI(input_gain, n, ci, dev):
    if input_gain is None:
        return torch.ones([n, ci], dtype=torch.float64, device=dev)
    return input_gain.to(device=dev, dtype=torch.float64).expand(n, ci)


def modgrad_abs(a, w, s, demodulate, input_gain):
    """|J|^T a for the chain rule dW_eff -> (dw, ds) of `_effective_weights`, with every stage's Jacobian taken in absolute value
    (a >= 0, [N,O,I,k,k]).  Bounds |J^T e| for any |e| <= a: what an error of dW_eff, or an fp32 rounding of each term of the
    chain rule, can do to dw and ds.  Returns (A_w [O,I,k,k], A_s [N,I]) float64."""
    w = w.detach().to(torch.float64); s = s.detach().to(torch.float64); a = a.to(torch.float64)
    n, ci = s.shape
    g = _gain_nI(input_gain, n, ci, w.device)[:, None, :, None, None]
    ae = a * g.abs()
    if not demodulate:
        aw = (ae * s.abs()[:, None, :, None, None]).sum(0)
        asn = (ae * w.abs()[None]).sum([1, 3, 4])
        return aw, asn
    m = w[0].numel()
    r = w.square().mean([1, 2, 3], keepdim=True).rsqrt()                      # [O,1,1,1]
    q = s.square().mean().rsqrt()
    wn, sn = w * r, s * q
    c = wn[None] * sn[:, None, :, None, None]
    d = (c.square().sum([2, 3, 4], keepdim=True) + 1e-8).rsqrt()
    ac = d * ae + d ** 3 * c.abs() * (ae * c.abs()).sum([2, 3, 4], keepdim=True)
    awn = (ac * sn.abs()[:, None, :, None, None]).sum(0)
    asn = (ac * wn.abs()[None]).sum([1, 3, 4])
    aw = r * awn + r ** 3 / m * w.abs() * (awn * w.abs()).sum([1, 2, 3], keepdim=True)
    as_ = q * asn + q ** 3 / (n * ci) * s.abs() * (asn * s.abs()).sum()
    return aw, as_


# ------------------------------------------------------------------------------------------------------------------ bounds

def wgrad_terms(oh, ow, k, n_bands, n_seg_groups):
    """Roundings a product passes through in the weight-gradient kernel + the caller's reduction (see the module docstring):
    pixels per workgroup L (a band of rows x a group of 32-column segments), three MFMAs per 16-pixel K step, 16 inside one
    MFMA, one per split partial."""
    band_rows = -(-oh // n_bands)
    n_segs = -(-ow // 32)
    cols = min(-(-n_segs // n_seg_groups) * 32, ow)
    return 3 * (band_rows * cols) // 16 + 16 + n_bands * n_seg_groups


def wgrad_bound(x, dy, k, pad, x_amax, dy_amax, n_terms, scale=None):
    """Element-wise bound on |dW_eff(kernel) - wgrad_ref| (fp32 x and dy as the kernel read them; `x_amax`, `dy_amax`: the
    maxima the kernel derived its power-of-two scales from; `n_terms`: `wgrad_terms`).  `scale`: abs_scale(x, dy) if the caller
    has it already."""
    if scale is None:
        scale = abs_scale(x=x, dy=dy, k=k, pad=pad)
    c_rel = C_SPLIT + _acc(n_terms) + 2 * U
    sx, sd = pow2_scale(x_amax), pow2_scale(dy_amax)
    n, co, oh, ow = dy.shape
    # sum |x| over each tap's window and sum |dy| over each output channel's plane: the floor terms
    sum_dy = dy.to(torch.float64).abs().sum([2, 3])                                             # [N,O]
    xa = F.pad(x.to(torch.float64).abs(), (pad, pad, pad, pad))
    sum_x = torch.stack([xa[:, :, ky:ky + oh, kx:kx + ow].sum([2, 3]) for ky in range(k) for kx in range(k)], -1)
    sum_x = sum_x.reshape(n, 1, -1, k, k)                                                        # [N,1,I,k,k]
    floor = FLOOR * (sum_dy[:, :, None, None, None] / sx + sum_x / sd)
    return c_rel * scale + floor * (1 + 1e-3)


def dgrad_bound(dy, w, s, demodulate, input_gain, k, pad, dy_amax, f23):
    """Element-wise bound on |dx(kernel) - dgrad_ref| for the data gradient as `modulated_conv._data_gradient` runs it: the
    forward kernel on dy * dcoef with the normalised transposed weights, s_in applied in the epilogue.  `f23`: the call takes the
    transform-domain kernel.  Returns (bound, scale) float64 [N,I,H,W]."""
    n, co, oh, ow = dy.shape
    ci = w.shape[1]
    w_eff = effective_weights64(w, s, demodulate, input_gain)
    e = 3 if f23 else 0
    sc = abs_scale(dy=dy, w_eff=w_eff, k=k, pad=pad, extra_cols=e)
    if f23:
        win = F.avg_pool2d(sc.reshape(n * ci, 1, sc.shape[2], sc.shape[3]), (1, 7), stride=1) * 7
        sc_rel = 2 * win.reshape(n, ci, sc.shape[2], -1)
        sc = sc[..., e:-e]
    else:
        sc_rel = sc
    kk = co * k * k
    c_prep = 1.5 * _acc(ci * k * k) + 16 * U if demodulate else 4 * U
    c_rel = C_SPLIT + _acc(3 * kk // 16 + 16 + 4) + c_prep + (8 * U if f23 else 6 * U)
    # floors: the operand dy * dcoef * 2^-e (peak below 2^15, one more halving for F(2,3)) and the packed weights, lifted per
    # block to a peak in [2^14, 2^15) -- an absolute 2^-37 * max |wn| at most
    w64, s64 = w.detach().to(torch.float64), s.detach().to(torch.float64)
    wn = w64 * w64.square().mean([1, 2, 3], keepdim=True).rsqrt() if demodulate else w64
    s_in = _gain_nI(input_gain, n, ci, w.device) * (s64 * s64.square().mean().rsqrt() if demodulate else s64)     # [N,I]
    if demodulate:
        dco = ((wn[None] * (s64 * s64.square().mean().rsqrt())[:, None, :, None, None]).square().sum([2, 3, 4]) + 1e-8).rsqrt()
    else:
        dco = torch.ones([n, co], dtype=torch.float64, device=w.device)
    peak = dco.max(1).values * float(dy_amax)                                                   # [N]
    ex = torch.ceil(torch.log2(peak.clamp_min(1e-300) / 32768.0)) + (1 if f23 else 0)
    op_floor = FLOOR * torch.exp2(ex)                                                           # |delta (dy * dcoef)| per element
    sum_wn = wn.abs().sum([0, 2, 3])                                                            # [I]
    dy_mass = (dy.to(torch.float64).abs().amax([2, 3]) * dco).sum(1) * k * k                    # >= sum_{o,t} |dy * dcoef| anywhere
    floor = s_in.abs() * (op_floor[:, None] * sum_wn[None] + 2.0 ** -37 * float(wn.abs().max()) * (2 if f23 else 1) * dy_mass[:, None])
    floor = floor * (2 if f23 else 1)
    return c_rel * sc_rel + floor[:, :, None, None] * (1 + 1e-3), sc


def modgrad_bound(dw_eff_bound, dw_eff_ref, w, s, demodulate, input_gain):
    """Element-wise bound on |(dw, ds)(kernels) - modgrad_ref(dW_eff exact)|: the dW_eff error pushed through the abs-Jacobian,
    plus the fp32 chain rule of sg3_modulation_backward (reductions over I k^2, O k^2 and N I terms, a few single roundings per
    term) applied to the magnitude of the exact terms."""
    n, co, ci, k, _ = dw_eff_ref.shape
    ew, es = modgrad_abs(dw_eff_bound, w, s, demodulate, input_gain)
    aw, as_ = modgrad_abs(dw_eff_ref.abs(), w, s, demodulate, input_gain)
    c = 2 * _acc(max(ci * k * k, co * k * k, n * ci, n)) + 24 * U
    return ew + c * aw, es + c * as_
