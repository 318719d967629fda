"""float64 reference of filtered_lrelu (forward and adjoint), a decoder of its sign tensor, and the error model its HIP kernels
are held to.

Plain torch, no libsg3hip call, and no float64 convolution: every FIR pass is a pair of banded (Toeplitz) matrices and two matmuls,
a 2-D filter is one such pair per filter row (a row selection times that row's taps), summed.  The references run wherever their
inputs live.  With x' = x + b, A the up pass (zero insertion, padding, correlation taps g[k] = f[k] with flip, f[n-1-k] without,
times `up` per axis), B the down pass (taps, keep every `down`-th sample) and act(u) = clamp(lrelu(gain * u)):

    u = A x'                y = B act(u)
    g_up = B^T dy           dx = A^T (m(u) * gain * g_up),   m(u) in {1, slope, 0}  (u >= 0 | u < 0 | clamped)        db = sum dx

Operands are the fp32 values that cross the ABI, converted to float64: taps, gain, slope, clamp.  `up` is a power of two in every
kernel form, so up^2 is exact wherever it is folded (the kernels scale the separable up taps by `up` per axis; the 12x12 up filter
of an adjoint call keeps raw taps and multiplies the output gain by up^2).  The adjoint call's gain is the fp32 rounding of
gain * up^2 / down^2 (filtered_lrelu._adjoint); `adjoint_ref` uses that value times down^2 / up^2.

Error model:  |got - ref| <= n * u * abs_scale  element by element, u = 2^-24, times (1 + 2^-16) for the second-order terms
(n <= 120).  The kernels are plain fp32 FMA chains, no split precision: a product passes through one rounding per FMA of its chain.
abs_scale is the same pipeline on |x + b| (or |dy|) with |taps|.  Counted from csrc/sg3_filtered_lrelu.hip (`Stream::step`),
with tu = taps per phase of the up filter (6), td = taps of the down filter (12 | 24):

    bias add                      1    fmaf(bias, rowFlag, load); the adjoint has no bias (0: exact)
    H-up                          tu   one multiply + tu - 1 FMAs                       } 12x12 up filter (adjoint of the radial
    V-up                          tu   one multiply + tu - 1 FMAs                       } layers): one chain of tu^2 = 36 FMAs
    activation                    1    forward: * slope before the clamp (max and med3 select exactly; the sign-writing form
                                       decides its codes from fp32(gain * u) besides, and stores the same values).
                                       Adjoint: 1 (the multiplier)
    V-down, separable             td   scatter into the output rows in flight, one FMA per tap
    H-down, separable             td/2 + 1   packed FMAs over tap pairs, then the two halves added
    12x12 down filter             td^2/2 + 1 = 73   each half of the packed accumulator takes 6 FMAs per upsampled row, 12 rows,
                                       then the halves are added;  mirror-symmetric rows: 1 (the fold's add) + td^2/4 + 1 = 38
    output gain                   1    once per output sample, after the down pass

  forward, separable: u 13, y 13 + 1 + 12 + 7 + 1 = 34;  12x12 down: 13 + 1 + 73 + 1 = 88, folded 53;
  adjoint (up 2), down 2: 12 + 1 + 12 + 7 + 1 = 33, down 4: 12 + 1 + 24 + 13 + 1 = 51;  12x12 up: 36 + 1 + ... = 57 | 75.
  The forward's activation is Lipschitz (constant gain), so the roundings before it count against gain * |B| |A| |x'|, and those
  after it against |B| min(gain |A| |x'|, clamp): what the down pass really sums.  A dropped outer tap is 1e-3 .. 1e-2 of
  abs_scale, hundreds of times the bound.
  Configurations without a fused kernel (ToRGB's 1x1 filters in training, 2-D up filters in a forward) run the generic composition
  of the same steps; the same counts are applied with their tap numbers.

  With `generic=True` the bounds count the composition as it runs (x + b -> upfirdn2d -> filtered_lrelu_act_ -> upfirdn2d, each a
  kernel of its own; every float64 call, every double backward and every configuration without a fused kernel):
    bias add 1;  up pass T_u + 2 (T_u taps that can meet a real sample: ceil(n / up) per axis of a separable filter, added; the
    product of the sides of a 2-D one; + 2: the gain product and the stored result);  activation 1;  down pass T_d + 2 (every tap).
    The adjoint is the same composition with (up, fu) <-> (down, fd) and no bias.  fp16 tensors store every intermediate: x + b,
    each pass of each upfirdn2d call (two for a separable filter) and the activation, one 2^-11 each.  `unit`: 2^-53 for float64.

  fp16 I/O: the inputs are what the kernel read (already rounded); the stored output adds 2^-11 (|ref| + bound), or 2^-25 on
  fp16's subnormal grid (|ref| below 2^-14).

  adjoint, discontinuity: m(u) jumps at u = 0 (by 1 - slope) and at |lrelu(gain u)| = clamp (by slope | 1).  A sample is
  ambiguous when |u64| <= bound(u) (and u is not identically zero: abs_scale 0 means the kernel's u is 0 too), or when
  |lrelu(gain u64)| is within the bound on that quantity (bound(u) * gain + 2 u |gain u|, times slope for u < 0) of clamp.
  No element is excluded: the bound of dx is widened by |A|^T (ambiguous * jump * gain * |g_up|), and the share of dx elements
  with a nonzero widening is computed from the float64 reference alone (the tests cap it at 1e-3 per layer).
  Sign codes (2 bits per upsampled sample, 1 = negative, 2 = clamped) must equal the float64 decision at every non-ambiguous
  sample of the active width.

  db: the kernel sums its fp32 dx before they are stored: per lane over the chunk's rows (CH adds, + 1 for the column pair), 6
  butterfly adds, then slots * N adds in flrelu_finish_partials_kernel:  sum(bound dx) + (CH + 7 + slots * N) * u * sum |dx|.
  Without the fused adjoint (ToRGB) db is torch's dx.sum: any summation order stays within (count - 1) * u * sum |dx|.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24                    # fp32 unit roundoff
SECOND = 1.0 + 2.0 ** -16         # n u / (1 - n u) <= n u (1 + 2^-16) for n <= 256
F16_REL = 2.0 ** -11
F16_SUB = 2.0 ** -25              # half a step of fp16's subnormal grid


def f32(v):
    """The float64 value of v rounded to fp32: what crosses the ABI."""
    return float(np.float32(v))


def _four(padding):
    if isinstance(padding, int):
        return padding, padding, padding, padding
    p = [int(v) for v in padding]
    if len(p) == 2:
        return p[0], p[0], p[1], p[1]
    return tuple(p)


def _filt(f, dev):
    """None -> one tap of 1;  otherwise the fp32 taps as float64 (1-D or 2-D)."""
    if f is None:
        return torch.ones([1], dtype=torch.float64, device=dev)
    f = torch.as_tensor(f)
    assert f.dtype == torch.float32 and f.ndim in (1, 2)
    if f.ndim == 2 and f.shape[0] == 1:
        f = f[0]
    return f.to(device=dev, dtype=torch.float64)


def _corr(f, flip):
    """correlation taps: g[k] = f[k] with flip, f[n-1-k] without (both axes of a 2-D filter)."""
    return f if flip else f.flip(list(range(f.ndim)))


def up_matrix(length, g, up, p0, p1):
    """[M, length] float64: zero insertion by `up`, padding (p0, p1; negative crops), correlation with g, times `up`.
    M = length * up + p0 + p1 - (n - 1);  out[m] = sum_k g[k] * z[m + k - p0], z[i * up] = in[i]."""
    n = int(g.shape[0])
    m_out = length * up + p0 + p1 - (n - 1)
    assert m_out > 0
    m = torch.arange(m_out, device=g.device)[:, None]
    i = torch.arange(length, device=g.device)[None, :]
    k = i * up + p0 - m
    ok = (k >= 0) & (k < n)
    return torch.where(ok, g[k.clamp(0, n - 1)], torch.zeros([], dtype=g.dtype, device=g.device)) * up


def down_matrix(length, g, down):
    """[O, length] float64: correlation with g, every `down`-th sample.  O = (length - (n - 1) + down - 1) // down."""
    n = int(g.shape[0])
    o_out = (length - (n - 1) + down - 1) // down
    assert o_out > 0
    o = torch.arange(o_out, device=g.device)[:, None]
    m = torch.arange(length, device=g.device)[None, :]
    k = m - o * down
    ok = (k >= 0) & (k < n)
    return torch.where(ok, g[k.clamp(0, n - 1)], torch.zeros([], dtype=g.dtype, device=g.device))


def _onehot(n, k, dev):
    e = torch.zeros([n], dtype=torch.float64, device=dev)
    e[k] = 1.0
    return e


class Ops:
    """The two linear passes of one call as lists of (V, H) matrix pairs: pass(X) = sum V @ X @ H^T."""

    def __init__(self, xh, xw, fu, fd, up, down, padding, flip, dev):
        px0, px1, py0, py1 = _four(padding)
        gu, gd = _corr(_filt(fu, dev), flip), _corr(_filt(fd, dev), flip)
        self.up, self.down = int(up), int(down)
        self.fu_shape, self.fd_shape = tuple(gu.shape), tuple(gd.shape)
        if gu.ndim == 1:
            self.A = [(up_matrix(xh, gu, up, py0, py1), up_matrix(xw, gu, up, px0, px1))]
        else:
            nh = int(gu.shape[0])
            self.A = [(up_matrix(xh, _onehot(nh, k, dev), up, py0, py1), up_matrix(xw, gu[k], up, px0, px1)) for k in range(nh)]
        mh, mw = int(self.A[0][0].shape[0]), int(self.A[0][1].shape[0])
        if gd.ndim == 1:
            self.B = [(down_matrix(mh, gd, down), down_matrix(mw, gd, down))]
        else:
            nh = int(gd.shape[0])
            self.B = [(down_matrix(mh, _onehot(nh, k, dev), down), down_matrix(mw, gd[k], down)) for k in range(nh)]
        self.u_hw = (mh, mw)
        self.y_hw = (int(self.B[0][0].shape[0]), int(self.B[0][1].shape[0]))
        # mirror-symmetric rows of a 2-D down filter: the kernel folds them (fdMirror of the binding)
        self.fd_mirror = gd.ndim == 2 and bool(torch.equal(gd, gd.flip([1])))

    @staticmethod
    def apply(pairs, x, absolute=False, transpose=False):
        out = None
        for v, h in pairs:
            if absolute:
                v, h = v.abs(), h.abs()
            t = (v.T @ x @ h) if transpose else (v @ x @ h.T)
            out = t if out is None else out + t
        return out

    # ---- rounding counts (module docstring)
    def n_u(self, bias=True):
        tu = [-(-s // self.up) for s in self.fu_shape]
        return (1 if bias else 0) + (tu[0] * tu[1] if len(tu) == 2 else 2 * tu[0])

    # ---- the generic composition (module docstring): (roundings, fp16 stores of intermediates) per stage
    @staticmethod
    def _generic_pass(shape, factor):
        t = [-(-n // factor) for n in shape]
        return (t[0] * t[1] + 2, 1) if len(t) == 2 else (2 * t[0] + 2, 2)

    def generic_u(self, bias=True):
        n, k = self._generic_pass(self.fu_shape, self.up)
        return n + (1 if bias else 0), k + (1 if bias else 0)

    def generic_down(self):
        n, k = self._generic_pass(self.fd_shape, 1)
        return n, k - 1                       # the last pass stores the result itself

    def generic_adjoint(self):
        (nu, ku), (nd, kd) = self._generic_pass(self.fd_shape, self.down), self._generic_pass(self.fu_shape, 1)
        return nu, ku, nd, kd - 1

    def n_down(self):
        td = self.fd_shape
        if len(td) == 1:
            return td[0] + (td[0] // 2 + 1 if td[0] > 1 else 1) + 1
        half = td[0] * td[1] // 2
        return (1 + half // 2 + 1 if self.fd_mirror else half + 1) + 1


_ops_cache = {}


def _ops(x_hw, fu, fd, up, down, padding, flip, dev):
    """The matrices of one call, kept for the next calls with the same geometry and taps (a few entries)."""
    taps = tuple(None if f is None else (tuple(f.shape), tuple(torch.as_tensor(f).flatten().tolist())) for f in (fu, fd))
    key = (int(x_hw[0]), int(x_hw[1]), taps, int(up), int(down), _four(padding), bool(flip), str(dev))
    if key not in _ops_cache:
        if len(_ops_cache) >= 4:
            _ops_cache.clear()
        _ops_cache[key] = Ops(int(x_hw[0]), int(x_hw[1]), fu, fd, up, down, padding, flip, dev)
    return _ops_cache[key]


def _planes(x, b=None):
    n, c, h, w = x.shape
    x64 = x.detach().to(torch.float64)
    if b is not None:
        x64 = x64 + b.detach().to(torch.float64)[None, :, None, None]
    return x64.reshape(n * c, h, w)


def _act(u, gain, slope, clamp):
    """clamp(lrelu(gain * u)) and the decision per sample: (value, negative, clamped)."""
    g, s = f32(gain), f32(slope)
    c = math.inf if clamp is None or math.isinf(clamp) else f32(clamp)
    v = u * g
    neg = v < 0
    lv = torch.where(neg, v * s, v)
    big = lv.abs() > c
    val = torch.where(big, torch.copysign(torch.full_like(lv, c if math.isfinite(c) else 0.0), lv), lv)
    return val, neg, big


def forward_ref(x, b, fu, fd, up, down, padding, gain, slope, clamp, flip):
    """(y64 [N,C,yH,yW], u64 [N,C,uH,uW]): the output and the upsampled pre-activation (before the gain) the sign code classifies."""
    n, c = x.shape[:2]
    ops = _ops(x.shape[2:], fu, fd, up, down, padding, flip, x.device)
    u = Ops.apply(ops.A, _planes(x, b))
    a, _, _ = _act(u, gain, slope, clamp)
    y = Ops.apply(ops.B, a)
    return y.reshape(n, c, *ops.y_hw), u.reshape(n, c, *ops.u_hw)


def sign_codes_ref(u64, gain, slope, clamp):
    """The float64 decision per upsampled sample as the 2-bit code: 0 = positive, 1 = negative, 2 = clamped."""
    _, neg, big = _act(u64, gain, slope, clamp)
    return torch.where(big, 2, torch.where(neg, 1, 0)).to(torch.uint8)


def _adj_gain(gain, up, down):
    return f32(gain * up ** 2 / down ** 2) * down ** 2 / up ** 2


def adjoint_ref(dy, u64, x_hw, fu, fd, up, down, padding, gain, slope, clamp, flip):
    """(dx64 [N,C,xH,xW], db64 [C]) of the forward call with these arguments at the pre-activation u64 (the float64 decision
    {1, slope, 0} * gain per upsampled sample)."""
    n, c = dy.shape[:2]
    ops = _ops(x_hw, fu, fd, up, down, padding, flip, dy.device)
    g_up = Ops.apply(ops.B, _planes(dy), transpose=True)
    _, neg, big = _act(u64.reshape(n * c, *ops.u_hw), gain, slope, clamp)
    s = f32(slope)
    m = torch.where(big, 0.0, torch.where(neg, s, 1.0)).to(torch.float64) * _adj_gain(gain, up, down)
    dx = Ops.apply(ops.A, g_up * m, transpose=True).reshape(n, c, *x_hw)
    return dx, dx.sum([0, 2, 3])


# ------------------------------------------------------------------------------------------------------------ abs scales

def abs_scale_forward(x, b, fu, fd, up, down, padding, gain, slope, clamp, flip):
    """(su, sy_pre, sy_post): |A| |x + b|;  gain |B| su (what the roundings before the activation count against);
    |B| min(gain su, clamp) (those after it)."""
    n, c = x.shape[:2]
    ops = _ops(x.shape[2:], fu, fd, up, down, padding, flip, x.device)
    su = Ops.apply(ops.A, _planes(x, b).abs(), absolute=True)
    g = f32(gain)
    cl = math.inf if clamp is None or math.isinf(clamp) else f32(clamp)
    sy_pre = Ops.apply(ops.B, su * g, absolute=True)
    sy_post = Ops.apply(ops.B, (su * g * SECOND).clamp(max=cl), absolute=True)
    return su.reshape(n, c, *ops.u_hw), sy_pre.reshape(n, c, *ops.y_hw), sy_post.reshape(n, c, *ops.y_hw)


def abs_scale_adjoint(dy, u64, x_hw, fu, fd, up, down, padding, gain, slope, clamp, flip):
    """(|B|^T |dy|, |A|^T (m gain |B|^T |dy|)): the adjoint's pipeline on |dy| with |taps|."""
    n, c = dy.shape[:2]
    ops = _ops(x_hw, fu, fd, up, down, padding, flip, dy.device)
    sg = Ops.apply(ops.B, _planes(dy).abs(), absolute=True, transpose=True)
    _, neg, big = _act(u64.reshape(n * c, *ops.u_hw), gain, slope, clamp)
    m = torch.where(big, 0.0, torch.where(neg, f32(slope), 1.0)).to(torch.float64) * _adj_gain(gain, up, down)
    sdx = Ops.apply(ops.A, sg * m, absolute=True, transpose=True)
    return sg.reshape(n, c, *ops.u_hw), sdx.reshape(n, c, *x_hw)


# ------------------------------------------------------------------------------------------------------------------ bounds

def _f16_store(ref, bound):
    return torch.maximum(F16_REL * (ref.abs() + bound), torch.full_like(ref, F16_SUB))


def forward_bounds(x, b, fu, fd, up, down, padding, gain, slope, clamp, flip, y_ref=None, fp16=False, scales=None, generic=False, unit=U):
    """(bound_y, bound_u): element-wise bounds on |y(kernel) - y64| and on the kernel's error of u.  x and b as the kernel read them.
    `generic`: the counts of the generic composition, `unit`: its tensors' unit roundoff (module docstring)."""
    ops = _ops(x.shape[2:], fu, fd, up, down, padding, flip, x.device)
    su, sy_pre, sy_post = scales or abs_scale_forward(x, b, fu, fd, up, down, padding, gain, slope, clamp, flip)      # `scales`: if the caller has them
    if generic:
        (nu, ku), (nd, kd) = ops.generic_u(), ops.generic_down()
        h = F16_REL if fp16 else 0.0
        bound_u = (nu * unit + ku * h) * SECOND * su
        bound_y = ((nu + 1) * unit + (ku + 1) * h) * SECOND * sy_pre + (nd * unit + kd * h) * SECOND * sy_post
        if fp16:
            bound_y = bound_y + _f16_store(y_ref, bound_y)
        return bound_y, bound_u
    bound_u = ops.n_u() * U * SECOND * su
    bound_y = ((ops.n_u() + 1) * sy_pre + ops.n_down() * sy_post) * U * SECOND
    if fp16:
        bound_y = bound_y + _f16_store(y_ref, bound_y)
    return bound_y, bound_u


def ambiguous(u64, bound_u, su, gain, slope, clamp, unit=U):
    """(at zero, at the clamp): samples whose decision the kernel's rounding of u may change."""
    g, s = f32(gain), f32(slope)
    at0 = (u64.abs() <= bound_u) & (su > 0)
    if clamp is None or math.isinf(clamp):
        return at0, torch.zeros_like(at0)
    v = u64 * g
    neg = v < 0
    k = torch.where(neg, s, 1.0).to(torch.float64)
    err = (bound_u * g + 2 * unit * v.abs()) * k * SECOND
    atc = ((v * k).abs() - f32(clamp)).abs() <= err
    return at0, atc


def adjoint_bounds(dy, u64, bound_u, su, x_hw, fu, fd, up, down, padding, gain, slope, clamp, flip, dx_ref=None, fp16=False, generic=False,
                   unit=U):
    """(bound_dx, widening, n_adj): the element-wise bound on |dx(kernel) - dx64| (widening included), the widening alone, and the
    rounding count.  `bound_u`, `su`: of the forward that wrote the signs (`forward_bounds`, `abs_scale_forward`).  `generic`, `unit`:
    as in `forward_bounds` (n_adj then counts an fp16 store as 2^-11 / unit roundings)."""
    n, c = dy.shape[:2]
    ops = _ops(x_hw, fu, fd, up, down, padding, flip, dy.device)
    # the adjoint call runs with (up, fu) <-> (down, fd): its "up" filter is fd, its "down" filter fu
    td = ops.fd_shape
    tu_adj = [-(-t // ops.down) for t in td]
    n_up = tu_adj[0] * tu_adj[1] if len(td) == 2 else 2 * tu_adj[0]
    tf = ops.fu_shape
    n_dn = (tf[0] + (tf[0] // 2 + 1 if tf[0] > 1 else 1) + 1) if len(tf) == 1 else (tf[0] * tf[1] // 2 + 2)
    n_adj = n_up + 1 + n_dn
    if generic:
        n_up, k_up, n_dn, k_dn = ops.generic_adjoint()
        h = F16_REL / unit if fp16 else 0.0
        n_adj = n_up + 1 + n_dn + (k_up + 1 + k_dn) * h
        n_up = n_up + k_up * h
    sg, sdx = abs_scale_adjoint(dy, u64, x_hw, fu, fd, up, down, padding, gain, slope, clamp, flip)
    at0, atc = ambiguous(u64, bound_u, su, gain, slope, clamp, unit)
    s = f32(slope)
    neg = u64 < 0
    jump = at0.to(torch.float64) * (1.0 - s) + atc.to(torch.float64) * torch.where(neg, s, 1.0).to(torch.float64)
    # the kernel's own g_up: within n_up u sg of the exact one
    g_up = Ops.apply(ops.B, _planes(dy), transpose=True).reshape(n, c, *ops.u_hw).abs() + n_up * unit * SECOND * sg
    wid = Ops.apply(ops.A, (jump * _adj_gain(gain, up, down) * g_up).reshape(n * c, *ops.u_hw), absolute=True,
                    transpose=True).reshape(n, c, *x_hw)
    bound = n_adj * unit * SECOND * sdx + wid
    if fp16:
        bound = bound + _f16_store(dx_ref, bound)
    return bound, wid, n_adj


def db_bound(bound_dx, dx_ref, acc_terms=None):
    """[C] bound on |db - sum dx64|: the sum of the element bounds plus the accumulation of the partial sums.  `acc_terms`:
    CH + 7 + slots * N for the fused adjoint; None: any order of a plain sum."""
    cnt = dx_ref.shape[0] * dx_ref.shape[2] * dx_ref.shape[3]
    t = cnt - 1 if acc_terms is None else acc_terms
    sb = bound_dx.sum([0, 2, 3])
    return sb + t * U * SECOND * (dx_ref.abs().sum([0, 2, 3]) + sb)


def widened_share(wid):
    return float((wid > 0).to(torch.float64).mean())


def ratio(err, bound):
    """max err / bound (an element with bound 0 must be exact)."""
    bad = (bound <= 0) & (err > 0)
    assert not bool(bad.any()), 'nonzero error where the bound is zero'
    return float((err / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------------------- sign tensor

def decode_signs(s, sx, sy, u_hw):
    """The 2-bit codes of the upsampled buffer [N,C,uH,uW] (uint8) from the sign tensor s [N,C,sH,sWbytes]: sample (uy, ux) sits
    in row uy + sy, column ux + sx; a byte holds 4 consecutive columns, the first in its lowest bits; 1 = negative, 2 = clamped.
    Samples outside the tensor decode to 255."""
    n, c, sh, swb = s.shape
    uh, uw = u_hw
    cols = torch.stack([(s >> (2 * q)) & 3 for q in range(4)], -1).reshape(n, c, sh, swb * 4)
    out = torch.full([n, c, uh, uw], 255, dtype=torch.uint8, device=s.device)
    y0, y1 = max(0, -sy), min(uh, sh - sy)
    x0, x1 = max(0, -sx), min(uw, swb * 4 - sx)
    out[:, :, y0:y1, x0:x1] = cols[:, :, y0 + sy:y1 + sy, x0 + sx:x1 + sx]
    return out


def sign_mismatches(s, sx, sy, u64, amb, gain, slope, clamp, active_hw=None):
    """Number of non-ambiguous samples whose stored code differs from the float64 decision.  `active_hw`: the rows and columns of
    the upsampled buffer the down pass reads (yH * down - (down - 1) + fdH - 1, likewise for the width); default: all."""
    got = decode_signs(s, sx, sy, tuple(u64.shape[2:]))
    want = sign_codes_ref(u64, gain, slope, clamp)
    bad = (got != want) & ~amb
    if active_hw is not None:
        bad = bad[:, :, :active_hw[0], :active_hw[1]]
    return int(bad.sum())
