"""float64 references, error bounds and test cases of the style and input stage: `sg3_affine_batch`, `sg3_input_transform`,
`sg3_fourier_features` (csrc/sg3_affine.hip, csrc/sg3_fourier.hip) and `sg3_modulated_conv2d_prep[_batch]` (csrc/sg3_modconv.hip).

Plain torch / numpy, no libsg3hip call.  Every reference takes the float32 values the kernel reads and evaluates the same formula in
float64.  u = 2^-24 is the fp32 unit roundoff; "n roundings" means a factor (1 + delta)^n, |delta| <= u, bounded by n u / (1 - n u)
(`_gamma`).  The bounds are worst-case and element-wise: the sums below are short (a lane adds at most 36 terms before a tree takes
over), so the worst case stays within 4e-6 relative at the largest shape and no probabilistic model is needed.

affine_batch.  One wave per output row: lane l adds its w_dim / 64 (rounded up) products x[k] W[r,k] with one fma each, six
    butterfly steps add the lanes, then (acc + b) * scale: ceil(w_dim / 64) + 8 roundings on sum_k |x_k W_rk| + |b_r|, times |scale|
    (`affine_bound`).  W = fp32(weight * weight_gain) and b = fp32(bias * bias_gain) are the kernel's INPUTS (`AffinePack._build`
    rounds them once, as the reference's FullyConnectedLayer does), so `affine_ref` starts from those.

modconv prep (`prep_ref`, `prep_bounds`; formulas: include/sg3_ops.h above sg3_modconv_prep_params).
    pre-normalisation  scale = rsqrt(sum_j a_j^2 / len), len = I k^2 (weights, per o) or N I (styles, whole batch): a thread adds
        m = ceil(len / 256) squares (m + 1 roundings on a sum of positive terms), an 8-level tree (8), the division (1); the rsqrt halves
        that and adds its own error, allowed 2 ulp = 4 u:  R(len) = (m + 10) / 2 + 4.  Without demodulation scale = 1 exactly: R = 0.
    wsq[o,i] = sum_t (w scale)^2:  each term 2 (R_w + 1) + 1, the sum of k^2 positive terms k^2 more:  A_wsq = 2 R_w + 3 + k^2.
    v = s scale g (sIn before its power of two):  A_v = R_s + 1 with demodulation (the product by the scale), one more with a gain;
        without demodulation s * 1 is exact: 1 with a gain, 0 without (sIn is then s times a power of two, exactly).
    s2 = (s scale)^2:  2 (R_s + 1) + 1.
    S = sum_i wsq s2: products A_wsq + A_s2 + 1; a lane adds ceil(I / 64) of them, six butterfly steps; + 1e-8f (the constant and the
        addition, 1 each):  A_S = A_wsq + A_s2 + ceil(I / 64) + 9;  d = rsqrt(S + 1e-8):  A_d = A_S / 2 + 4.
    All of it relative to the float64 value (every sum is of positive terms), so |wsq - ref| <= gamma(A_wsq) ref etc.
    The power of two: e = ceil(log2(peak / 32768)), peak = max_i |v| xBound, one more in the transform-domain forms, 0 for fp32 and for a
        peak of 0 / inf / NaN; sIn = v 2^-e and dcoef = d 2^e are exact scalings.  The kernel keeps e within [-E_LIMIT, E_LIMIT] so that
        both factors are normal floats (`prep_ref` returns the exact e and the kept one).  Tests keep peak at least 1e-4 relative away from a
        power of two (log2f's own error at |log2| ~ 135 is 1e-5 relative), but for one case constructed to sit on it exactly.

input_transform (`input_transform_bound`).  t' = t / sqrt(t0^2 + t1^2): 2 + 2 (sqrt, allowed 2 u) + 1 (division) = 5 on every entry of
    R(t') and T(t').  A 3x3 product row is mul, fma, fma: 3 roundings on sum_j |a_ij| |b_jk|; two products (R T) U: with
    P = |R| |T| |U| (float64, element-wise absolute values) |M - M_ref| <= gamma(5 + 5 + 3 + 3) P.  Then
        phase' = phase + (f0 M02 + f1 M12):   gamma(16 + 2) (|f0| P02 + |f1| P12) + u |phase'|          (one addition)
        f'_k   = f0 M0k + f1 M1k:             gamma(16 + 2) (|f0| P0k + |f1| P1k)                        =: E_k
        |f'|:  |fl - ref| <= hypot(E_0, E_1) + 4 u |f'|  (the norm is 1-Lipschitz; two squares, sum, sqrt allowed 2 u)
        amp = clamp(1 - (|f'| - bw) / (sr / 2 - bw), 0, 1): the clamp is 1-Lipschitz; with D = sr / 2 - bw (2 roundings, relative)
              |amp - ref| <= (E_norm + 4 u ||f'| - bw|) / D + u (1 + ||f'| - bw| / D)
    Without `normalise` the 5 roundings of t' are absent (the bound keeps them: an upper bound all the same).

fourier_features (`fourier_bound`).  arg = (gy f1 + gx f0 + phase) * 2 pi: with a = |gx f0| + |gy f1| + |phase| (cycles) the product,
    the fma, the addition and the multiplication by fp32(2 pi) (itself 0.47 u off) are at most 4.5 u a: 5 u a taken.  sin is
    1-Lipschitz, sinf allowed 2 ulp <= 4 u absolute, the amplitude product u:
        |out - ref| <= |amp| (2 pi 5 u a + 4 u) + u |ref|
    -- the error grows with the argument: at 200 cycles 2 pi 5 u 200 = 4e-4.

The second, device-relative yardstick (tests/test_gpu_styleclip_mapper.py): per tensor
    max |hip - fp64| <= 2 max |torch32 - fp64| + 1e-7 max |fp64|,  torch32 = the module's own chain of fp32 torch ops on the same device;
`input_transform_chain` and `fourier_chain` are that chain, written once and run in float64 (the reference) or float32 (torch32).
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
E_LIMIT = 126                      # |e| the prep kernel keeps: 2^e and 2^-e are normal floats
CONV_FP32, CONV_F16X3, CONV_F16, CONV_F16X3_F23, CONV_F16_F23 = range(5)          # torch_utils/_sg3abi.py
F23_FORMS = (CONV_F16X3_F23, CONV_F16_F23)
PREC_NAMES = ('fp32', 'f16x3', 'f16', 'f16x3_f23', 'f16_f23')


def _gamma(n):
    return n * U / (1 - n * U)


# ---------------------------------------------------------------------------------------------------------------- affine_batch

def affine_inputs(weight, bias, weight_gain, bias_gain):
    """(W, b) float32 as `AffinePack._build` hands them to the kernel: fp32(weight * weight_gain), fp32(bias * bias_gain) or zeros."""
    w = weight.detach().to(device='cpu', dtype=torch.float32) * weight_gain
    b = torch.zeros([w.shape[0]]) if bias is None else bias.detach().to(device='cpu', dtype=torch.float32) * bias_gain
    return w, b


def affine_ref(ws, weight, bias, weight_gain, bias_gain, post):
    """((ws @ W^T + b) * post, element-wise bound) float64 [N, rows] for one layer; ws [N, w_dim] float32."""
    w, b = affine_inputs(weight, bias, weight_gain, bias_gain)
    x, w, b = ws.detach().cpu().double(), w.double(), b.double()
    sc = float(np.float32(post))
    ref = (x @ w.t() + b) * sc
    return ref, affine_bound(x, w, b, sc)


def affine_bound(x, w, b, scale):
    return _gamma(math.ceil(x.shape[1] / 64) + 8) * (x.abs() @ w.abs().t() + b.abs()) * abs(scale)


# ------------------------------------------------------------------------------------------------------------------ modconv prep

def prep_ref(w, s, demodulate, input_gain, x_bound, precision):
    """float64 outcome of the prep kernels for w [O,I,k,k], s [N,I], input_gain None | [] | [I] | [N,I] (float32 values), x_bound the
    fp32 bound as a number.  dict: wn [O,I,k,k], wsq [O,I], v [N,I] (= sIn 2^e), d [N,O] (= dcoef 2^-e; ones without demodulation),
    peak [N], e [N] (exact, int), e_kept [N] (within +-E_LIMIT: what the kernel applies)."""
    w, s = w.detach().cpu().double(), s.detach().cpu().double()
    n, ci = s.shape
    if demodulate:
        w = w * w.square().mean([1, 2, 3], keepdim=True).rsqrt()
        s = s * s.square().mean().rsqrt()
    wsq = w.square().sum([2, 3])
    v = s if input_gain is None else s * input_gain.detach().cpu().double().expand(n, ci)
    d = (s.square() @ wsq.t() + 1e-8).rsqrt() if demodulate else torch.ones([n, w.shape[0]], dtype=torch.float64)
    peak = torch.where(torch.isnan(v), torch.zeros_like(v), v.abs()).amax(dim=1) * float(x_bound)     # fmaxf drops a NaN
    e = []
    for pk in peak.tolist():
        ex = 0
        if precision != CONV_FP32:
            if 0 < pk < 3.0e38:
                ex = math.ceil(math.log2(pk / 32768.0))
            if precision in F23_FORMS:
                ex += 1
        e.append(ex)
    e = np.asarray(e, dtype=np.int64)
    return dict(wn=w, wsq=wsq, v=v, d=d, peak=peak.numpy(), e=e, e_kept=np.clip(e, -E_LIMIT, E_LIMIT))


def _norm_roundings(length):
    return (math.ceil(length / 256) + 10) / 2 + 4


def prep_bounds(n, ci, k, demodulate, has_gain):
    """Relative element-wise bounds (wsq, v, d) of the prep outputs, module docstring."""
    r_w = _norm_roundings(ci * k * k) if demodulate else 0
    r_s = _norm_roundings(n * ci) if demodulate else 0
    a_wsq = 2 * r_w + 3 + k * k
    a_v = r_s + (1 if demodulate else 0) + (1 if has_gain else 0)
    a_s2 = 2 * (r_s + 1) + 1
    a_d = (a_wsq + a_s2 + math.ceil(ci / 64) + 9) / 2 + 4
    return _gamma(a_wsq), _gamma(a_v), _gamma(a_d)


def pow2_distance(peak):
    """Relative distance of `peak` from the nearest power of two."""
    m, _ = math.frexp(peak)                    # m in [0.5, 1)
    return min(m / 0.5 - 1, 1 - m)


# test cases of the prep kernels, shared by the GPU test (runs them) and the CPU test (checks the conditions they rely on)
PREP_I = (1, 17, 64, 70, 257, 1024)
PREP_O = (3, 33, 130, 513, 1024)
PREP_XBOUNDS = (2.0 ** -100, 1e-6, 1.0, 3.0, 65504.0)
PREP_STYLE_SCALES = (1e-4, 1.0, 1e4)
PREP_WEIGHT_SCALES = (2.0 ** -8, 1.0, 2.0 ** 8)
MAX_WEIGHT_ELEMENTS = 2_400_000              # 10 MB of fp32


def make_case(n, ci, co, k, demodulate, gain_mode, precision, x_bound, bound_on_device=False, style_scale=1.0, weight_scale=1.0,
              small_sample=False, seed=0, tag='shape'):
    return dict(N=n, I=ci, O=co, k=k, demodulate=bool(demodulate), gain_mode=gain_mode, precision=precision,
                x_bound=float(np.float32(x_bound)), bound_on_device=bool(bound_on_device), style_scale=style_scale, weight_scale=weight_scale,
                small_sample=bool(small_sample), seed=seed,
                id=tag + '_N%d_I%d_O%d_k%d_%s_g%d_%s_x%.3g%s_s%g_w%g%s' % (n, ci, co, k, 'demod' if demodulate else 'plain', gain_mode, PREC_NAMES[precision],
                                                                 x_bound, 'dev' if bound_on_device else '', style_scale, weight_scale,
                                                                 '_small' if small_sample else ''))


def shape_cases():
    """Every (I, O) pair at k = 1 and k = 3 (weights up to 10 MB), the other settings cycling so that each value meets many shapes."""
    out, j = [], 0
    for k in (1, 3):
        for ci in PREP_I:
            for co in PREP_O:
                if ci * co * k * k > MAX_WEIGHT_ELEMENTS:
                    continue
                prec = (CONV_F16X3, CONV_FP32, CONV_F16, CONV_F16X3_F23, CONV_F16_F23)[j % 5] if k == 3 else (CONV_F16X3, CONV_FP32, CONV_F16)[j % 3]
                n, demod, mode = (1, 3)[j % 2], (j // 2) % 2 == 0, j % 4
                if n * ci == 1 and demod and mode == 0:
                    mode = 1                    # one normalised style is +-1: without a gain the peak would be the bound itself, often 2^j
                out.append(make_case(n, ci, co, k, demod, mode, prec, 0.0 if prec == CONV_FP32 else PREP_XBOUNDS[j % 5],
                                     bound_on_device=(j % 7 in (2, 5, 6) and prec != CONV_FP32), small_sample=(j % 2 == 1), seed=100 + j))
                j += 1
    return out


VARIATION_SHAPES = ((3, 70, 33, 3), (3, 257, 513, 1), (1, 64, 130, 3))          # N, I, O, k


def variation_cases(shape):
    """demodulate x gain mode x precision x (host | device bound) at one shape."""
    n, ci, co, k = shape
    out = []
    for demod in (True, False):
        for mode in range(4):
            for prec in range(5 if k == 3 else 3):
                for dev in ((False,) if prec == CONV_FP32 else (False, True)):
                    out.append(make_case(n, ci, co, k, demod, mode, prec, 0.0 if prec == CONV_FP32 else 3.0, dev, small_sample=(n > 1),
                                         seed=300 + len(out), tag='var'))
    return out


MAGNITUDE_SHAPES = ((3, 17, 33, 3), (3, 1, 3, 1))


def magnitude_cases(shape):
    """styles x weights x bound magnitudes, with and without demodulation; one sample of the batch 1e-3 of the others."""
    n, ci, co, k = shape
    out = []
    for ss in PREP_STYLE_SCALES:
        for wscale in PREP_WEIGHT_SCALES:
            for xb in PREP_XBOUNDS:
                for demod in (True, False):
                    j = len(out)
                    prec = (CONV_F16X3, CONV_F16, CONV_F16X3_F23 if k == 3 else CONV_F16X3)[j % 3]
                    out.append(make_case(n, ci, co, k, demod, (1, 0, 3, 2)[j % 4], prec, xb, j % 2 == 1, ss, wscale, True, seed=520 + j, tag='mag'))
    return out


EXACT_J = (-40, -3, 0, 1, 7, 30)


def exact_cases():
    """peak = 32768 * 2^j exactly: I = 1, no demodulation, no gain, s = 1 (see `case_inputs`): e = j."""
    return [dict(make_case(2, 1, 3, 1, False, 0, prec, 32768.0 * 2.0 ** j, dev, seed=700, tag='exact'), exact_j=j)
            for j in EXACT_J for prec, dev in ((CONV_F16X3, False), (CONV_F16, True))]


def tiny_cases():
    """peak near 2^-120 through the device bound (a gradient that has almost underflowed): below the exponents both scale factors can
    take as normal floats."""
    return [make_case(3, 70, 33, k, demod, 1 if demod else 0, prec, 1.3 * 2.0 ** -121, True, seed=800 + j, tag='tiny')
            for j, (k, demod, prec) in enumerate(((3, True, CONV_F16X3), (3, False, CONV_F16), (1, True, CONV_F16), (3, True, CONV_F16X3_F23),
                                                  (3, False, CONV_F16_F23)))]


def all_exponent_cases():
    out = shape_cases() + exact_cases() + tiny_cases()
    for sh in VARIATION_SHAPES:
        out += variation_cases(sh)
    for sh in MAGNITUDE_SHAPES:
        out += magnitude_cases(sh)
    return out


def case_styles(c):
    """(s [N,I], gain None | [1] | [I] | [N,I]) float32 numpy of a case (their own random stream: the exponent depends on these alone)."""
    r = np.random.RandomState(c['seed'])
    n, ci = c['N'], c['I']
    if 'exact_j' in c:
        return np.ones([n, ci], dtype=np.float32), None
    s = (r.randn(n, ci) + 1).astype(np.float32) * np.float32(c['style_scale'])
    if c['small_sample'] and n > 1:
        s[n - 1] *= np.float32(1e-3)
    gain = [None, np.asarray([0.8]), r.rand(ci) + 0.5, r.rand(n, ci) + 0.5][c['gain_mode']]
    return s.astype(np.float32), None if gain is None else gain.astype(np.float32)


def case_weights(c):
    r = np.random.RandomState(c['seed'] + 10000)
    return (r.randn(c['O'], c['I'], c['k'], c['k']).astype(np.float32) * np.float32(c['weight_scale'])).astype(np.float32)


def case_peaks(c):
    """peak [N] float64 of a case without its weights."""
    s, gain = case_styles(c)
    s = torch.from_numpy(s).double()
    if c['demodulate']:
        s = s * s.square().mean().rsqrt()
    v = s if gain is None else s * torch.from_numpy(gain).double()
    return (v.abs().amax(dim=1) * c['x_bound']).numpy()


# ------------------------------------------------------------------------------------------------------------- input_transform

def input_transform_chain(t, user, freqs, phases, bandwidth, sampling_rate, normalise, dtype=torch.float64):
    """(freqs [N,C,2], phases [N,C], amps [N,C]) of SynthesisInput.forward (networks_stylegan3.py:204-230) in `dtype`, on the device of
    `t`: the module's own op chain (t [N,4], user [3,3] | [N,3,3], freqs [C,2], phases [C]).  float64: the reference; float32: the
    torch composite the kernel replaces."""
    t, user, freqs, phases = (a.to(dtype) for a in (t, user, freqs, phases))
    if normalise:
        t = t / t[:, :2].norm(dim=1, keepdim=True)
    rows = lambda a, b, c: torch.stack([a, b, c], dim=1)          # noqa: E731
    one, zero = torch.ones_like(t[:, 0]), torch.zeros_like(t[:, 0])
    rot = torch.stack([rows(t[:, 0], -t[:, 1], zero), rows(t[:, 1], t[:, 0], zero), rows(zero, zero, one)], dim=1)
    trans = torch.stack([rows(one, zero, -t[:, 2]), rows(zero, one, -t[:, 3]), rows(zero, zero, one)], dim=1)
    m = rot @ trans @ user
    f = freqs.unsqueeze(0)
    ph = phases.unsqueeze(0) + (f @ m[:, :2, 2:]).squeeze(2)
    f = f @ m[:, :2, :2]
    amps = (1 - (f.norm(dim=2) - bandwidth) / (sampling_rate / 2 - bandwidth)).clamp(0, 1)
    return f, ph, amps


def input_transform_ref(t, user, freqs, phases, bandwidth, sampling_rate, normalise):
    return input_transform_chain(t, user, freqs, phases, bandwidth, sampling_rate, normalise, torch.float64)


def input_transform_bound(t, user, freqs, phases, bandwidth, sampling_rate, normalise):
    """Element-wise bounds (freqs [N,C,2], phases [N,C], amps [N,C]) float64 on the error of the kernel, module docstring."""
    t, user, freqs, phases = (a.double() for a in (t, user, freqs, phases))
    f_ref, ph_ref, _ = input_transform_chain(t, user, freqs, phases, bandwidth, sampling_rate, normalise)
    if normalise:
        t = t / t[:, :2].norm(dim=1, keepdim=True)
    a = t.abs()
    n = t.shape[0]
    one, zero = torch.ones_like(a[:, 0]), torch.zeros_like(a[:, 0])
    rows = lambda x, y, z: torch.stack([x, y, z], dim=1)          # noqa: E731
    rot = torch.stack([rows(a[:, 0], a[:, 1], zero), rows(a[:, 1], a[:, 0], zero), rows(zero, zero, one)], dim=1)
    trans = torch.stack([rows(one, zero, a[:, 2]), rows(zero, one, a[:, 3]), rows(zero, zero, one)], dim=1)
    p = rot @ trans @ user.abs().expand(n, 3, 3)
    fa = freqs.abs().unsqueeze(0)
    g = _gamma(18)
    e_f = g * (fa @ p[:, :2, :2])                                                     # [N,C,2]
    e_ph = g * (fa @ p[:, :2, 2:]).squeeze(2) + U * ph_ref.abs()
    nrm = f_ref.norm(dim=2)
    den = sampling_rate / 2 - bandwidth
    e_nrm = e_f.norm(dim=2) + 4 * U * nrm
    off = (nrm - bandwidth).abs()
    e_amp = (e_nrm + 4 * U * off) / den + U * (1 + off / den)
    return e_f, e_ph, e_amp


# ------------------------------------------------------------------------------------------------------------ fourier_features

def fourier_chain(grid, freqs, phases, amps, dtype=torch.float64):
    """[N,C,H,W] of the reference's feature chain (networks_stylegan3.py:236-241, channels first) in `dtype`: grid [H,W,2],
    freqs [N,C,2], phases [N,C], amps [N,C]."""
    grid, freqs, phases, amps = (a.to(dtype) for a in (grid, freqs, phases, amps))
    x = (grid.unsqueeze(0).unsqueeze(3) @ freqs.permute(0, 2, 1).unsqueeze(1).unsqueeze(2)).squeeze(3)      # [N,H,W,C]
    x = x + phases.unsqueeze(1).unsqueeze(2)
    x = torch.sin(x * (np.pi * 2))
    x = x * amps.unsqueeze(1).unsqueeze(2)
    return x.permute(0, 3, 1, 2)


def fourier_ref(grid, freqs, phases, amps):
    return fourier_chain(grid, freqs, phases, amps, torch.float64)


def fourier_bound(grid, freqs, phases, amps, ref):
    """Element-wise bound [N,C,H,W] float64, module docstring."""
    grid, freqs, phases, amps = (a.double() for a in (grid, freqs, phases, amps))
    a = (grid.abs().unsqueeze(0).unsqueeze(3) @ freqs.abs().permute(0, 2, 1).unsqueeze(1).unsqueeze(2)).squeeze(3)
    a = (a + phases.abs().unsqueeze(1).unsqueeze(2)).permute(0, 3, 1, 2)
    return amps.abs().unsqueeze(2).unsqueeze(3) * (2 * np.pi * 5 * U * a + 4 * U) + U * ref.abs()


def sampling_grid(width, height, sampling_rate, device='cpu'):
    """The [H,W,2] float32 grid of SynthesisInput (reference :231-234)."""
    theta = torch.eye(2, 3, device=device)
    theta[0, 0] = 0.5 * width / sampling_rate
    theta[1, 1] = 0.5 * height / sampling_rate
    return torch.nn.functional.affine_grid(theta.unsqueeze(0), [1, 1, height, width], align_corners=False)[0]


def synth_freqs(c, bandwidth, seed):
    """(freqs [C,2], phases [C]) float32 drawn like SynthesisInput.__init__ (reference :181-186)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn([c, 2], generator=g)
    r = f.norm(dim=1, keepdim=True)
    f = f / (r * r.square().exp().pow(0.25)) * bandwidth
    return f, torch.rand([c], generator=g) - 0.5


def rotation_user(angle_deg, tx, ty):
    """A [3,3] float32 user transform: rotation by `angle_deg`, then a translation."""
    a = math.radians(angle_deg)
    return torch.tensor([[math.cos(a), -math.sin(a), tx], [math.sin(a), math.cos(a), ty], [0.0, 0.0, 1.0]], dtype=torch.float32)
