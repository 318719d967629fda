"""float64 references and error models of the three generic operators: upfirdn2d, bias_act and filtered_lrelu_act_.

Plain torch, no libsg3hip call.  Everything runs wherever its inputs live.  Scalars (gain, alpha, slope, clamp) are the fp32 values
that cross the ABI, converted to float64; filter taps are fp32 tensors converted to float64 before any scaling.

upfirdn2d
    `upfirdn_ref`: zero-stuff, pad or crop, correlate (taps flipped unless `flip`), decimate, multiply by the gain.  No convolution
    call: one shifted, strided slice of the padded image per tap.
    `upfirdn_bound`, element by element:  (T + 2) * u * upfirdn_abs,  upfirdn_abs the same pipeline on |x|, |f|, |gain|.
    T = ceil(fH / upy) * ceil(fW / upx) taps can meet a real sample; each is one product accumulated in the tensor's accumulate type
    (fp32 for fp32 and fp16 tensors, u = 2^-24; float64 for float64, u = 2^-53); + 2: the gain product and the result's rounding.
    A separable filter is two calls: T = ceil(fW / upx) + ceil(fH / upy), + 4.  An fp16 result adds 2^-11 |ref| + 2^-25 (half a
    step of the normal / of the subnormal grid); a separable fp16 call also stores its first pass in fp16: 2^-11 times the second
    pass on |first pass|, and where that intermediate is subnormal 2^-25 instead (the same two grids).

bias_act
    `bias_act_def`: the definition from torch's float64 functions; derivatives by autograd.
    `bias_act_formulas`: value (order 0), d/dx applied to dy (order 1) and d2/dx2 applied to ddx (order 2) from the formulas of the
    reference's kernel: derivatives in terms of the saved output y / gain (of x + b for swish), tanh as (e^x - e^-x) / (e^x + e^-x),
    the +-80 cut-offs of tanh / sigmoid / softplus / swish and the 40 cut-off of swish's derivatives, the clamp as a mask on the
    saved output.  `dtype` selects the arithmetic: float32 is the yardstick of the kernel's fp32 arithmetic (`bias_act_formulas32`),
    float64 ties the formulas to the definition.

filtered_lrelu_act_
    `act_ref` / `act_codes`: v = x * gain; where v < 0, v * slope; clamp.  Codes: 1 negative, 2 clamped.  Each step is one IEEE
    operation, so evaluated in the accumulate type they are the kernel's exact result.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U64 = 2.0 ** -53
F16_REL = 2.0 ** -11
F16_SUB = 2.0 ** -25


def f32(v):
    """The float64 value of v rounded to fp32: what crosses the ABI."""
    return float(np.float32(v))


def unit(dtype):
    return U64 if dtype == torch.float64 else U32


# ------------------------------------------------------------------------------------------------------------------ upfirdn2d

def _xy(v):
    if isinstance(v, int):
        return v, v
    v = [int(a) for a in v]
    assert len(v) == 2
    return v[0], v[1]


def _four(padding):
    if isinstance(padding, int):
        return padding, padding, padding, padding
    p = [int(v) for v in padding]
    if len(p) == 2:
        return p[0], p[0], p[1], p[1]
    assert len(p) == 4
    return tuple(p)


def _taps(f, dev):
    """None -> a 1x1 one;  the fp32 taps as float64, untouched otherwise."""
    if f is None:
        return torch.ones([1, 1], dtype=torch.float64, device=dev)
    f = torch.as_tensor(f)
    assert f.dtype == torch.float32 and f.ndim in (1, 2)
    return f.detach().to(device=dev, dtype=torch.float64)


def _stuff_pad(x, upx, upy, px0, px1, py0, py1):
    n, c, h, w = x.shape
    z = x.new_zeros([n, c, h, upy, w, upx])
    z[:, :, :, 0, :, 0] = x
    z = z.reshape(n, c, h * upy, w * upx)
    z = F.pad(z, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    hh, ww = z.shape[2:]
    return z[:, :, max(-py0, 0): hh - max(-py1, 0), max(-px0, 0): ww - max(-px1, 0)]


def _correlate(z, g, downx, downy):
    """out[oy, ox] = sum g[ky, kx] z[oy * downy + ky, ox * downx + kx] over every position where the taps fit."""
    fh, fw = g.shape
    oh = (z.shape[2] - fh + downy) // downy
    ow = (z.shape[3] - fw + downx) // downx
    assert oh >= 1 and ow >= 1
    out = None
    for ky in range(fh):
        for kx in range(fw):
            t = z[:, :, ky: ky + (oh - 1) * downy + 1: downy, kx: kx + (ow - 1) * downx + 1: downx] * g[ky, kx]
            out = t if out is None else out + t
    return out


def _passes(f, flip, dev, absolute=False):
    """The correlation kernels of the call, in order: one 2-D kernel, or (row kernel, column kernel) of a separable filter."""
    g = _taps(f, dev)
    if absolute:
        g = g.abs()
    if not flip:
        g = g.flip(list(range(g.ndim)))
    return [g] if g.ndim == 2 else [g[None, :], g[:, None]]


def _pipeline(x, f, up, down, padding, flip, gain, absolute=False):
    upx, upy = _xy(up)
    downx, downy = _xy(down)
    px0, px1, py0, py1 = _four(padding)
    x = x.to(torch.float64)
    g = f32(gain)
    if absolute:
        x, g = x.abs(), abs(g)
    ks = _passes(f, flip, x.device, absolute)
    if len(ks) == 1:
        y = _correlate(_stuff_pad(x, upx, upy, px0, px1, py0, py1), ks[0], downx, downy)
        return y * g, None
    first = _correlate(_stuff_pad(x, upx, 1, px0, px1, 0, 0), ks[0], downx, 1)            # along x ...
    y = _correlate(_stuff_pad(first, 1, upy, 0, 0, py0, py1), ks[1], 1, downy)            # ... then along y
    return y * g, first


def upfirdn_ref(x, f, up=1, down=1, padding=0, flip=False, gain=1.0):
    return _pipeline(x, f, up, down, padding, flip, gain)[0]


def upfirdn_abs(x, f, up=1, down=1, padding=0, flip=False, gain=1.0):
    return _pipeline(x, f, up, down, padding, flip, gain, absolute=True)[0]


def tap_count(f, up):
    """(T, extra) of the module docstring."""
    upx, upy = _xy(up)
    if f is None:
        return 1, 2
    fh, fw = (int(f.shape[0]), int(f.shape[1])) if f.ndim == 2 else (int(f.shape[0]), int(f.shape[0]))
    if f.ndim == 2:
        return -(-fh // upy) * -(-fw // upx), 2
    return -(-fw // upx) + -(-fh // upy), 4


def upfirdn_bound(x, f, up=1, down=1, padding=0, flip=False, gain=1.0, dtype=torch.float32, ref=None):
    """Element-wise bound on |kernel - upfirdn_ref| for tensors of `dtype`; x as the kernel read it (already rounded)."""
    t, extra = tap_count(f, up)
    bound = (t + extra) * unit(dtype) * upfirdn_abs(x, f, up, down, padding, flip, gain)
    if dtype == torch.float16:
        if ref is None:
            ref = upfirdn_ref(x, f, up, down, padding, flip, gain)
        bound = bound + F16_REL * ref.abs() + F16_SUB
        if f is not None and f.ndim == 1:
            _, upy = _xy(up)
            _, downy = _xy(down)
            _, _, py0, py1 = _four(padding)
            first = _pipeline(x, f, up, down, padding, flip, gain)[1].abs()
            store = torch.where(first < 2.0 ** -14, torch.full_like(first, F16_SUB), F16_REL * first)
            col = _passes(f, flip, x.device, absolute=True)[1]
            bound = bound + _correlate(_stuff_pad(store, 1, upy, 0, 0, py0, py1), col, 1, downy) * abs(f32(gain))
    return bound


def adjoint_geometry(x_hw, y_hw, f, up, down, padding, flip):
    """(up, down, padding, flip) of the call that maps dy to dx: factors exchanged, the filter flipped, padded to the input's size."""
    upx, upy = _xy(up)
    downx, downy = _xy(down)
    px0, _, py0, _ = _four(padding)
    fh, fw = (1, 1) if f is None else ((int(f.shape[0]), int(f.shape[1])) if f.ndim == 2 else (int(f.shape[0]), int(f.shape[0])))
    (ih, iw), (oh, ow) = x_hw, y_hw
    pad = [fw - px0 - 1, iw * upx - ow * downx + px0 - upx + 1, fh - py0 - 1, ih * upy - oh * downy + py0 - upy + 1]
    return [downx, downy], [upx, upy], pad, not flip


def ratio(err, bound):
    """max err / bound (an element with bound 0 must be exact)."""
    bad = (bound <= 0) & (err > 0)
    assert not bool(bad.any()), 'nonzero error where the bound is zero'
    return float((err / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------------------------- bias_act

ACTS = ['linear', 'relu', 'lrelu', 'tanh', 'sigmoid', 'elu', 'selu', 'softplus', 'swish']
DEF_ALPHA = dict(lrelu=0.2)
DEF_GAIN = dict(relu=math.sqrt(2), lrelu=math.sqrt(2), swish=math.sqrt(2))
SELU_SCALE = 1.0507009873554804934193349852946
SELU_ALPHA = 1.6732632423543772848170429916717


def scalars(act, alpha, gain, clamp):
    """(alpha, gain, clamp) as they cross the ABI; clamp < 0: none."""
    a = f32(DEF_ALPHA.get(act, 0.0) if alpha is None else alpha)
    g = f32(DEF_GAIN.get(act, 1.0) if gain is None else gain)
    c = -1.0 if clamp is None else f32(clamp)
    return a, g, c


def _bshape(x, dim):
    return [-1 if i == dim else 1 for i in range(x.ndim)]


def bias_act_def(x, b=None, dim=1, act='linear', alpha=None, gain=None, clamp=None):
    """clamp(act(x + b) * gain) in float64 from torch's own functions; differentiable (pass float64 leaves)."""
    a, g, c = scalars(act, alpha, gain, clamp)
    x = x.to(torch.float64)
    if b is not None:
        x = x + b.to(torch.float64).reshape(_bshape(x, dim))
    y = dict(linear=lambda v: v, relu=torch.relu, lrelu=lambda v: F.leaky_relu(v, a), tanh=torch.tanh, sigmoid=torch.sigmoid,
             elu=F.elu, selu=lambda v: SELU_SCALE * torch.where(v >= 0, v, SELU_ALPHA * torch.expm1(v)), softplus=F.softplus,
             swish=lambda v: v * torch.sigmoid(v))[act](x)
    y = y * g
    return y if c < 0 else y.clamp(-c, c)


def bias_act_formulas(x, b=None, dim=1, act='linear', alpha=None, gain=None, clamp=None, order=0, xref=None, yref=None, dy=None,
                      dtype=torch.float32):
    """The reference kernel's formulas in `dtype` arithmetic.  order 0: y from x.  order 1: x is the incoming gradient, `xref` /
    `yref` the saved input / output.  order 2: x is the incoming second-order gradient, `dy` the first-order one.  The bias is
    added to x at order 0 and to xref otherwise."""
    a, g, c = scalars(act, alpha, gain, clamp)
    cv = lambda v: torch.tensor(v, dtype=dtype, device=x.device)                            # noqa: E731
    alpha_t, gain_t = cv(a), cv(g)
    one, two, big, half_big = cv(1.0), cv(2.0), cv(80.0), cv(40.0)
    ss, sa = cv(SELU_SCALE), cv(SELU_ALPHA)
    zero = torch.zeros([], dtype=dtype, device=x.device)
    x = x.to(dtype)
    bb = None if b is None else b.to(dtype).reshape(_bshape(x, dim))
    xr = None if xref is None else xref.to(dtype)
    if bb is not None:
        if order == 0:
            x = x + bb
        elif xr is not None:
            xr = xr + bb
    yr = None if yref is None else yref.to(dtype)
    yy = None if yr is None else (yr / gain_t if g != 0 else torch.zeros_like(yr))
    d1 = one if dy is None else dy.to(dtype)
    G = order
    if act == 'linear':
        y = x if G <= 1 else torch.zeros_like(x)
    elif act == 'relu':
        y = torch.where(x > 0, x, zero) if G == 0 else (torch.where(yy > 0, x, zero) if G == 1 else torch.zeros_like(x))
    elif act == 'lrelu':
        y = torch.where(x > 0, x, x * alpha_t) if G == 0 else (torch.where(yy > 0, x, x * alpha_t) if G == 1 else torch.zeros_like(x))
    elif act == 'tanh':
        if G == 0:
            e = torch.exp(x); d = one / e
            y = torch.where(x < -big, -one, torch.where(x > big, one, (e - d) / (e + d)))
        else:
            t = x * (one - yy * yy)
            y = t if G == 1 else t * (-two * yy)
    elif act == 'sigmoid':
        if G == 0:
            y = torch.where(x < -big, zero, one / (torch.exp(-x) + one))
        else:
            t = x * yy * (one - yy)
            y = t if G == 1 else t * (one - two * yy)
    elif act == 'elu':
        if G == 0:
            y = torch.where(x >= 0, x, torch.exp(x) - one)
        else:
            y = torch.where(yy >= 0, x if G == 1 else torch.zeros_like(x), x * (yy + one))
    elif act == 'selu':
        if G == 0:
            y = torch.where(x >= 0, ss * x, (ss * sa) * (torch.exp(x) - one))
        else:
            y = torch.where(yy >= 0, x * ss if G == 1 else torch.zeros_like(x), x * (yy + ss * sa))
    elif act == 'softplus':
        if G == 0:
            y = torch.where(x > big, x, torch.log(torch.exp(x) + one))
        else:
            e = torch.exp(-yy)
            y = x * (one - e) if G == 1 else x * e * (one - e)
    else:
        assert act == 'swish'
        if G == 0:
            y = torch.where(x < -big, zero, x / (torch.exp(-x) + one))
        else:
            e = torch.exp(xr); d = e + one
            if G == 1:
                y = torch.where(xr > half_big, x, x * e * (xr + d) / (d * d))
            else:
                y = torch.where(xr > half_big, zero, x * e * (xr * (two - d) + two * d) / (d * d * d))
            yr = torch.where(xr < -big, zero, xr / (torch.exp(-xr) + one) * gain_t)
    y = y * (gain_t * d1)
    if c >= 0:
        cl = cv(c)
        if G == 0:
            y = torch.where((y > -cl) & (y < cl), y, torch.where(y >= 0, cl, -cl))
        else:
            y = torch.where((yr > -cl) & (yr < cl), y, zero)
    return y


def bias_act_formulas32(*args, **kwargs):
    kwargs['dtype'] = torch.float32
    return bias_act_formulas(*args, **kwargs)


def bias_act_chain(x, b, dim, act, alpha, gain, clamp, w, v1, v2, dtype=torch.float32, store=None):
    """(y, gx, gb, ggx) of  L1 = sum(y w),  L2 = sum(gx v1) + sum(gb v2)  from the formulas in `dtype` arithmetic: gx = order 1 on w,
    gb its sum over every axis but `dim`, ggx = order 2 on v1 + v2[dim] with dy = w.  `store`: the tensor type every intermediate is
    rounded to, as the op stores it (fp16 tensors); sums accumulate in `dtype`."""
    st = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)          # noqa: E731
    kw = dict(b=b, dim=dim, act=act, alpha=alpha, gain=gain, clamp=clamp, dtype=dtype)
    y = st(bias_act_formulas(x, order=0, **kw))
    if act == 'linear':
        assert clamp is None                       # the op keeps no output for `linear`: its gradient cannot see a clamp
    gx = st(bias_act_formulas(w, order=1, xref=x, yref=y, **kw))
    axes = [i for i in range(x.ndim) if i != dim]
    gb = st(gx.sum(axes))
    ddx = st(v1.to(dtype) + v2.to(dtype).reshape(_bshape(x, dim)))
    ggx = st(bias_act_formulas(ddx, order=2, xref=x, yref=y, dy=w, **kw))
    return y, gx, gb, ggx


def bias_act_chain_def(x, b, dim, act, alpha, gain, clamp, w, v1, v2):
    """The same four quantities from `bias_act_def` and float64 autograd."""
    x = x.detach().to(torch.float64).requires_grad_(True)
    b = b.detach().to(torch.float64).requires_grad_(True)
    y = bias_act_def(x, b, dim, act, alpha, gain, clamp)
    gx, gb = torch.autograd.grad((y * w.to(torch.float64)).sum(), [x, b], create_graph=True)
    l2 = (gx * v1.to(torch.float64)).sum() + (gb * v2.to(torch.float64)).sum()
    if l2.requires_grad:
        ggx, = torch.autograd.grad(l2, [x], allow_unused=True)
    else:
        ggx = None
    ggx = torch.zeros_like(x) if ggx is None else ggx
    return y.detach(), gx.detach(), gb.detach(), ggx.detach()


def clamp_window(y64, clamp, dtype):
    """Elements whose clamp mask the tensor type's rounding of y may change: | |y64| - clamp | within 8 * 2^-24 clamp (fp32) or
    1.25 * 2^-11 clamp (fp16).  None for float64 or without a clamp."""
    if clamp is None or dtype == torch.float64:
        return torch.zeros_like(y64, dtype=torch.bool)
    c = f32(clamp)
    win = (8 * U32 if dtype == torch.float32 else 1.25 * F16_REL) * c
    return (y64.abs() - c).abs() <= win


# -------------------------------------------------------------------------------------------------------- filtered_lrelu_act_

def act_ref(x, gain, slope, clamp, dtype):
    """v = x * gain; where v < 0, v * slope; clamp -- each one operation in `dtype` (the accumulate type)."""
    g, s = torch.tensor(f32(gain), dtype=dtype, device=x.device), torch.tensor(f32(slope), dtype=dtype, device=x.device)
    v = x.to(dtype) * g
    v = torch.where(v < 0, v * s, v)
    if clamp is not None and not math.isinf(clamp):
        c = torch.tensor(f32(clamp), dtype=dtype, device=x.device)
        v = torch.where(v.abs() > c, torch.where(v < 0, -c, c), v)
    return v


def act_codes(x, gain, slope, clamp, dtype):
    """uint8 codes of the same decisions: 1 negative, 2 clamped (clamped wins)."""
    g, s = torch.tensor(f32(gain), dtype=dtype, device=x.device), torch.tensor(f32(slope), dtype=dtype, device=x.device)
    v = x.to(dtype) * g
    neg = v < 0
    v = torch.where(neg, v * s, v)
    code = neg.to(torch.uint8)
    if clamp is not None and not math.isinf(clamp):
        code = torch.where(v.abs() > f32(clamp), torch.full_like(code, 2), code)
    return code


def act_read_ref(x, codes_at, gain, slope, dtype):
    """Read mode: x * gain, times slope where the code has bit 0, zero where it has bit 1; `codes_at` holds the code that applies to
    each element of x, 255 where the sample falls outside the sign tensor (only scaled by the gain)."""
    g, s = torch.tensor(f32(gain), dtype=dtype, device=x.device), torch.tensor(f32(slope), dtype=dtype, device=x.device)
    v = x.to(dtype) * g
    inside = codes_at != 255
    v = torch.where(inside & ((codes_at & 1) != 0), v * s, v)
    return torch.where(inside & ((codes_at & 2) != 0), torch.zeros_like(v), v)


# ------------------------------------------------------------------------------------------------------------------ the cases
# (shared by tests/test_generic_ops_ref_cpu.py and tests/test_gpu_generic_ops_fp64.py; inputs are regenerated from seeds)

MAGNITUDES = (1e-3, 1.0, 30.0)

# name: (shape of the dense tensor, how x is viewed, bias dim, axis along which the magnitude groups alternate)
BIAS_ACT_SHAPES = {
    'rows_dim1':     ((1031, 1019), 'plain', 1, 0),              # 1 050 589 elements: three passes for the first threads, ragged tail
    'rows_dim0':     ((1031, 1019), 'plain', 0, 1),
    'channels_last': ((3, 37, 97, 101), 'channels_last', 1, 2),  # stepB = 1
    'permuted':      ((5, 211, 997), 'permute021', 2, 1),        # a permute(0, 2, 1) view: [5, 997, 211], bias along the 211 (stepB = 997)
}
BIAS_ACT_GAINS = (None, 1.7)
BIAS_ACT_CLAMP = 0.5
BIAS_ACT_ALPHA = 0.2


def view_as(t, how):
    if how == 'channels_last':
        return t.contiguous(memory_format=torch.channels_last)
    if how == 'permute021':
        return t.permute(0, 2, 1)
    return t


def bias_act_inputs(name, seed=0):
    """(x, b, w, v1, v2, group index) as float32 CPU tensors in the logical (viewed) shape; x = N(0, 1) * magnitude of its group,
    b = 0.5 N(0, 1), the cotangents N(0, 1)."""
    shape, how, dim, gaxis = BIAS_ACT_SHAPES[name]
    r = np.random.RandomState(1000 + seed)
    mk = lambda: view_as(torch.from_numpy(r.randn(*shape).astype(np.float32)), how)         # noqa: E731
    x, w, v1 = mk(), mk(), mk()
    b = torch.from_numpy((0.5 * r.randn(x.shape[dim])).astype(np.float32))
    v2 = torch.from_numpy(r.randn(x.shape[dim]).astype(np.float32))
    gidx = (torch.arange(x.shape[gaxis]) % 3).reshape([-1 if i == gaxis else 1 for i in range(x.ndim)]).expand(x.shape)
    x = x * torch.tensor(MAGNITUDES, dtype=torch.float32)[gidx]
    return x, b, w, v1, v2, gidx


# name: dict(shape, f (golden_cases.make_filter spec), up, down, padding, flips, gains, layout)
UPFIRDN_BIG_CASES = {
    'sep_up2':       dict(shape=(2, 3, 300, 301), f='kaiser:12:2.0:4.6:32', up=2, down=1, padding=[6, 5, 6, 5], flips=(False,), gains=(4.0, 1.7)),   # 2.17 M outputs
    'radial_dn2':    dict(shape=(1, 2, 1100, 1030), f='kaiser:12:2.8:5.2:32:radial', up=1, down=2, padding=0, flips=(False,), gains=(1.0,)),
    'asym_rational': dict(shape=(1, 2, 400, 420), f='asym2d:5:3', up=[2, 3], down=[3, 2], padding=[2, 1, -1, 3], flips=(True, False), gains=(1.7,)),
    'crop_only':     dict(shape=(1, 2, 700, 900), f=None, up=2, down=1, padding=[-2, -1, -3, 0], flips=(False,), gains=(1.0,)),
    'sep_up2_cl':    dict(shape=(2, 3, 300, 301), f='kaiser:12:2.0:4.6:32', up=2, down=1, padding=[6, 5, 6, 5], flips=(False,), gains=(1.7,), layout='channels_last'),
    'sep_up2_view':  dict(shape=(2, 3, 300, 301), f='kaiser:12:2.0:4.6:32', up=2, down=1, padding=[6, 5, 6, 5], flips=(False,), gains=(1.7,), layout='view'),
    'filter_larger': dict(shape=(1, 1, 3, 4), f='asym2d:9:7', up=1, down=1, padding=[4, 4, 3, 3], flips=(False, True), gains=(1.7,)),
    'skipped_taps':  dict(shape=(1, 1, 40, 40), f='asym:3', up=1, down=5, padding=0, flips=(False,), gains=(1.7,)),
    'filter_stride': dict(shape=(1, 2, 21, 23), f='asym2d:5:3', up=2, down=1, padding=[2, 1, 1, 2], flips=(False,), gains=(1.7,), layout='f_transposed'),
}


def upfirdn_input(name, seed=0):
    """x as float32 CPU tensor, dense [N,C,H,W] values; the test lays it out as the case says."""
    c = UPFIRDN_BIG_CASES[name]
    return torch.from_numpy(np.random.RandomState(2000 + seed).randn(*c['shape']).astype(np.float32))


# the generic filtered_lrelu composition: name -> dict(shape, fu, fd, up, down, padding, gain, slope, clamp, flips, dtypes)
SG2 = float(np.sqrt(2))
FLRELU_GENERIC_CASES = {
    'up1_dn2':     dict(shape=(2, 3, 300, 650), fu=None, fd='kaiser:12:4.0:8.0:64', up=1, down=2, padding=[5, 5, 5, 5], gain=SG2, slope=0.2, clamp=256,
                        flips=(False,), dtypes=('float32', 'float16', 'float64')),
    'up2_dn1':     dict(shape=(1, 2, 150, 330), fu='kaiser:12:2.0:4.6:32', fd=None, up=2, down=1, padding=[5, 6, 5, 6], gain=SG2, slope=0.2, clamp=256,
                        flips=(False,), dtypes=('float32', 'float16', 'float64')),
    'up3_dn2':     dict(shape=(1, 2, 90, 140), fu='asym:9', fd='asym:7', up=3, down=2, padding=[-3, 5, 2, -1], gain=SG2, slope=0.1, clamp=0.5,
                        flips=(True, False), dtypes=('float32', 'float16', 'float64')),
    'both_2d':     dict(shape=(1, 2, 60, 70), fu='asym2d:5:3', fd='asym2d:5:3', up=2, down=2, padding=[3, 2, 4, 3], gain=SG2, slope=0.2, clamp=1.0,
                        flips=(False,), dtypes=('float32', 'float16', 'float64')),
    't_up2_dn2':   dict(shape=(1, 2, 100, 140), fu='kaiser:12:2.0:4.6:32', fd='kaiser:12:2.8:5.2:32', up=2, down=2, padding=[9, 8, 9, 8], gain=SG2, slope=0.2,
                        clamp=256, flips=(False,), dtypes=('float64',)),
}


def flrelu_inputs(name, seed=0):
    c = FLRELU_GENERIC_CASES[name]
    r = np.random.RandomState(3000 + seed)
    return torch.from_numpy(r.randn(*c['shape']).astype(np.float32)), torch.from_numpy(r.randn(c['shape'][1]).astype(np.float32))
