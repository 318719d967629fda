"""GPU: the three generic operators -- bias_act, upfirdn2d, filtered_lrelu_act_ -- and the generic filtered_lrelu composition built
from them, against the float64 references of tests/generic_ops_ref.py and tests/flrelu_ref.py, at sizes that run more than one grid
pass (the stride loops, the 64-bit indices, the bias index), in fp32, fp16 and float64, in dense non-contiguous layouts.

Every float64 reference runs on the device.  Every test prints its worst error / bound ratio.
"""
import ctypes

import pytest
import torch

import flrelu_ref as R
import generic_ops_ref as G
from golden_cases import make_filter
from helpers import product_design

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = {'float32': torch.float32, 'float16': torch.float16, 'float64': torch.float64}
NONE = torch.empty([0])


def _f(spec):
    f = make_filter(spec, product_design)
    return None if f is None else torch.from_numpy(f).to(DEV)


def _mx(t, mask=None):
    if mask is not None:
        t = t[mask]
    return float(t.abs().max()) if t.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------ a. bias_act

# float64: |hip - def| <= n * 2^-53 * (|def| + |gain * cotangents|).  n counts the roundings of the formula chain from x to the result:
# one per IEEE operation, two per libm call (exp, log: within 1 ulp), and the roundings of the saved y once for every time y / gain
# enters the derivative's formula (every factor it enters is at most 2 in magnitude relative to the scale above):
#   linear    x + b, gain * dy, the product: 3                                                         -> 4
#   relu      the same                                                                                 -> 4
#   lrelu     + the slope                                                                              -> 5
#   tanh      y: add, exp 2, 1 / c, c - d, c + d, divide, gain = 8, y / gain 9; order 2 = x (1 - yy yy)(-2 yy) gain dy:
#             yy enters twice at weight one (the third time inside 1 - yy^2 <= 1 next to 2 yy (1 - yy^2) <= 0.77): 2 * 9 + 8 ops + 2
#   sigmoid   y: add, exp 2, + 1, divide, gain = 6, y / gain 7; order 2 = x yy (1 - yy)(1 - 2 yy) gain dy: 3 * 7 + 5 ops
#   elu       y: add, exp 2, - 1, gain = 5; orders 1, 2 = x (yy + 1) gain dy: y / gain 6 + 4 ops
#   selu      as elu with the two constants' products in y and in the derivative: + 4
#   softplus  y: add, exp 2, + 1, log 2, gain = 7, y / gain 8; order 2 = x c (1 - c) gain dy, c = exp(-yy) 2: c enters twice:
#             2 * (8 + 2) + 4 ops
#   swish     order 2 = x c (xr (2 - d) + 2 d) / (d d d) gain dy on c = exp(xr) (add, exp 2), d = c + 1: c once 3, d four times
#             at 4 each, the bracket 4 ops, products and quotient 6, gain dy 2: 3 + 16 + 4 + 6 + 2
# Measured worst ratio 0.25 (selu, second order).
N64 = dict(linear=4, relu=4, lrelu=5, tanh=28, sigmoid=26, elu=10, selu=14, softplus=24, swish=31)
assert max(N64.values()) <= 32


def _op_chain(x, b, dim, act, gain, clamp, w, v1, v2, impl='cuda'):
    """(y, gx, gb, ggx) through the public op: L1 = <y, w>, L2 = <gx, v1> + <gb, v2>, create_graph=True.  The cotangents are given
    instead of the squares of test_bias_act_gradients: each result is then one kernel applied to known inputs, and fp16's gb (a sum
    over up to 29 391 elements) stays inside fp16's range."""
    from torch_utils.ops import bias_act
    x = x.detach().requires_grad_(True)
    b = b.detach().requires_grad_(True)
    y = bias_act.bias_act(x, b, dim=dim, act=act, alpha=G.BIAS_ACT_ALPHA, gain=gain, clamp=clamp, impl=impl)
    gx, gb = torch.autograd.grad([y], [x, b], grad_outputs=[w], create_graph=True)
    ggx = None
    outs = [(t, v) for t, v in ((gx, v1), (gb, v2)) if t.requires_grad]
    if outs:
        ggx, = torch.autograd.grad([t for t, _ in outs], [x], grad_outputs=[v for _, v in outs], allow_unused=True)
    ggx = torch.zeros_like(x) if ggx is None else ggx
    return y.detach(), gx.detach(), gb.detach(), ggx.detach()


def _free(x, b, dim, act, gain, w):
    """float64 output and first derivative (times w) of the unclamped definition."""
    x64 = x.detach().double().requires_grad_(True)
    y = G.bias_act_def(x64, b.double(), dim, act, G.BIAS_ACT_ALPHA, gain, None)
    gx, = torch.autograd.grad([y], [x64], grad_outputs=[w.double()])
    return y.detach(), gx


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('shape', sorted(G.BIAS_ACT_SHAPES))
def test_bias_act_all_activations_and_orders(shape, dtype):
    """Forward, gx, gb and ggx of all nine activations, default gain and 1.7, clamp 0.5 (linear unclamped, and forward-only clamped),
    per magnitude group (x = N(0, 1) * 1e-3 | 1 | 30 in turn).

    fp32 / fp16:  e_hip <= 2 e_formulas32 + floor * max|ref| in max-abs norm, per group; floor 1e-7 (fp32), 2^-11 (fp16, the yardstick
    being the fp32 formulas on the fp16-rounded inputs, every stored tensor rounded to fp16).  Elements whose unclamped |y64| lies
    within 8 * 2^-24 clamp (fp32) / 1.25 * 2^-11 clamp (fp16) of the clamp are left out of gx and ggx (their share is asserted from the
    reference); gb cannot leave them out, so its bound grows by the sum of |gain * w * act'| over those elements of each bias slot:
    what one flipped mask bit changes.  float64: N64 above, nothing left out."""
    dt = DTYPES[dtype]
    _, how, dim, _ = G.BIAS_ACT_SHAPES[shape]
    x, b, w, v1, v2, gidx = G.bias_act_inputs(shape)
    strides = x.stride()
    x, b, w, v1, v2 = (t.to(DEV).to(dt) for t in (x, b, w, v1, v2))
    gidx = gidx.to(DEV)
    assert x.stride() == strides and w.stride() == strides            # the layout under test reached the device
    axes = [i for i in range(x.ndim) if i != dim]
    floor = 2.0 ** -11 if dt == torch.float16 else 1e-7
    cap = {torch.float32: 1e-4, torch.float16: 2e-3, torch.float64: 0.0}[dt]
    table, failed = [], []
    for act in G.ACTS:
        for gain in G.BIAS_ACT_GAINS:
            clamp = None if act == 'linear' else G.BIAS_ACT_CLAMP
            _, g, _ = G.scalars(act, G.BIAS_ACT_ALPHA, gain, clamp)
            hip = _op_chain(x, b, dim, act, gain, clamp, w, v1, v2)
            ref = G.bias_act_chain_def(x, b, dim, act, G.BIAS_ACT_ALPHA, gain, clamp, w, v1, v2)
            names = ('y', 'gx', 'gb', 'ggx')
            if dt == torch.float64:
                cot = dict(y=torch.ones_like(ref[0]), gx=w.abs(), ggx=(w * (v1 + v2.reshape(G._bshape(x, dim)))).abs())
                for nm, h, r in zip(names, hip, ref):
                    if nm == 'gb':
                        eb = N64[act] * G.U64 * (ref[1].abs() + g * cot['gx'])
                        bound = eb.sum(axes) + x.numel() // b.numel() * G.U64 * ref[1].abs().sum(axes)
                    else:
                        bound = N64[act] * G.U64 * (r.abs() + g * cot[nm])
                    ratio = G.ratio((h - r).abs(), bound)
                    table.append((act, gain, nm, 'all', ratio))
                    if ratio > 1.0:
                        failed.append((act, gain, nm, ratio))
                continue
            yard = G.bias_act_chain(x, b, dim, act, G.BIAS_ACT_ALPHA, gain, clamp, w, v1, v2, dtype=torch.float32,
                                    store=torch.float16 if dt == torch.float16 else None)
            tor = _op_chain(x.float(), b.float(), dim, act, gain, clamp, w.float(), v1.float(), v2.float(), impl='ref') if dt == torch.float32 else None
            if clamp is None:
                window, wid = torch.zeros(x.shape, dtype=torch.bool, device=DEV), 0.0
            else:
                y_free, gx_free = _free(x, b, dim, act, gain, w)
                window = G.clamp_window(y_free, clamp, dt)
                share = float(window.double().mean())
                assert share <= cap, (act, gain, share)
                wid = (gx_free.abs() * window).sum(axes)
            for k, (nm, h, r, f) in enumerate(zip(names, hip, ref, yard)):
                t = None if tor is None else tor[k]
                if nm == 'gb':
                    # gb is torch's sum of the kernel's gx.  The kernel answers for the sum of its gx taken exactly (in float64: a
                    # bias of gx that no max-abs norm sees shows here), under the same bound against the yardstick's gx summed
                    # exactly -- with the definition's gx inside the window, so that a mask flip of the yardstick's own does not
                    # loosen it.  The op's sum itself: any order of an fp32 accumulation stays within (count - 1) u sum|gx|.
                    hx = hip[1].double().sum(axes)
                    fx = torch.where(window, ref[1], yard[1].double()).sum(axes)
                    e_f = _mx(fx - r)
                    err = (hx - r).abs()
                    ratio = G.ratio(err, 2 * e_f + floor * _mx(r) + wid + torch.zeros_like(err))
                    sb = (x.numel() // b.numel() - 1) * G.U32 * hip[1].double().abs().sum(axes)
                    if dt == torch.float16:
                        sb = sb + G.F16_REL * (hx.abs() + sb) + G.F16_SUB
                    ratio = max(ratio, G.ratio((h.double() - hx).abs(), sb))
                    table.append((act, gain, nm, 'all', _mx(err), e_f, None if t is None else _mx(t.double() - r), ratio))
                    if ratio > 1.0:
                        failed.append((act, gain, nm, ratio))
                    continue
                for grp in range(3):
                    m = gidx == grp
                    if nm != 'y':
                        m = m & ~window
                    e_h, e_f = _mx(h.double() - r, m), _mx(f.double() - r, m)
                    bound = 2 * e_f + floor * _mx(r, m)
                    ratio = 0.0 if e_h == 0.0 else e_h / bound
                    table.append((act, gain, nm, G.MAGNITUDES[grp], e_h, e_f, None if t is None else _mx(t.double() - r, m), ratio))
                    if ratio > 1.0:
                        failed.append((act, gain, nm, G.MAGNITUDES[grp], e_h, e_f))
        # linear with a clamp: forward only (the op keeps no output for it, so its gradient cannot see the clamp)
        if act == 'linear':
            from torch_utils.ops import bias_act
            h = bias_act.bias_act(x, b, dim=dim, act=act, gain=1.7, clamp=G.BIAS_ACT_CLAMP)
            r = G.bias_act_def(x, b, dim, act, None, 1.7, G.BIAS_ACT_CLAMP)
            if dt == torch.float64:
                ratio = G.ratio((h - r).abs(), N64[act] * G.U64 * (r.abs() + G.f32(1.7)))
            else:
                f = G.bias_act_formulas32(x, b, dim, act, None, 1.7, G.BIAS_ACT_CLAMP)
                f = f.to(dt) if dt == torch.float16 else f
                ratio = max(_mx(h.double() - r, gidx == k) / (2 * _mx(f.double() - r, gidx == k) + floor * _mx(r, gidx == k)) for k in range(3))
            table.append((act, 1.7, 'y clamped', 'all', ratio))
            if ratio > 1.0:
                failed.append((act, 'clamped forward', ratio))
    print(f'bias_act {shape} {dtype}: act, gain, quantity, group, [e_hip, e_formulas32, e_torch32,] err/bound')
    for row in table:
        print('   ', '  '.join(f'{v:.3e}' if isinstance(v, float) else str(v) for v in row))
    assert not failed, failed


@pytest.mark.parametrize('order', [0, 1, 2])
def test_bias_act_plugin_honours_the_bias_step_of_a_permuted_view(order):
    """The kernel on the permute(0, 2, 1) view itself (stepB = 997; the public op copies a rank-3 view first) equals, bit for bit, the
    kernel on its contiguous copy, for every order and type."""
    from torch_utils.ops import bias_act
    bias_act._init()
    P = bias_act._plugin
    x, b, w, v1, _, _ = G.bias_act_inputs('permuted')
    for dt in DTYPES.values():
        xv, bv, wv, vv = (t.to(DEV).to(dt) for t in (x, b, w, v1))
        assert xv.stride(2) == 997 and not xv.is_contiguous()
        for act, idx in (('lrelu', 3), ('tanh', 4), ('swish', 9)):
            def run(conv):
                y = P.bias_act(conv(xv), bv, NONE, NONE, NONE, 0, 2, idx, 0.2, 1.7, 0.5)
                if order == 0:
                    return y
                if order == 1:
                    return P.bias_act(conv(wv), bv, conv(xv), y, NONE, 1, 2, idx, 0.2, 1.7, 0.5)
                return P.bias_act(conv(vv), bv, conv(xv), y, conv(wv), 2, 2, idx, 0.2, 1.7, 0.5)
            a, c = run(lambda t: t), run(lambda t: t.contiguous())
            assert a.stride() == xv.stride() and c.is_contiguous()
            assert torch.equal(a, c), (dt, act, order)


@pytest.mark.parametrize('act', G.ACTS)
def test_bias_act_special_values(act):
    """fp32, b = 0: +-0, +-80, +-81 (the exp cut-offs), +-40, 41 (swish's derivative cut-off), +-1e-30, +-65504 through all three
    orders, against the formulas evaluated in float64 with the kernel's conventions at the kinks:
    8 * 2^-24 * (|ref| + |gain|)."""
    vals = [0.0, -0.0, 80.0, -80.0, 81.0, -81.0, 40.0, -40.0, 41.0, 1e-30, -1e-30, 65504.0, -65504.0]
    x = torch.tensor(vals, dtype=torch.float32, device=DEV).reshape(1, -1)
    b = torch.zeros([len(vals)], dtype=torch.float32, device=DEV)
    one = torch.ones_like(x)
    worst = 0.0
    for gain in G.BIAS_ACT_GAINS:
        for clamp in ((None,) if act == 'linear' else (None, G.BIAS_ACT_CLAMP)):
            _, g, _ = G.scalars(act, G.BIAS_ACT_ALPHA, gain, clamp)
            hip = _op_chain(x, b, 1, act, gain, clamp, one, one, torch.zeros_like(b))
            ref = G.bias_act_chain(x, b, 1, act, G.BIAS_ACT_ALPHA, gain, clamp, one, one, torch.zeros_like(b), dtype=torch.float64)
            for nm, h, r in zip(('y', 'gx', 'gb', 'ggx'), hip, ref):
                assert bool(torch.isfinite(h).all()), (act, gain, clamp, nm, h)
                if nm != 'gb':
                    worst = max(worst, G.ratio((h.double() - r).abs(), 8 * G.U32 * (r.abs() + g)))
    print(f'bias_act special values {act}: worst err/bound {worst:.3f}')
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------- b. upfirdn2d

def _upfirdn_abi(x, f, y, up, down, padding, flip, gain):
    """sg3_upfirdn2d straight through the C ABI, writing into the given (possibly strided) y."""
    from torch_utils import _sg3abi as abi
    upx, upy = G._xy(up); downx, downy = G._xy(down); px0, _, py0, _ = G._four(padding)
    p = abi.Upfirdn2dParams()
    p.x, p.f, p.y = abi.ptr(x), abi.ptr(f), abi.ptr(y)
    p.dtype = abi.dtype_code(x.dtype)
    p.N, p.C, p.xH, p.xW, p.yH, p.yW = (int(v) for v in (*x.shape, *y.shape[2:]))
    p.xStride, p.yStride = abi.strides4(x), abi.strides4(y)
    p.fH, p.fW = int(f.shape[0]), int(f.shape[1])
    p.fStride = (ctypes.c_int64 * 2)(int(f.stride(0)), int(f.stride(1)))
    p.upx, p.upy, p.downx, p.downy, p.padx0, p.pady0 = upx, upy, downx, downy, px0, py0
    p.flip, p.gain = int(bool(flip)), float(gain)
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_upfirdn2d(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_upfirdn2d')


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('name', sorted(G.UPFIRDN_BIG_CASES))
def test_upfirdn2d_forward_and_adjoint(name, dtype):
    """Forward and x.grad through the public op against `upfirdn_ref` under `upfirdn_bound` (the adjoint under the bound of its own
    geometry), element by element."""
    from torch_utils.ops import upfirdn2d
    dt = DTYPES[dtype]
    c = G.UPFIRDN_BIG_CASES[name]
    layout = c.get('layout')
    x = G.upfirdn_input(name).to(DEV).to(dt)
    f = _f(c['f'])
    f_ref = f
    guard = 12345.0
    if layout == 'channels_last':
        x = x.contiguous(memory_format=torch.channels_last)
    elif layout == 'view':
        big = torch.full([x.shape[0], x.shape[1], x.shape[2] + 1, x.shape[3] + 2], guard, dtype=dt, device=DEV)
        big[:, :, 1:, 1:-1] = x
        x = big[:, :, 1:, 1:-1]
        assert not x.is_contiguous() and x.stride(2) == x.shape[3] + 2
    elif layout == 'f_transposed':
        f_ref = f.t().contiguous()
        f = f.t()
        assert f.stride() == (1, f.shape[0]) and tuple(f.shape) == tuple(f_ref.shape)
    gen = torch.Generator(device=DEV).manual_seed(11)
    worst = {}
    for flip in c['flips']:
        for gain in c['gains']:
            kw = dict(up=c['up'], down=c['down'], padding=c['padding'], flip=flip, gain=gain)
            xs = x.detach().requires_grad_(True)
            y = upfirdn2d.upfirdn2d(xs, f, up=c['up'], down=c['down'], padding=c['padding'], flip_filter=flip, gain=gain)
            assert y.dtype == dt
            ref = G.upfirdn_ref(x, f_ref, **kw)
            assert tuple(y.shape) == tuple(ref.shape)
            r = G.ratio((y.detach().double() - ref).abs(), G.upfirdn_bound(x, f_ref, dtype=dt, ref=ref, **kw))
            gy = torch.randn(y.shape, device=DEV, generator=gen).to(dt)
            y.backward(gy)
            aup, adown, apad, aflip = G.adjoint_geometry(tuple(x.shape[2:]), tuple(y.shape[2:]), f_ref, c['up'], c['down'], c['padding'], flip)
            akw = dict(up=aup, down=adown, padding=apad, flip=aflip, gain=gain)
            adj = G.upfirdn_ref(gy, f_ref, **akw)
            assert xs.grad.dtype == dt and tuple(adj.shape) == tuple(x.shape)
            ra = G.ratio((xs.grad.double() - adj).abs(), G.upfirdn_bound(gy, f_ref, dtype=dt, ref=adj, **akw))
            worst[(flip, gain)] = (r, ra)
            if layout == 'view':
                # the input's guard frame is untouched, and the kernel writing into a framed output leaves that frame alone
                assert bool((big[:, :, 0] == guard).all()) and bool((big[:, :, :, 0] == guard).all()) and bool((big[:, :, :, -1] == guard).all())
                f2 = f[None, :] if f.ndim == 1 else f
                if f.ndim == 1:                        # the row pass of the separable call, as the op issues it
                    frame = torch.full([y.shape[0], y.shape[1], x.shape[2] + 2, y.shape[3] + 3], guard, dtype=dt, device=DEV)
                    out = frame[:, :, 1:-1, 2:-1]
                    _upfirdn_abi(x, f2, out, [G._xy(c['up'])[0], 1], [G._xy(c['down'])[0], 1], [c['padding'][0], c['padding'][1], 0, 0], flip, 1.0)
                    inner = torch.zeros_like(frame, dtype=torch.bool)
                    inner[:, :, 1:-1, 2:-1] = True
                    assert bool((frame[~inner] == guard).all())
                    want = G.upfirdn_ref(x, f2, up=[G._xy(c['up'])[0], 1], down=[G._xy(c['down'])[0], 1], padding=[c['padding'][0], c['padding'][1], 0, 0],
                                         flip=flip, gain=1.0)
                    bnd = G.upfirdn_bound(x, f2, up=[G._xy(c['up'])[0], 1], down=[G._xy(c['down'])[0], 1], padding=[c['padding'][0], c['padding'][1], 0, 0],
                                          flip=flip, gain=1.0, dtype=dt, ref=want)
                    worst[('framed row pass', gain)] = (G.ratio((out.double() - want).abs(), bnd), 0.0)
    print(f'upfirdn2d {name} {dtype} {tuple(x.shape)} -> {tuple(y.shape)}: worst err/bound (forward, adjoint) per (flip, gain): '
          + '  '.join(f'{k}: {v[0]:.3f} {v[1]:.3f}' for k, v in worst.items()))
    assert max(max(v) for v in worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------- c. filtered_lrelu_act_

GUARD_BYTES = 64
GUARD = 0xA5


def _act_abi(x, s, sx, sy, gain, slope, clamp, write, read):
    """sg3_filtered_lrelu_act straight through the C ABI: x in place, s a uint8 [N,C,sH,sW/4] tensor (or None)."""
    from torch_utils import _sg3abi as abi
    p = abi.FilteredLreluActParams()
    p.x = abi.ptr(x)
    p.s = abi.ptr(s) if s is not None else None
    p.dtype = abi.dtype_code(x.dtype)
    p.N, p.C, p.H, p.W = (int(v) for v in x.shape)
    p.xStride = abi.strides4(x)
    p.sH, p.sW = (int(s.shape[2]), int(s.shape[3]) * 4) if s is not None else (0, 0)
    p.sx, p.sy = int(sx), int(sy)
    p.gain, p.slope, p.clamp = float(gain), float(slope), float(clamp)
    p.writeSigns, p.readSigns = int(write), int(read)
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_filtered_lrelu_act(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_filtered_lrelu_act')


def _guarded_signs(n, c, sh, swb):
    """(whole buffer, the [n, c, sh, swb] sign tensor inside it) with GUARD_BYTES of GUARD on either side."""
    size = n * c * sh * swb
    buf = torch.full([size + 2 * GUARD_BYTES], GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD_BYTES:GUARD_BYTES + size].view(n, c, sh, swb)


def _guards_intact(buf):
    return bool((buf[:GUARD_BYTES] == GUARD).all()) and bool((buf[-GUARD_BYTES:] == GUARD).all())


def _pack(codes):
    """[N,C,sH,sW] codes (0 .. 3) -> the byte tensor [N,C,sH,sW/4], the first column of four in the lowest bits."""
    n, c, sh, sw = codes.shape
    q = codes.reshape(n, c, sh, sw // 4, 4).to(torch.int32)
    return (q[..., 0] | (q[..., 1] << 2) | (q[..., 2] << 4) | (q[..., 3] << 6)).to(torch.uint8)


ACT_SHAPES = {
    'three_x_blocks': ((2, 3, 9, 661), False),             # three x blocks, W no multiple of 4
    'plane_loop':     ((70001, 1, 2, 5), False),           # more planes than grid z
    'row_loop':       ((1, 1, 65600, 5), False),           # more rows than grid y
    'channels_last':  ((2, 5, 33, 300), True),
}
ACT_ARGS = (1.5, 0.2, 1.0)                                 # gain, slope, clamp


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('name', sorted(ACT_SHAPES))
def test_filtered_lrelu_act_write_and_plain(name, dtype):
    """Write and plain mode: values bit-equal to `act_ref` in the accumulate type (rounded once for fp16 tensors), codes equal to
    `act_codes`, the padding bits of each sign row zero, the bytes around the sign buffer untouched."""
    dt = DTYPES[dtype]
    acc = torch.float64 if dt == torch.float64 else torch.float32
    shape, cl = ACT_SHAPES[name]
    n, c, h, w = shape
    gen = torch.Generator(device=DEV).manual_seed(3)
    x0 = (torch.randn(shape, device=DEV, generator=gen) * 2).to(dt)
    if cl:
        x0 = x0.contiguous(memory_format=torch.channels_last)
    want = G.act_ref(x0, *ACT_ARGS, acc).to(dt)
    codes = G.act_codes(x0, *ACT_ARGS, acc)
    assert 0.02 < float((codes == 2).double().mean()) < 0.9 and 0.02 < float((codes == 1).double().mean())
    # plain
    x = x0.clone()
    assert x.stride() == x0.stride()
    _act_abi(x, None, 0, 0, *ACT_ARGS, False, False)
    assert torch.equal(x, want)
    # write
    swb = ((w + 15) & ~15) // 4
    buf, s = _guarded_signs(n, c, h, swb)
    x = x0.clone()
    _act_abi(x, s, 0, 0, *ACT_ARGS, True, False)
    assert torch.equal(x, want)
    assert _guards_intact(buf)
    got = R.decode_signs(s, 0, 0, (h, swb * 4))
    assert torch.equal(got[..., :w], codes)
    assert bool((got[..., w:] == 0).all())                                   # padding bits beyond W
    # the binding's own call allocates the same tensor
    from torch_utils.ops import filtered_lrelu
    filtered_lrelu._init()
    x = x0.clone()
    so = filtered_lrelu._plugin.filtered_lrelu_act_(x, NONE, 0, 0, *ACT_ARGS, True)
    assert torch.equal(so, s) and torch.equal(x, want)


@pytest.mark.parametrize('dtype', sorted(DTYPES))
@pytest.mark.parametrize('name,sign_hw', [('three_x_blocks', (7, 640)), ('three_x_blocks', (12, 672)), ('channels_last', (30, 304)),
                                          ('plane_loop', (3, 16)), ('row_loop', (65601, 16))])
def test_filtered_lrelu_act_read(name, sign_hw, dtype):
    """Read mode with offsets (0, 0), (3, 2), (-5, -1) and a sign tensor smaller / larger than x: bit-equal to x * gain, times slope
    under code bit 0, zero under bit 1; samples that fall outside the sign tensor are only scaled by the gain."""
    dt = DTYPES[dtype]
    acc = torch.float64 if dt == torch.float64 else torch.float32
    shape, cl = ACT_SHAPES[name]
    n, c, h, w = shape
    sh, sw = sign_hw
    gen = torch.Generator(device=DEV).manual_seed(4)
    x0 = (torch.randn(shape, device=DEV, generator=gen) * 2).to(dt)
    if cl:
        x0 = x0.contiguous(memory_format=torch.channels_last)
    codes = torch.randint(0, 4, [n, c, sh, sw], device=DEV, generator=gen, dtype=torch.uint8)
    buf, s = _guarded_signs(n, c, sh, sw // 4)
    s.copy_(_pack(codes))
    before = buf.clone()
    for sx, sy in ((0, 0), (3, 2), (-5, -1)):
        at = R.decode_signs(s, sx, sy, (h, w))
        outside = float((at == 255).double().mean())
        if sx < 0 or sh < h or sw < w:
            assert outside > 0
        want = G.act_read_ref(x0, at, ACT_ARGS[0], ACT_ARGS[1], acc).to(dt)
        x = x0.clone()
        _act_abi(x, s, sx, sy, *ACT_ARGS, False, True)
        assert torch.equal(x, want), (sx, sy, float((x.double() - want.double()).abs().max()))
        assert torch.equal(buf, before)                                      # read mode writes no sign byte


# ---------------------------------------------------------------------------------------------- d. the generic composition

def _filter_dims(f):
    return (1, 1) if f is None else ((int(f.shape[1]), int(f.shape[0])) if f.ndim == 2 else (int(f.shape[0]), 0))


def _no_fused_kernel(c, fu, fd):
    from torch_utils import _sg3abi
    lib = _sg3abi.load()
    return (lib.sg3_filtered_lrelu_has_kernel(c['up'], c['down'], *_filter_dims(fu), *_filter_dims(fd)) == 0
            and lib.sg3_filtered_lrelu_has_kernel(c['down'], c['up'], *_filter_dims(fd), *_filter_dims(fu)) == 0)


def _flrelu(c, x, b, fu, fd, flip):
    from torch_utils.ops import filtered_lrelu as fl
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return fl.filtered_lrelu(x, fu=fu, fd=fd, b=b, up=c['up'], down=c['down'], padding=c['padding'], gain=c['gain'], slope=c['slope'],
                                 clamp=c['clamp'], flip_filter=flip)


@pytest.mark.parametrize('name,dtype', [(n, d) for n in sorted(G.FLRELU_GENERIC_CASES) for d in G.FLRELU_GENERIC_CASES[n]['dtypes']])
def test_generic_filtered_lrelu_composition(name, dtype):
    """y, sign codes, dx and db of configurations the fused kernels refuse (and of float64) against `flrelu_ref` with the generic
    counts.  Ambiguous samples widen the bound of dx; nothing is excluded; the widened share is at most 1e-3.
    fp16 tensors: the composition stores u in fp16 before the activation reads it, so 2^-11 of every sample's scale would be ambiguous
    against the float64 u (3e-3 of the samples, a quarter of dx widened).  Instead the stored tensor itself is reproduced by the up
    pass's own call and held to the float64 u; the codes must equal the fp32 decisions on it everywhere, and the adjoint's mask is
    the float64 decision on that tensor (ambiguous only within fp32 rounding of the clamp)."""
    dt = DTYPES[dtype]
    fp16 = dt == torch.float16
    unit = G.unit(dt)
    c = G.FLRELU_GENERIC_CASES[name]
    fu, fd = _f(c['fu']), _f(c['fd'])
    assert dt == torch.float64 or _no_fused_kernel(c, fu, fd)
    x0, b0 = (t.to(DEV).to(dt) for t in G.flrelu_inputs(name))
    gen = torch.Generator(device=DEV).manual_seed(21)
    worst = {}
    for flip in c['flips']:
        kw = dict(up=c['up'], down=c['down'], padding=c['padding'], gain=c['gain'], slope=c['slope'], clamp=c['clamp'], flip=flip)
        x = x0.clone().requires_grad_(True); b = b0.clone().requires_grad_(True)
        y = _flrelu(c, x, b, fu, fd, flip)
        signs = y.grad_fn.saved_tensors[2]
        assert y.dtype == dt and signs.dtype == torch.uint8 and signs.numel() > 0
        gy = torch.randn(y.shape, device=DEV, generator=gen).to(dt)
        y.backward(gy)
        xhw = tuple(x.shape[2:])
        y64, u64 = R.forward_ref(x0, b0, fu, fd, **kw)
        assert tuple(y.shape) == tuple(y64.shape)
        scales = R.abs_scale_forward(x0, b0, fu, fd, **kw)
        by, bu = R.forward_bounds(x0, b0, fu, fd, y_ref=y64, fp16=fp16, scales=scales, generic=True, unit=unit, **kw)
        w = {'y': R.ratio((y.detach().double() - y64).abs(), by)}
        if fp16:
            # the activation kernel decides from the fp16 tensor the up pass stored: the same two calls give that tensor, it is held
            # to the float64 u, and the decisions are then exact -- from its values, in fp32 -- at every sample
            from torch_utils.ops import upfirdn2d
            with torch.no_grad():
                u16 = upfirdn2d.upfirdn2d(x0.add(b0[:, None, None]), fu, up=c['up'], padding=c['padding'], gain=c['up'] ** 2, flip_filter=flip)
            w['u'] = R.ratio((u16.double() - u64).abs(), bu + R.F16_SUB)            # + fp16's subnormal grid
            got = R.decode_signs(signs, 0, 0, tuple(u16.shape[2:]))
            w['sign mismatches'] = float((got != G.act_codes(u16, kw['gain'], kw['slope'], kw['clamp'], torch.float32)).sum())
            u64, bu = u16.double(), torch.zeros_like(bu)
            at0, atc = R.ambiguous(u64, bu, scales[0], kw['gain'], kw['slope'], kw['clamp'], unit)
            at0 = torch.zeros_like(at0)                                             # +-0 stored: code 0 and slope 1 on both sides
        else:
            at0, atc = R.ambiguous(u64, bu, scales[0], kw['gain'], kw['slope'], kw['clamp'], unit)
            w['sign mismatches'] = float(R.sign_mismatches(signs, 0, 0, u64, at0 | atc, kw['gain'], kw['slope'], kw['clamp']))
        dx64, db64 = R.adjoint_ref(gy, u64, xhw, fu, fd, **kw)
        bdx, wid, _ = R.adjoint_bounds(gy, u64, bu, scales[0], xhw, fu, fd, dx_ref=dx64, fp16=fp16, generic=True, unit=unit, **kw)
        w['dx'] = R.ratio((x.grad.double() - dx64).abs(), bdx)
        bdb = R.db_bound(bdx, dx64, None)                # torch's sum of the stored dx, accumulated in fp32 (float64: in float64)
        if fp16:
            bdb = bdb + R._f16_store(db64, bdb)
        w['db'] = R.ratio((b.grad.double() - db64).abs(), bdb)
        w['widened share'] = R.widened_share(wid)
        w['ambiguous share'] = float((at0 | atc).double().mean())
        worst[flip] = w
    print(f'generic filtered_lrelu {name} {dtype} {tuple(x0.shape)} -> {tuple(y.shape)}: ' +
          '  '.join(f'flip={k}: ' + ' '.join(f'{a} {v:.3g}' for a, v in w.items()) for k, w in worst.items()))
    for w in worst.values():
        assert w['sign mismatches'] == 0 and w['widened share'] <= 1e-3, worst
        assert max(w['y'], w.get('u', 0.0), w['dx'], w['db']) <= 1.0, worst


def test_generic_filtered_lrelu_double_backward():
    """fp32 up 1 / down 2: the backward run with grad enabled (the generic composition reading the signs) and differentiated once
    more with respect to the incoming gradient, against float64 autograd of `forward_ref`'s pipeline.  d<gx, v>/d gy is the
    forward's linear passes around the fixed mask, B (m gain (A v)): bound (n_u + 1 + n_d + 2) u |B| (m gain |A| |v|) with the
    generic counts without the bias, + 2 for the gain that is scaled by up^2 / down^2 and back on the host; ambiguous samples widen
    it by |B| (jump * gain * |A v|)."""
    c = G.FLRELU_GENERIC_CASES['up1_dn2']
    fu, fd = _f(c['fu']), _f(c['fd'])
    assert _no_fused_kernel(c, fu, fd)
    x0, b0 = (t.to(DEV) for t in G.flrelu_inputs('up1_dn2'))
    kw = dict(up=c['up'], down=c['down'], padding=c['padding'], gain=c['gain'], slope=c['slope'], clamp=c['clamp'], flip=False)
    gen = torch.Generator(device=DEV).manual_seed(22)
    x = x0.clone().requires_grad_(True); b = b0.clone().requires_grad_(True)
    y = _flrelu(c, x, b, fu, fd, False)
    gy = torch.randn(y.shape, device=DEV, generator=gen).requires_grad_(True)
    v = torch.randn(x.shape, device=DEV, generator=gen)
    gx, = torch.autograd.grad([y], [x], grad_outputs=[gy], create_graph=True)
    ggy, = torch.autograd.grad([gx], [gy], grad_outputs=[v])
    # float64 autograd of the same pipeline
    n, ch = x0.shape[:2]
    ops = R._ops(x0.shape[2:], fu, fd, c['up'], c['down'], c['padding'], False, DEV)
    x64 = x0.double().requires_grad_(True)
    u = R.Ops.apply(ops.A, (x64 + b0.double()[None, :, None, None]).reshape(n * ch, *x0.shape[2:]))
    a, neg, big = R._act(u, kw['gain'], kw['slope'], kw['clamp'])
    y64 = R.Ops.apply(ops.B, a).reshape(n, ch, *ops.y_hw)
    gy64 = gy.detach().double().requires_grad_(True)
    gx64, = torch.autograd.grad([y64], [x64], grad_outputs=[gy64], create_graph=True)
    ggy64, = torch.autograd.grad([gx64], [gy64], grad_outputs=[v.double()])
    e_gx = R.ratio((gx.detach().double() - gx64.detach()).abs(),
                   R.adjoint_bounds(gy.detach(), u.detach().reshape(n, ch, *ops.u_hw),
                                    R.forward_bounds(x0, b0, fu, fd, generic=True, **kw)[1], R.abs_scale_forward(x0, b0, fu, fd, **kw)[0],
                                    tuple(x0.shape[2:]), fu, fd, generic=True, **kw)[0])
    # the bound of ggy
    g = R.f32(kw['gain'])
    m = torch.where(big, 0.0, torch.where(neg, R.f32(kw['slope']), 1.0)).double() * g
    vp = v.double().reshape(n * ch, *x0.shape[2:])
    s1 = R.Ops.apply(ops.A, vp.abs(), absolute=True)
    pre = R.Ops.apply(ops.B, m * s1, absolute=True)
    (nu, _), (nd, _) = ops.generic_u(bias=False), ops.generic_down()
    _, bu = R.forward_bounds(x0, b0, fu, fd, generic=True, **kw)
    at0, atc = R.ambiguous(u.detach().reshape(n, ch, *ops.u_hw), bu, R.abs_scale_forward(x0, b0, fu, fd, **kw)[0], kw['gain'], kw['slope'], kw['clamp'])
    jump = (at0.double() * (1.0 - R.f32(kw['slope'])) + atc.double() * torch.where(neg.reshape(at0.shape), R.f32(kw['slope']), 1.0).double()).reshape(n * ch, *ops.u_hw)
    av = R.Ops.apply(ops.A, vp).abs() + nu * R.U * R.SECOND * s1
    wid = R.Ops.apply(ops.B, jump * g * av, absolute=True)
    bound = ((nu + 1 + nd + 2) * R.U * R.SECOND * pre + wid).reshape(n, ch, *ops.y_hw)
    e_ggy = R.ratio((ggy.double() - ggy64).abs(), bound)
    share = float((wid > 0).double().mean())
    print(f'generic filtered_lrelu double backward {tuple(x0.shape)}: err/bound gx {e_gx:.3f}  d<gx, v>/d gy {e_ggy:.3f}  widened share {share:.1e}')
    assert e_gx <= 1.0 and e_ggy <= 1.0 and share <= 1e-3
