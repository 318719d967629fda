"""GPU: the encoder's matrix-core kernels (csrc/sg3_conv2d.hip, csrc/sg3_head_gemm.hip) against float64, across kernel forms and
operand magnitudes.

Reference: a float64 CPU convolution of x * inScale + inShift (real pixels only; the padding stays zero) with the folded weights,
plus bias and activation.  Every output is bounded relative to mag = sum |a| |w| over its window, with no absolute floor.  The fp32
kernel is held to the worst-case fp32 summation bound; the split-precision form (fp16 hi + lo) is held, per output channel, to
max(2 x the fp32 kernel's error on the same data, the error of one split product) plus the absolute floors of its operand contract
(tests/split_model.py: activations below 2^-3, weights below 2^-17 of their channel's maximum).  The errors measured are printed
(pytest -s)."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import split_model as M

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24                                              # fp32 unit roundoff


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class _Precision:
    def __init__(self, prec):
        self.prec = prec

    def __enter__(self):
        from torch_utils.ops import plain_conv
        self.saved, plain_conv.precision = plain_conv.precision, self.prec

    def __exit__(self, *exc):
        from torch_utils.ops import plain_conv
        plain_conv.precision = self.saved


def _case(n, ci, co, h, w, k, stride, pad, act, affine, bias, seed, bn_log2=(-0.5, 0.5), w_scale=1.0, x_scale=1.0):
    r = np.random.RandomState(seed)
    c = dict(k=k, stride=stride, pad=pad, act=act)
    c['x'] = (r.randn(n, ci, h, w) * x_scale).astype(np.float32)
    c['w'] = (r.randn(co, ci, k, k) / np.sqrt(ci * k * k) * w_scale).astype(np.float32)
    c['out_scale'] = np.exp2(r.uniform(*bn_log2, co)).astype(np.float32)
    c['in_scale'] = r.uniform(0.5, 1.5, ci).astype(np.float32) if affine else None
    c['in_shift'] = (0.2 * x_scale * r.randn(ci)).astype(np.float32) if affine == 2 else None
    c['bias'] = (0.2 * r.randn(co)).astype(np.float32) if bias else None
    c['slope'] = r.uniform(0.1, 0.4, co).astype(np.float32) if act == 1 else (np.asarray([0.2], np.float32) if act == 2 else None)
    return c


def _conv(c):
    from torch_utils.ops.plain_conv import PackedConv
    T = lambda v: None if v is None else torch.from_numpy(v).to(DEV)  # noqa: E731
    return PackedConv(T(c['w']), out_scale=T(c['out_scale']), bias=T(c['bias']), in_scale=T(c['in_scale']), in_shift=T(c['in_shift']),
                      act=c['act'], slope=T(c['slope']), stride=c['stride'], padding=c['pad'])


def _reference(c):
    """float64: (out, mag = sum|a||w|, sum|w| over the real pixels of the window, sum|a| over the window, |out before the
    activation|: the fp32 rounding of the bias addition)."""
    x = torch.from_numpy(c['x']).double()
    a = x
    if c['in_scale'] is not None:
        a = a * torch.from_numpy(c['in_scale']).double()[None, :, None, None]
        if c['in_shift'] is not None:
            a = a + torch.from_numpy(c['in_shift']).double()[None, :, None, None]
    w = torch.from_numpy(c['w']).double() * torch.from_numpy(c['out_scale']).double()[:, None, None, None]
    kw = dict(stride=c['stride'], padding=c['pad'])
    y = F.conv2d(a, w, **kw)
    mag = F.conv2d(a.abs(), w.abs(), **kw)
    sumw = F.conv2d(torch.ones_like(a), w.abs(), **kw)
    suma = F.conv2d(a.abs(), torch.ones_like(w), **kw)
    if c['bias'] is not None:
        y = y + torch.from_numpy(c['bias']).double()[None, :, None, None]
    lin = y.abs().numpy()
    if c['act']:
        sl = torch.from_numpy(c['slope']).double()
        sl = sl[None, :, None, None] if c['act'] == 1 else sl[0]
        y = torch.where(y < 0, y * sl, y)
    return y.numpy(), mag.numpy(), sumw.numpy(), suma.numpy(), lin


def _run(conv, c, prec):
    from torch_utils.ops import plain_conv
    x = torch.from_numpy(c['x']).to(DEV)
    with _Precision(prec):
        form = conv.form(x)
        plain_conv.reset_overflow(DEV)
        y = conv(x)
        flagged = prec == 'f16x3' and plain_conv.overflowed(DEV)
    return y.cpu().numpy().astype(np.float64), form, flagged


def _model_weight_scale(c):
    """[O] inverse lifts the pack must apply (split_model.conv_pack on the same fp32 folded weights): the floor of the weight
    contract is taken from here, never from what the kernel reports."""
    return M.conv_pack(c['w'], c['out_scale'])[2].astype(np.float64)


def _per_channel(v):
    return v.transpose(1, 0, 2, 3).reshape(v.shape[1], -1).max(axis=1)


def _check_conv(c, label, forms=None):
    """Both kernels against float64; returns a list of failure messages (empty when the case passes)."""
    conv = _conv(c)
    ref, mag, sumw, suma, lin = _reference(c)
    y32, f32, _ = _run(conv, c, 'fp32')
    ys, fs, flagged = _run(conv, c, 'f16x3')
    if forms is not None:
        forms.setdefault(f32, label)
        forms.setdefault(fs, label)
    fails = []
    assert y32.shape == ref.shape and ys.shape == ref.shape
    if flagged:
        return [f'{label}: range flag raised']
    safe = np.where(mag > 0, mag, 1.0)
    k_terms = c['w'].shape[1] * c['k'] * c['k']
    rnd = U * lin / safe                                    # both round acc + bias to fp32 once
    e32 = np.abs(y32 - ref) / safe - rnd
    es = np.abs(ys - ref) / safe - rnd
    # fp32: worst-case summation bound (K terms) + the input affine and the weight fold (one rounding each)
    lim32 = (k_terms + 4) * U / (1 - (k_terms + 4) * U)
    ws = _model_weight_scale(c)
    assert np.array_equal(conv.weight_scale(1).cpu().numpy().astype(np.float64), ws), label
    floor = (M.ACT_ABS * sumw + M.CONV_W_ABS_LIFTED * ws[None, :, None, None] * suma) / safe
    ch32 = np.maximum(_per_channel(e32), 0.0)
    allow = np.maximum(2 * ch32, M.PROD_REL_CONV)
    chs = _per_channel(es - floor)
    print(f'{label:48s} form {f32:2d}/{fs:2d}  fp32 {ch32.max():.2e}  split {_per_channel(es).max():.2e}  '
          f'(split - floor) / allowed {np.max(chs / allow):.3f}')
    if not np.all(e32 <= lim32):
        fails.append(f'{label}: fp32 kernel error {e32.max():.3e} > summation bound {lim32:.3e}')
    if not np.all(chs <= allow):
        o = int(np.argmax(chs / allow))
        fails.append(f'{label}: split error {chs[o]:.3e} of channel {o} (folded scale {c["out_scale"][o]:.3g}) > allowed {allow[o]:.3e} '
                     f'(fp32 kernel {ch32[o]:.3e})')
    z = mag == 0
    if z.any() and not (np.all(np.abs(ys - ref)[z] <= U * np.abs(ref[z])) and np.all(np.abs(y32 - ref)[z] <= U * np.abs(ref[z]))):
        fails.append(f'{label}: outputs with an all-zero window differ from bias + activation')
    return fails


def _form_cases():
    """Shapes for every form of both dispatchers, ragged everywhere (I not a multiple of the 8 / 16 channel chunk, O not a multiple
    of the tile, odd output planes), every activation, with and without input affine and bias, every padding the ABI accepts."""
    cus = _cus()
    per8 = lambda co, oh, ow: math.ceil(co / 64) * math.ceil(oh / 8) * math.ceil(ow / 32)  # noqa: E731
    n8 = math.ceil(2 * cus / per8(70, 33, 37)) + 1            # >= 2 eight-row tiles per CU: the 8-row split tile
    assert n8 * per8(70, 33, 37) >= 2 * cus and per8(70, 33, 37) < 2 * cus
    cases = []
    #            n, ci,  co,  h,  w, k, s, pad, act, affine, bias
    for k, pads in ((3, (0, 1, 2)), (1, (0, 1))):
        for s in (1, 2):
            for j, pad in enumerate(pads):
                cases += [(2, 21, 150, 35 if s == 2 else 19, 41, k, s, pad, j % 3, (j + 1) % 3, j != 1),   # O >= 128, outH >= 8
                          (1, 37, 70, 13, 9, k, s, pad, (j + 1) % 3, j % 3, j == 1),                         # 32 < O
                          (3, 9, 29, 23, 35, k, s, pad, (j + 2) % 3, 2, True)]                               # O <= 32
    cases += [(1, 40, 70, 33, 37, 3, 1, 1, 1, 2, True),        # 3x3 stride 1, outH > 16, few tiles: 4-row split tile
              (n8, 40, 70, 31, 35, 3, 1, 2, 2, 1, False),       # ... padding 2: 33 x 37 output, the 8-row split tile
              (2, 17, 33, 12, 14, 3, 1, 1, 0, 0, True)]         # outH <= 16
    return cases


def test_conv2d_every_form_against_float64():
    forms, fails = {}, []
    for i, (n, ci, co, h, w, k, s, pad, act, affine, bias) in enumerate(_form_cases()):
        c = _case(n, ci, co, h, w, k, s, pad, act, affine, bias, seed=100 + i)
        fails += _check_conv(c, f'n{n} i{ci} o{co} {h}x{w} k{k} s{s} p{pad} act{act} aff{affine} b{int(bias)}', forms)
    from torch_utils import _sg3abi as abi
    print('forms hit:', {f: forms[f] for f in sorted(forms)})
    assert sorted(forms) == list(range(12)) + [abi.SG3_CONV2D_FORM_F16X3 + j for j in range(6)]
    assert not fails, '\n'.join(fails)


# one shape per split form (k, stride, pad, and the size that selects it)
def _split_form_shapes():
    cus = _cus()
    n8 = math.ceil(2 * cus / (2 * 5 * 2)) + 1                  # 70 channels (2 M tiles) x 33 rows (5) x 35 columns (2)
    return [(2, 51, 70, 20, 22, 1, 2, 0), (2, 51, 70, 20, 22, 1, 1, 0), (2, 51, 70, 20, 22, 3, 2, 1), (2, 51, 70, 14, 22, 3, 1, 1),
            (1, 51, 70, 33, 35, 3, 1, 1), (n8, 27, 70, 33, 35, 3, 1, 1)]


@pytest.mark.parametrize('form', range(6))
def test_conv2d_split_magnitude_sweep(form):
    """Per-output-channel folded scales log-uniform over 2^-12 .. 2^4, a global weight scale and activation scales 2^-8 .. 2^8
    (peak below the 65000 guard): the split form stays within twice the fp32 kernel's error per channel (plus its activation
    floor).  Before the per-channel weight lift of the pack, small folded scales fail here by orders of magnitude."""
    from torch_utils import _sg3abi as abi
    from torch_utils.ops import plain_conv
    n, ci, co, h, w, k, s, pad = _split_form_shapes()[form]
    fails = []
    for j, (ws, xs) in enumerate([(1.0, 1.0), (2.0 ** -6, 2.0 ** -8), (2.0 ** -6, 2.0 ** 8), (2.0 ** 3, 1.0), (1.0, 2.0 ** -4), (2.0 ** -10, 2.0 ** 4)]):
        c = _case(n, ci, co, h, w, k, s, pad, act=j % 3, affine=1 + j % 2, bias=True, seed=300 + 10 * form + j, bn_log2=(-12, 4),
                  w_scale=ws, x_scale=xs)
        assert np.abs(c['x']).max() * 1.5 + 0.2 * xs * 5 < M.FP16_GUARD
        conv = _conv(c)
        with _Precision('f16x3'):
            assert conv.form(torch.from_numpy(c['x']).to(DEV)) == abi.SG3_CONV2D_FORM_F16X3 + form
        fails += _check_conv(c, f'form {form} w x{ws:g} x x{xs:g}')
    plain_conv.reset_overflow(DEV)
    assert not fails, '\n'.join(fails)


def test_conv2d_split_large_plane_64bit_epilogue():
    """O = 64, 1x1 on a 2400^2 plane: (64 + 32) * plane bytes passes 2^31, so the split kernel stores through 64-bit addresses.
    Windows of the big result equal, bit for bit, the convolution of the matching input crop (descriptor epilogue), and one
    window is checked against float64."""
    from torch_utils import _sg3abi as abi
    side, ci, co = 2400, 16, 64
    c = _case(1, ci, co, 8, 8, 1, 1, 0, act=1, affine=2, bias=True, seed=7, bn_log2=(-10, 2))
    conv = _conv(c)
    assert (64 + 32) * side * side * 4 >= 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn([1, ci, side, side], device=DEV, generator=g)
    with _Precision('f16x3'):
        assert conv.form(x) == abi.SG3_CONV2D_FORM_F16X3 + 1
        big = conv(x)
        for (y0, x0) in ((0, 0), (1234, 987), (side - 200, side - 200)):
            crop = x[:, :, y0:y0 + 200, x0:x0 + 200].contiguous()
            small = conv(crop)
            assert torch.equal(big[:, :, y0:y0 + 200, x0:x0 + 200], small), (y0, x0)
        win = big[:, :, side - 200:, side - 200:].cpu().numpy()
    del big, x
    torch.cuda.empty_cache()
    c['x'] = crop.cpu().numpy()
    ref, mag, sumw, suma, lin = _reference(c)
    ws = _model_weight_scale(c)
    assert np.array_equal(conv.weight_scale(1).cpu().numpy().astype(np.float64), ws)
    err = np.abs(win - ref) / mag - (M.ACT_ABS * sumw + M.CONV_W_ABS_LIFTED * ws[None, :, None, None] * suma + U * lin) / mag
    print(f'large plane: split error {err.max():.2e} of sum|a||w|')
    assert err.max() <= M.PROD_REL_CONV + 2 * (ci + 4) * U


@pytest.mark.parametrize('prec', ['f16x3', 'fp32'])
def test_conv2d_nonfinite_inputs(prec):
    """A NaN input stays in exactly the outputs whose window contains it (every output channel of that sample); +-inf raises the
    split form's range flag."""
    from torch_utils.ops import plain_conv
    c = _case(2, 20, 40, 18, 21, 3, 1, 1, act=0, affine=0, bias=True, seed=11)
    conv = _conv(c)
    c['x'][1, 7, 5, 9] = np.nan
    x = torch.from_numpy(c['x']).to(DEV)
    with _Precision(prec):
        plain_conv.reset_overflow(DEV)
        y = conv(x).cpu()
        assert not plain_conv.overflowed(DEV)
    want = torch.zeros_like(y, dtype=torch.bool)
    want[1, :, 4:7, 8:11] = True                              # outputs (y, x) with |y - 5| <= 1, |x - 9| <= 1
    assert torch.equal(torch.isnan(y), want)
    assert torch.isfinite(y[~want]).all()
    for v in (np.inf, -np.inf):
        xi = c['x'].copy()
        xi[1, 7, 5, 9] = 0.0
        xi[0, 3, 17, 20] = v
        with _Precision(prec):
            plain_conv.reset_overflow(DEV)
            conv(torch.from_numpy(xi).to(DEV))
            assert plain_conv.overflowed(DEV) == (prec == 'f16x3')
    plain_conv.reset_overflow(DEV)


@pytest.mark.parametrize('g,m,k,n,slope', [(4, 8, 512, 64, 0.01), (3, 40, 4608, 96, 1.0), (2, 130, 144, 32, 0.2)])
def test_head_gemm_magnitude_sweep(g, m, k, n, slope):
    """Per-column weight scales log-uniform over 2^-12 .. 2^4 (and a global one), activation scales 2^-8 .. 2^8: per column,
    the split GEMM stays within max(2 x fp32 torch.baddbmm's error, one split product) plus its activation floor, bounded by
    sum |a| |w| with no absolute term."""
    from torch_utils.ops import plain_conv
    from torch_utils.ops.head_gemm import PackedHeadWeights
    fails = []
    for j, (ws, xs) in enumerate([(1.0, 1.0), (2.0 ** -6, 2.0 ** -8), (2.0 ** -6, 2.0 ** 8), (2.0 ** 3, 2.0 ** -4)]):
        r = np.random.RandomState(500 + j)
        a = (r.randn(g, m, k) * xs).astype(np.float32)
        w = (r.randn(g, k, n) / np.sqrt(k) * ws * np.exp2(r.uniform(-12, 4, (g, 1, n)))).astype(np.float32)
        b = r.randn(g, n).astype(np.float32)
        pw = PackedHeadWeights(torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV))
        assert pw.usable
        plain_conv.reset_overflow(DEV)
        at = torch.from_numpy(a).to(DEV)
        out = pw.run(at, slope).cpu().numpy().astype(np.float64)
        assert not plain_conv.overflowed(DEV)
        act32 = F.leaky_relu(at, slope)
        blas = torch.baddbmm(torch.from_numpy(b).to(DEV)[:, None, :], act32, torch.from_numpy(w).to(DEV)).cpu().numpy().astype(np.float64)
        a64 = a.astype(np.float64)
        act = np.where(a64 < 0, a64 * np.float64(np.float32(slope)), a64)
        ref = np.einsum('gmk,gkn->gmn', act, w.astype(np.float64)) + b.astype(np.float64)[:, None, :]
        mag = np.einsum('gmk,gkn->gmn', np.abs(act), np.abs(w.astype(np.float64)))
        sumw = np.abs(w.astype(np.float64)).sum(axis=1)[:, None, :]
        suma = np.abs(act).sum(axis=2)[:, :, None]
        cs = M.head_pack(w)[2].astype(np.float64)[:, None, :]       # the model's lift, not the kernel's
        assert np.array_equal(pw.col_scale.cpu().numpy().astype(np.float64), cs[:, 0, :])
        rnd = U * np.abs(ref) / mag                                  # the fp32 rounding of the bias addition
        floor = (M.ACT_ABS * sumw + M.HEAD_W_ABS_LIFTED * cs * suma) / mag
        es = (np.abs(out - ref) / mag - floor - rnd).max(axis=1)    # per (head, column)
        eb = np.maximum((np.abs(blas - ref) / mag - rnd).max(axis=1), 0.0)
        allow = np.maximum(2 * eb, M.PROD_REL_HEAD)
        print(f'head g{g} m{m} k{k} n{n} w x{ws:g} a x{xs:g}: baddbmm {eb.max():.2e}  split {(np.abs(out - ref) / mag).max():.2e}  '
              f'(split - floor) / allowed {np.max(es / allow):.3f}')
        if not np.all(es <= allow):
            fails.append(f'w x{ws:g} a x{xs:g}: split {es.max():.3e} > allowed (baddbmm {eb.max():.3e})')
    assert not fails, '\n'.join(fails)


def _own_bn_statistics(enc, seed):
    """BatchNorm statistics of the test's own: the BatchNorm behind each residual branch (folded into the packed weights) gets
    gammas log-uniform over 2^-8 .. 2^0, every other one gammas around 1; means and variances random."""
    r = np.random.RandomState(seed)
    with torch.no_grad():
        for name, m in enc.named_modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                small = name.endswith('res_layer.4') or name.endswith('bn2')
                gamma = np.exp2(r.uniform(-8, 0, c)) if small else r.uniform(0.7, 1.3, c)
                m.weight.copy_(torch.from_numpy(gamma * r.choice([-1.0, 1.0], c)))
                m.bias.copy_(torch.from_numpy(0.1 * r.randn(c)))
                m.running_mean.copy_(torch.from_numpy(0.1 * r.randn(c)))
                m.running_var.copy_(torch.from_numpy(r.uniform(0.5, 2.0, c)))
    return enc


@pytest.mark.parametrize('kind', ['ir_se50', 'resnet34'])
def test_encoder_split_against_float64(kind):
    """Whole encoders with small folded BatchNorm gammas: the split path's error against a float64 CPU forward of the same
    modules is at most twice the fp32 path's; the range-guard fallback (inputs beyond the fp16 range) matches float64 too."""
    from test_encoder_cpu import _input, build_product_encoder, build_resnet_encoder
    from torch_utils.ops import plain_conv
    enc = build_product_encoder('cpu') if kind == 'ir_se50' else build_resnet_encoder(4, 'cpu')[0]
    enc = _own_bn_statistics(enc, seed=21).eval().requires_grad_(False)
    enc64 = copy.deepcopy(enc).double()
    enc = enc.to(DEV)
    x = _input()
    with torch.no_grad():
        ref = enc64._forward_torch(torch.from_numpy(x).double()).numpy()
        xt = torch.from_numpy(x).to(DEV)
        plain_conv.reset_overflow(DEV)
        split = enc(xt).cpu().numpy().astype(np.float64)
        assert not plain_conv.overflowed(DEV)
        with _Precision('fp32'):
            fp32 = enc(xt).cpu().numpy().astype(np.float64)
        scale = np.abs(ref).max()
        es, e32 = np.abs(split - ref).max() / scale, np.abs(fp32 - ref).max() / scale
        print(f'{kind}: split {es:.2e}  fp32 {e32:.2e} of max|ref| {scale:.3g}')
        assert es <= 2 * e32
        # the range guard: 1e6-scale inputs overflow fp16 in the first layer; the forward repeats on the fp32 kernels
        big = x * 1e6
        ref_big = enc64._forward_torch(torch.from_numpy(big).double()).numpy()
        plain_conv.reset_overflow(DEV)
        fb = enc(torch.from_numpy(big.astype(np.float32)).to(DEV)).cpu().numpy().astype(np.float64)
        assert plain_conv.overflowed(DEV)
        plain_conv.reset_overflow(DEV)
        sb = np.abs(ref_big).max()
        eb = np.abs(fb - ref_big).max() / sb
        print(f'{kind}: fallback {eb:.2e} of max|ref| {sb:.3g}')
        # another input, so no same-data fp32 twin to compare with: twice the split-input fp32 error, at least 1e-5 of max|ref|
        assert eb <= max(2 * e32, 1e-5)
