"""GPU: the style and input stage against float64 -- `sg3_modulated_conv2d_prep[_batch]`, `sg3_affine_batch`, `sg3_input_transform`,
`sg3_fourier_features` -- with the references, bounds and cases of tests/style_stage_ref.py (derivations in its docstring).

Every test prints its worst error / bound (and, where a torch composite exists, e_hip / e_torch32 against float64) before it asserts;
the module prints the maxima per kernel at the end (pytest -s)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import style_stage_ref as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAN = float('nan')
SUB = 2.0 ** -150                    # half a step of the fp32 subnormal grid: what a product that underflows can lose

_worst = {}


def note(key, value, what=''):
    if value > _worst.get(key, (-1.0, ''))[0]:
        _worst[key] = (float(value), what)


@pytest.fixture(scope='module', autouse=True)
def _report():
    yield
    print('\nstyle stage against float64, worst over the module:')
    for key in sorted(_worst):
        print('    %-34s %.3f   %s' % (key, _worst[key][0], _worst[key][1]))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- modconv prep

class Prep:
    """One parameter block of sg3_modulated_conv2d_prep with its tensors; outputs are filled with NaN beforehand."""

    def __init__(self, c, w, s, gain, weights_from=None):
        from torch_utils import _sg3abi as abi
        lib = abi.load()
        n, ci, co, k, prec = c['N'], c['I'], c['O'], c['k'], c['precision']
        assert tuple(w.shape) == (co, ci, k, k) and tuple(s.shape) == (n, ci) and w.is_contiguous() and s.is_contiguous()
        assert gain is None or gain.numel() == (1, 1, ci, n * ci)[c['gain_mode']]
        self.c, self.w, self.s, self.gain = c, w, s, gain
        floats = int(lib.sg3_modconv_packed_floats(co, ci, k, prec))
        if weights_from is None:
            self.wn = torch.full([floats], NAN, dtype=torch.float32, device=DEV)
            self.wsq = torch.full([co, ci], NAN, dtype=torch.float32, device=DEV)
        else:
            assert weights_from.wn.numel() == floats
            self.wn, self.wsq = weights_from.wn.clone(), weights_from.wsq.clone()
        self.s_in = torch.full([n, ci], NAN, dtype=torch.float32, device=DEV)
        self.dcoef = torch.full([n, co], NAN, dtype=torch.float32, device=DEV)
        self.bound = torch.full([1], c['x_bound'], dtype=torch.float32, device=DEV) if c['bound_on_device'] else None
        pp = abi.ModconvPrepParams()
        pp.w, pp.s, pp.wPacked, pp.wsq, pp.sIn, pp.dcoef = (abi.ptr(t) for t in (w, s, self.wn, self.wsq, self.s_in, self.dcoef))
        pp.inputGain, pp.inputGainMode = abi.ptr(gain), c['gain_mode']
        pp.N, pp.I, pp.O, pp.k, pp.demodulate, pp.precision = n, ci, co, k, int(c['demodulate']), prec
        pp.xBound = 0.0 if c['bound_on_device'] else c['x_bound']
        pp.xBoundDev = abi.ptr(self.bound)
        pp.reuseWeights = int(weights_from is not None)
        self.params = pp

    def run(self):
        from torch_utils import _sg3abi as abi
        with torch.cuda.device(DEV):
            abi.check(abi.load().sg3_modulated_conv2d_prep(ctypes.byref(self.params), abi.stream_ptr(torch.device(DEV))), 'sg3_modulated_conv2d_prep')
            torch.cuda.synchronize()
        return self

    def outputs(self):
        return self.wn, self.wsq, self.s_in, self.dcoef


def f23_allowed(c):
    """The transform-domain forms exist for shapes sg3_modconv_f23_supported takes (a 52 x 52 plane, padding 2)."""
    from torch_utils import _sg3abi as abi
    if c['precision'] not in S.F23_FORMS:
        return True
    dtype = abi.SG3_F32 if c['precision'] == S.CONV_F16X3_F23 else abi.SG3_F16
    return abi.load().sg3_modconv_f23_supported(dtype, c['I'], c['O'], 52, 52, c['k'], 2, 0) == 1


def case_tensors(c):
    s, gain = S.case_styles(c)
    return dev(S.case_weights(c)), dev(s), dev(gain)


def check_prep(c, w, s, gain, wsq, s_in, dcoef, check_weights=True):
    """wsq, sIn, dcoef of one call against prep_ref under prep_bounds; the exponent read off sIn / v.  Returns the exponents [N]."""
    n, ci, co, k, prec, demod = c['N'], c['I'], c['O'], c['k'], c['precision'], c['demodulate']
    r = S.prep_ref(w, s, demod, gain, c['x_bound'], prec)
    b_wsq, b_v, b_d = S.prep_bounds(n, ci, k, demod, gain is not None)
    wsq, s_in, dcoef = wsq.double().cpu(), s_in.double().cpu(), dcoef.double().cpu()
    if check_weights:
        assert bool(torch.isfinite(wsq).all()), c['id']
        q = float(((wsq - r['wsq']).abs() / (b_wsq * r['wsq'] + k * k * 2.0 ** -126)).max())
        note('prep wsq err/bound', q, c['id'])
        assert q <= 1.0, (c['id'], 'wsq', q)
    assert bool(torch.isfinite(s_in).all()), (c['id'], 'sIn not finite')
    es = []
    for j in range(n):
        v, d = r['v'][j], r['d'][j]
        ratio = s_in[j] / v
        assert bool((ratio > 0).all()), (c['id'], j)
        each = torch.round(-torch.log2(ratio))
        e = int(each[0])
        assert bool((each == e).all()), (c['id'], j, 'sIn / v is not one power of two', each.unique().tolist())
        assert e == int(r['e_kept'][j]), (c['id'], j, 'exponent', e, int(r['e'][j]), float(r['peak'][j]))
        es.append(e)
        err = (s_in[j] * 2.0 ** e - v).abs()
        bound = b_v * v.abs() + SUB * 2.0 ** e
        assert bool((err <= bound).all()), (c['id'], j, 'sIn', float((err / bound).max()))
        if b_v > 0:
            note('prep sIn err/bound', float((err / bound).max()), c['id'])
        if prec != S.CONV_FP32 and e == int(r['e'][j]):
            top = 14 if prec in S.F23_FORMS else 15
            scaled = float(r['peak'][j]) * 2.0 ** -e
            assert 2.0 ** (top - 1) < scaled <= 2.0 ** top, (c['id'], j, scaled)
        if demod:
            assert bool(torch.isfinite(dcoef[j]).all()), (c['id'], j, 'dcoef not finite')
            err = (dcoef[j] * 2.0 ** -e - d).abs()
            bound = b_d * d + SUB * 2.0 ** -e
            q = float((err / bound).max())
            note('prep dcoef err/bound', q, c['id'])
            assert q <= 1.0, (c['id'], j, 'dcoef', q)
        elif prec != S.CONV_FP32:
            assert bool((dcoef[j] == 2.0 ** e).all()), (c['id'], j, 'dcoef is not 2^e')
        else:
            assert bool(torch.isnan(dcoef[j]).all()), (c['id'], j, 'dcoef written without demodulation in fp32')
    return es, r


def run_and_check(c):
    assert f23_allowed(c), c['id']
    w, s, gain = case_tensors(c)
    p = Prep(c, w, s, gain).run()
    return check_prep(c, w, s, gain, p.wsq, p.s_in, p.dcoef), p


SHAPE_CASES = [c for c in S.shape_cases()]


@pytest.mark.parametrize('c', SHAPE_CASES, ids=[c['id'] for c in SHAPE_CASES])
def test_prep_shapes(c):
    """Every (I, O) pair of the 256-thread strides, the 64-lane tails, the sixteen workgroups per sample (O = 513: their tail) and the
    LDS sizing, at k = 1 and k = 3, the other settings cycling."""
    assert f23_allowed(c), c['id']
    run_and_check(c)


@pytest.mark.parametrize('shape', S.VARIATION_SHAPES, ids=lambda sh: 'N%d_I%d_O%d_k%d' % sh)
def test_prep_variations(shape):
    """demodulate x inputGainMode 0-3 x every precision x bound on the host | the device, at one shape each."""
    seen = set()
    for c in S.variation_cases(shape):
        assert f23_allowed(c), c['id']
        run_and_check(c)
        seen.add(c['precision'])
    assert seen == set(range(5 if shape[3] == 3 else 3))


@pytest.mark.parametrize('shape', S.MAGNITUDE_SHAPES, ids=lambda sh: 'N%d_I%d_O%d_k%d' % sh)
def test_prep_magnitudes(shape):
    """Styles x 1e-4 .. 1e4 (one sample 1e-3 of the others: the 1e-8 of the demodulation matters for it), weights x 2^-8 .. 2^8, bounds
    2^-100 .. 65504."""
    for c in S.magnitude_cases(shape):
        assert f23_allowed(c), c['id']
        run_and_check(c)


def test_prep_exponent_on_a_power_of_two():
    """peak = 32768 * 2^j exactly: e = j, the peak lands on 2^15 itself."""
    for c in S.exact_cases():
        (es, _), _ = run_and_check(c)
        assert es == [c['exact_j']] * c['N'], (c['id'], es)


def test_prep_peak_near_2_to_minus_120():
    """A device bound of 1.3 * 2^-121 (a gradient that has almost underflowed): the exact exponent, about -134, has no normal 2^-e.
    sIn, dcoef and their product are finite, the exponent is the kept one and sIn * dcoef = v * d all the same."""
    for c in S.tiny_cases():
        (es, r), p = run_and_check(c)
        assert (r['e'] < -S.E_LIMIT).all() and es == [-S.E_LIMIT] * c['N'], (c['id'], es, r['e'])
        s_in, dcoef = p.s_in.double().cpu(), p.dcoef.double().cpu()
        prod = s_in.unsqueeze(1) * dcoef.unsqueeze(2)                            # [N,O,I], exact in float64
        want = r['v'].unsqueeze(1) * r['d'].unsqueeze(2)
        assert bool(torch.isfinite(prod).all()) and bool(torch.isfinite(p.s_in).all()) and bool(torch.isfinite(p.dcoef).all())
        _, b_v, b_d = S.prep_bounds(c['N'], c['I'], c['k'], c['demodulate'], c['gain_mode'] != 0)
        # dcoef = d 2^-126 is subnormal where d < 1 and then sits on the 2^-149 grid: half a step of it, times |sIn|
        bound = (b_v + b_d) * (1 + 1e-6) * want.abs() + SUB * s_in.abs().unsqueeze(1)
        q = float(((prod - want).abs() / bound).max())
        note('prep sIn*dcoef err/bound (tiny)', q, c['id'])
        assert q <= 1.0, (c['id'], q)


def test_prep_reuse_weights():
    """reuseWeights = 1 after a first call: wsq and wPacked keep their bits, sIn and dcoef follow the new styles."""
    for c in (S.make_case(3, 70, 130, 3, True, 2, S.CONV_F16X3, 3.0, seed=41, tag='reuse'),
              S.make_case(3, 257, 513, 1, True, 1, S.CONV_F16, 3.0, True, seed=42, tag='reuse'),
              S.make_case(1, 64, 130, 3, True, 0, S.CONV_F16X3_F23, 3.0, seed=43, tag='reuse'),
              S.make_case(3, 17, 33, 3, True, 3, S.CONV_FP32, 0.0, seed=44, tag='reuse'),
              S.make_case(3, 64, 3, 1, False, 0, S.CONV_F16X3, 3.0, seed=45, tag='reuse')):
        assert f23_allowed(c)
        w, s, gain = case_tensors(c)
        first = Prep(c, w, s, gain).run()
        check_prep(c, w, s, gain, first.wsq, first.s_in, first.dcoef)
        assert not bool(torch.isnan(first.wn).any()), 'the packed buffer is written in full'
        s2 = (s.flip(1) * 1.75 + 0.25).contiguous()
        second = Prep(c, w, s2, gain, weights_from=first).run()
        assert second.params.reuseWeights == 1
        assert torch.equal(bits(second.wn), bits(first.wn)) and torch.equal(bits(second.wsq), bits(first.wsq)), c['id']
        check_prep(c, w, s2, gain, second.wsq, second.s_in, second.dcoef)
        assert not torch.equal(second.s_in, first.s_in)


def _batch_pool():
    pool = [c for c in S.shape_cases() if c['I'] * c['O'] * c['k'] ** 2 <= 300_000]
    for sh in S.VARIATION_SHAPES:
        pool += S.variation_cases(sh)[::7]
    return pool


@pytest.mark.parametrize('count', [1, 16, 17, 33])
def test_prep_batch_is_the_single_call(count):
    """sg3_modulated_conv2d_prep_batch on lists that end in, fill, and run past its chunks of sixteen (17: a second chunk of one; 33:
    a third): every entry bit-identical to its own sg3_modulated_conv2d_prep.  Shapes, precisions and demodulation are mixed; the
    first and the last entry of a chunk (and one inside) have reuseWeights = 1 and keep their packed weights' bits."""
    from torch_utils import _sg3abi as abi
    pool = _batch_pool()
    cases = [pool[(5 * j + 3 * count) % len(pool)] for j in range(count)]
    reuse = {0, 5, 15, 16, count - 1} if count > 1 else set()
    assert {c['precision'] for c in cases} >= ({0, 1, 2} if count > 1 else set()) and (count == 1 or len({c['demodulate'] for c in cases}) == 2)
    single, batch = [], []
    for j, c in enumerate(cases):
        assert f23_allowed(c), c['id']
        w, s, gain = case_tensors(c)
        single.append(Prep(c, w, s, gain).run())
        batch.append(Prep(c, w, s, gain, weights_from=single[-1] if j in reuse else None))
    block = (abi.ModconvPrepParams * count)(*[p.params for p in batch])
    with torch.cuda.device(DEV):
        abi.check(abi.load().sg3_modulated_conv2d_prep_batch(block, count, abi.stream_ptr(torch.device(DEV))), 'sg3_modulated_conv2d_prep_batch')
        torch.cuda.synchronize()
    for j, (a, b) in enumerate(zip(single, batch)):
        for name, x, y in zip(('wPacked', 'wsq', 'sIn', 'dcoef'), a.outputs(), b.outputs()):
            assert torch.equal(bits(x), bits(y)), (count, j, a.c['id'], name, 'reuse' if j in reuse else '')
        assert not bool(torch.isnan(b.s_in).any())
    # one entry of the last chunk against float64 as well (the single calls are checked case by case above)
    c, b = cases[-1], batch[-1]
    check_prep(c, b.w, b.s, b.gain, b.wsq, b.s_in, b.dcoef)


def test_prepare_batch_against_float64():
    """modulated_conv.prepare_batch (what inference calls) on seventeen layers: sIn, dcoef and wsq of every entry against prep_ref with
    the form `_choose_form` picked; a second pass takes the packed weights from the cache (reuseWeights = 1), leaves them untouched and
    follows the new styles."""
    from torch_utils.ops import modulated_conv as mc
    g = torch.Generator().manual_seed(77)
    layers = []
    for j in range(17):
        ci, co = (70, 33, 257, 64, 130, 17)[j % 6], (33, 130, 3, 513, 64)[j % 5]
        k = 1 if co == 3 or j % 4 == 3 else 3
        n = (1, 3)[j % 2]
        w = torch.randn(co, ci, k, k, generator=g).to(DEV)
        gain = [None, torch.tensor(0.8), torch.rand(ci, generator=g) + 0.5, torch.rand(n, ci, generator=g) + 0.5][j % 4]
        layers.append(dict(w=w, demodulate=co != 3, padding=k - 1 if k == 3 else 0, input_gain=None if gain is None else gain.to(DEV), x_bound=3.0, n=n, h=52,
                           wd=52, dtype=torch.float16 if j % 5 == 4 or j == 3 else torch.float32))
    mc.clear_weight_cache()
    try:
        seen = set()
        for rnd in range(2):
            specs = [dict(sp, s=(torch.randn(sp['n'], sp['w'].shape[1], generator=g) + 1).to(DEV)) for sp in layers]
            with torch.no_grad():
                plans = mc.prepare_batch(specs)
                torch.cuda.synchronize()
            if rnd == 0:
                kept = [(pl.wn, bits(pl.wn).clone(), bits(pl.wsq).clone()) for pl in plans]
            for sp, pl, (wn, wn_bits, wsq_bits) in zip(specs, plans, kept):
                assert pl.params.reuseWeights == rnd
                assert pl.wn is wn and torch.equal(bits(pl.wn), wn_bits) and torch.equal(bits(pl.wsq), wsq_bits)
                co, ci, k, _ = sp['w'].shape
                gain = sp['input_gain']
                mode = 0 if gain is None else (1 if gain.numel() == 1 else gain.ndim + 1)
                c = S.make_case(sp['n'], ci, co, k, sp['demodulate'], mode, pl.prec, sp['x_bound'] if pl.prec != S.CONV_FP32 else 0.0,
                                tag='prepare_batch%d' % rnd)
                seen.add(pl.prec)
                dcoef = pl.dcoef if pl.dcoef is not None else torch.full([sp['n'], co], NAN)
                check_prep(c, sp['w'], sp['s'], gain, pl.wsq, pl.s_in, dcoef)
        assert seen == set(range(5)), seen
    finally:
        mc.clear_weight_cache()


@pytest.mark.parametrize('prec', [S.CONV_FP32, S.CONV_F16X3])
@pytest.mark.parametrize('bad', [NAN, float('inf')])
def test_prep_non_finite_styles(bad, prec):
    """One NaN, one inf in one sample's styles with demodulation: the non-finite pattern of sIn and dcoef is that of the float64 formula
    (the normalisation runs over the whole batch: a NaN reaches every sample, an inf zeroes the finite styles)."""
    c = S.make_case(3, 70, 33, 3, True, 1, prec, 3.0 if prec else 0.0, seed=61, tag='nonfinite')
    w, s, gain = case_tensors(c)
    s[1, 17] = bad
    p = Prep(c, w, s, gain).run()
    r = S.prep_ref(w, s, True, gain, c['x_bound'], prec)
    assert (r['e'] == 0).all()                                     # the peak is 0: fmaxf drops the NaN, the finite styles are 0 or NaN
    for name, got, want in (('sIn', p.s_in, r['v']), ('dcoef', p.dcoef, r['d'])):
        got = got.cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want)), (name, bad)
        fin = torch.isfinite(want)
        assert bool(((got.double()[fin] - want[fin]).abs() <= 1e-5 * want[fin].abs()).all()), name
    assert bool(torch.isnan(r['v']).any()) and (math.isnan(bad) or bool(torch.isfinite(r['d']).any()))


# ---------------------------------------------------------------------------------------------------------------- affine_batch

def _fc_layers(w_dim, count, variant, seed):
    from models.stylegan3.networks_stylegan3 import FullyConnectedLayer
    torch.manual_seed(seed)
    # one layer: 37 rows with a bias | a single row without; twenty: 1097 rows in all, the third layer without a bias
    rows = ((37, 1)[variant],) if count == 1 else (1, 3, 4, 5, 64, 130, 1, 7, 33, 2, 512, 9, 1, 6, 31, 17, 4, 258, 3, 6)
    assert len(rows) == count
    fcs = []
    for j in range(count):
        fc = FullyConnectedLayer(w_dim, rows[j], bias=(j != 2 and not (count == 1 and variant == 1)), bias_init=1.0, lr_multiplier=(1, 0.5)[j % 2])
        if fc.bias is not None:
            fc.bias.data.normal_()
        fcs.append(fc.to(DEV).requires_grad_(False))
    return fcs


@pytest.mark.parametrize('n', [1, 7])
@pytest.mark.parametrize('count', [1, 20])
@pytest.mark.parametrize('w_dim', [64, 100, 512])
def test_affine_batch(w_dim, count, n):
    """AffinePack on hand-built layer lists: rows that are no multiple of 4, one-row layers, a layer without bias, post-scales all 1
    (no scale vector) and not, latents x 1e-3 .. 1e3, contiguous and sliced (num_ws and batch) latents; element-wise
    |hip - fp64| <= gamma(ceil(w_dim / 64) + 8) (|ws| |W|^T + |b|) |scale|."""
    from torch_utils.ops import affine_batch
    for variant in range(2 if count == 1 else 1):
        fcs = _fc_layers(w_dim, count, variant, seed=w_dim + variant)
        assert sum(int(fc.weight.shape[0]) for fc in fcs) % 4 != 0 and any(fc.bias is None for fc in fcs) == (count > 1 or variant == 1)
        num_ws = count + 1
        index = [(3 * j + 1) % num_ws for j in range(count)]
        g = torch.Generator().manual_seed(n)
        for scale in (1e-3, 1.0, 1e3):
            for posts in ([1.0] * count, [1.0 if j % 3 == 0 else 1 / math.sqrt(3 + j) for j in range(count)] if count > 1 else [0.37]):
                for sliced in (False, True):
                    if sliced:
                        wide = (torch.randn(n + 2, num_ws + 3, w_dim, generator=g) * scale).to(DEV)
                        ws = wide[1:1 + n, 2:2 + num_ws]
                        assert ws.stride(0) == (num_ws + 3) * w_dim != num_ws * w_dim and ws.stride(2) == 1 and ws.data_ptr() != wide.data_ptr()
                    else:
                        ws = (torch.randn(n, num_ws, w_dim, generator=g) * scale).to(DEV)
                    pack = affine_batch.AffinePack()
                    outs = pack(ws, fcs, index, posts)
                    torch.cuda.synchronize()
                    assert (pack.scale is None) == all(p == 1.0 for p in posts) and len(outs) == count
                    for j, (fc, out) in enumerate(zip(fcs, outs)):
                        x = ws[:, index[j]]
                        ref, bound = S.affine_ref(x, fc.weight, fc.bias, fc.weight_gain, fc.bias_gain, posts[j])
                        got = out.double().cpu()
                        assert got.shape == ref.shape and out.is_contiguous()
                        q = float(((got - ref).abs() / bound).max())
                        note('affine_batch err/bound', q, f'w_dim {w_dim} layers {count} N {n} x{scale:g}')
                        assert q <= 1.0, (w_dim, count, n, scale, j, sliced, q)
                        t32 = (fc(x) * float(np.float32(posts[j]))).double().cpu()
                        e_t = float((t32 - ref).abs().max())
                        if e_t > 0:
                            note('affine_batch e_hip/e_torch32', float((got - ref).abs().max()) / e_t, f'w_dim {w_dim} layers {count} N {n} x{scale:g}')


# ------------------------------------------------------------------------------------------------------------- input_transform

BANDWIDTH, SAMPLING_RATE = 2.0, 16.0


def _zoomed(user, zoom):
    user = user.clone()
    user[..., :2, :2] *= zoom
    return user


def _transform_inputs(c, n, seed):
    g = torch.Generator().manual_seed(seed)
    freqs, phases = S.synth_freqs(c, BANDWIDTH, seed)
    ang = torch.rand(n, generator=g) * 6.2 - 3.1
    t = torch.stack([torch.cos(ang), torch.sin(ang), torch.rand(n, generator=g) * 100 - 50, torch.rand(n, generator=g) * 100 - 50], dim=1)
    t[0, 2], t[0, 3] = 50.0, -50.0
    users = [S.rotation_user(-33.0, 50.0, -7.5)]
    if n > 1:
        users.append(torch.stack([S.rotation_user(40.0 * i - 60, 25.0 * i - 50, 50.0 - 30 * i) for i in range(n)]))
    return freqs, phases, t, users


def _check_transform(got, t, user, freqs, phases, normalise, what):
    ref = S.input_transform_ref(t, user, freqs, phases, BANDWIDTH, SAMPLING_RATE, normalise)
    bounds = S.input_transform_bound(t, user, freqs, phases, BANDWIDTH, SAMPLING_RATE, normalise)
    t32 = S.input_transform_chain(t.to(DEV), user.to(DEV), freqs.to(DEV), phases.to(DEV), BANDWIDTH, SAMPLING_RATE, normalise, torch.float32)
    for name, a, r, b, c32 in zip(('freqs', 'phases', 'amps'), got, ref, bounds, t32):
        a = a.double().cpu()
        assert a.shape == r.shape and bool(torch.isfinite(a).all()), (what, name)
        q = float(((a - r).abs() / b).max())
        note(f'input_transform {name} err/bound', q, what)
        assert q <= 1.0, (what, name, q)
        e_t = float((c32.double().cpu() - r).abs().max())
        if e_t > 0:
            note(f'input_transform {name} e_hip/e_torch32', float((a - r).abs().max()) / e_t, what)
    return ref


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('c', [1, 255, 256, 257, 1024])
def test_input_transform(c, n):
    """[3,3] and [N,3,3] user transforms with rotations and translations up to +-50, t scaled to |t[:2]| = 1e-12, 1, 1e6 with
    `normalise`, already normalised without; zooms that put |f'| below the bandwidth (amplitude clamped to 1) and above
    sampling_rate / 2 (clamped to 0); element-wise bounds of style_stage_ref."""
    from torch_utils.ops import fourier_features as ff
    freqs, phases, t, users = _transform_inputs(c, n, seed=10 * c + n)
    for user in users:
        for zoom in (0.3, 1.0, 6.0):
            u = _zoomed(user, zoom)
            settings = [(t * scale, True) for scale in (1e-12, 1.0, 1e6)] + [(t, False)]
            for tt, normalise in settings:
                tt = tt.float()
                got = ff.input_transform(tt.to(DEV), u.to(DEV), freqs.to(DEV), phases.to(DEV), BANDWIDTH, SAMPLING_RATE, normalise)
                torch.cuda.synchronize()
                what = f'C {c} N {n} user {tuple(u.shape)} zoom {zoom} |t| {float(tt[0, :2].norm()):.0e} normalise {normalise}'
                ref = _check_transform(got, tt, u, freqs, phases, normalise, what)
                amps = ref[2]
                if zoom == 0.3:
                    assert bool((amps == 1).all())                       # |f'| <= 0.3 * bandwidth: below the band limit, clamped from above
                    assert bool((got[2] == 1).all())
                if zoom == 6.0 and c >= 255:
                    assert bool((amps == 0).any()) and bool((got[2] == 0).any())        # |f'| beyond sampling_rate / 2
                    assert bool(((amps > 0) & (amps < 1)).any())
            assert float(S.input_transform_ref(t, u, freqs, phases, BANDWIDTH, SAMPLING_RATE, False)[1].abs().max()) > (40 if c > 1 else 0)


@pytest.mark.parametrize('normalise', [True, False])
def test_input_transform_zero_rotation(normalise):
    """|t[:2]| = 0 (`normalise`: 0 / 0 and x / 0) or a NaN / inf handed in: the kernel's outputs are non-finite exactly where the torch
    chain's are, sample by sample; the other samples keep their bounds."""
    from torch_utils.ops import fourier_features as ff
    freqs, phases, t, users = _transform_inputs(257, 3, seed=9)
    t = t.clone()
    t[1] = torch.tensor([0.0, 0.0, 3.0, -4.0]) if normalise else torch.tensor([NAN, 1.0, float('inf'), 0.0])
    for user in users:
        got = ff.input_transform(t.to(DEV), user.to(DEV), freqs.to(DEV), phases.to(DEV), BANDWIDTH, SAMPLING_RATE, normalise)
        t32 = S.input_transform_chain(t.to(DEV), user.to(DEV), freqs.to(DEV), phases.to(DEV), BANDWIDTH, SAMPLING_RATE, normalise, torch.float32)
        for name, a, b in zip(('freqs', 'phases', 'amps'), got, t32):
            assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.isinf(a), torch.isinf(b)), (name, normalise)
            assert not bool(torch.isfinite(a[1]).any()) and bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[2]).all()), name
        keep = [0, 2]
        _check_transform([a[keep] for a in got], t[keep], user if user.ndim == 2 else user[keep], freqs, phases, normalise, 'next to a zero rotation')


# ------------------------------------------------------------------------------------------------------------ fourier_features

FOURIER_CASES = [(1, 1, 3, 1024), (15, 17, 2, 7), (16, 16, 1, 64), (1, 257, 1, 1), (36, 36, 3, 64), (5, 541, 1, 1), (36, 36, 1, 1024)]


@pytest.mark.parametrize('h,w,n,c', FOURIER_CASES, ids=['%dx%d_N%d_C%d' % k for k in FOURIER_CASES])
def test_fourier_features(h, w, n, c):
    """Plane sizes 1, 255, 256, 257, 36^2, 52^2 + 1 (non-square), N C from 1 to 3 x 1024; frequencies, phases and amplitudes as
    input_transform gives them for translations of 0, 5 and 50 image widths (|x + phase| up to hundreds of cycles), amplitude 0 and
    random per channel.  Element-wise |hip - fp64| <= |amp| (2 pi 5 u a + 4 u) + u |ref| with a = |gx f0| + |gy f1| + |phase|, and per
    tensor e_hip <= 2 e_torch32 + 1e-7 max |fp64|; whether the kernel still equals the torch chain bit for bit is printed."""
    from torch_utils.ops import fourier_features as ff
    freqs0, phases0 = S.synth_freqs(c, BANDWIDTH, seed=h * w + c)
    grid = S.sampling_grid(w, h, SAMPLING_RATE, DEV)
    assert tuple(grid.shape) == (h, w, 2) and grid.dtype == torch.float32
    width = w / SAMPLING_RATE
    g = torch.Generator().manual_seed(n * c)
    for widths in (0, 5, 50):
        ang = torch.arange(n, dtype=torch.float32) * 0.7 + 0.2
        t = torch.stack([torch.cos(ang), torch.sin(ang), torch.full([n], widths * width), torch.full([n], -0.5 * widths * width)], dim=1)
        f, ph, am = (a.float() for a in S.input_transform_ref(t, torch.eye(3), freqs0, phases0, BANDWIDTH, SAMPLING_RATE, False))
        for amp_kind in ('transform', 'zero', 'random'):
            amps = am if amp_kind == 'transform' else (torch.zeros(n, c) if amp_kind == 'zero' else torch.rand(n, c, generator=g) * 2 - 0.5)
            got = ff.fourier_features(grid, f.to(DEV), ph.to(DEV), amps.to(DEV))
            t32 = S.fourier_chain(grid, f.to(DEV), ph.to(DEV), amps.to(DEV), torch.float32).contiguous()
            torch.cuda.synchronize()
            ref = S.fourier_ref(grid.cpu(), f, ph, amps)
            bound = S.fourier_bound(grid.cpu(), f, ph, amps, ref)
            a = got.double().cpu()
            what = f'{h}x{w} N {n} C {c} {widths} widths amp {amp_kind}'
            assert a.shape == ref.shape == (n, c, h, w)
            err = (a - ref).abs()
            if amp_kind == 'zero':
                assert bool((got == 0).all()), what
            else:
                q = float((err / bound).max())
                note('fourier err/bound', q, what)
                assert q <= 1.0, (what, q)
            e_hip, e_t32 = float(err.max()), float((t32.double().cpu() - ref).abs().max())
            same = torch.equal(got, t32)
            cycles = float((ph.abs().max()))
            print(f'fourier {what}: largest |phase| {cycles:.1f} cycles, e_hip {e_hip:.3e} e_torch32 {e_t32:.3e}, bit-equal to the torch chain: {same}')
            note('fourier bit-equal to torch (1 = no)', 0.0 if same else 1.0, what)
            if e_t32 > 0:
                note('fourier e_hip/e_torch32', e_hip / e_t32, what)
            assert e_hip <= 2 * e_t32 + 1e-7 * float(ref.abs().max()), (what, e_hip, e_t32)
        if widths == 50 and w >= 36:
            assert float(ph.abs().max()) > 100, float(ph.abs().max())
