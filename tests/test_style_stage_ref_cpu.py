"""CPU: the float64 references of tests/style_stage_ref.py against the product's own modules run in float64, and the conditions on
the test inputs that tests/test_gpu_style_stage_fp64.py relies on."""
import contextlib

import numpy as np
import pytest
import torch

import style_stage_ref as S


@contextlib.contextmanager
def default_float64():
    """The modules build identities with torch.eye(3) / torch.eye(2, 3) in the default dtype: float64 for the duration."""
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(torch.float32)


def _close(a, b, rel=1e-12):
    a, b = a.double(), b.double()
    assert a.shape == b.shape
    assert bool(((a - b).abs() <= rel * b.abs() + 1e-300).all()), float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('gain_mode', [0, 1, 2, 3])
@pytest.mark.parametrize('demodulate', [True, False])
def test_prep_ref_is_the_effective_weight(demodulate, gain_mode, k):
    """w_eff[n,o,i] of the reference formulation (modulated_conv._effective_weights, float64) == wn[o,i] * v[n,i] * d[n,o]."""
    from torch_utils.ops import modulated_conv as mc
    c = S.make_case(3, 17, 33, k, demodulate, gain_mode, S.CONV_F16X3, 3.0, small_sample=True, seed=5 + gain_mode)
    s, gain = S.case_styles(c)
    w, s = torch.from_numpy(S.case_weights(c)), torch.from_numpy(s)
    gain = None if gain is None else torch.from_numpy(gain)
    r = S.prep_ref(w, s, demodulate, None if gain is None else (gain.reshape([]) if gain_mode == 1 else gain), 3.0, S.CONV_F16X3)
    w_eff = mc._effective_weights(w.double(), s.double(), demodulate, None if gain is None else (gain.reshape([]) if gain_mode == 1 else gain).double(), 3)
    mine = r['wn'].unsqueeze(0) * r['v'][:, None, :, None, None] * r['d'][:, :, None, None, None]
    _close(mine, w_eff)
    _close(r['wsq'], r['wn'].square().sum([2, 3]))
    if not demodulate:
        assert bool((r['d'] == 1).all()) and torch.equal(r['wn'], w.double())


def test_prep_ref_exponent():
    """e = ceil(log2(peak / 2^15)) brings the peak into (2^14, 2^15]; one more for the transform-domain forms; 0 for fp32; kept within
    +-E_LIMIT; the constructed cases sit on the power of two exactly."""
    for c in S.all_exponent_cases():
        pk = S.case_peaks(c)
        s, gain = S.case_styles(c)
        r = S.prep_ref(torch.zeros(1, c['I'], 1, 1) + 1, torch.from_numpy(s), c['demodulate'], None if gain is None else torch.from_numpy(gain),
                       c['x_bound'], c['precision'])
        assert np.allclose(r['peak'], pk, rtol=1e-14, atol=0)
        if c['precision'] == S.CONV_FP32:
            assert (r['e'] == 0).all()
            continue
        top = 14 if c['precision'] in S.F23_FORMS else 15
        scaled = pk * 2.0 ** (-r['e'].astype(np.float64))
        assert ((scaled > 2.0 ** (top - 1)) & (scaled <= 2.0 ** top)).all(), (c['id'], scaled)
        assert (np.abs(r['e_kept']) <= S.E_LIMIT).all() and ((r['e_kept'] == r['e']) | (np.abs(r['e']) > S.E_LIMIT)).all()
        if 'exact_j' in c:
            assert (r['e'] == c['exact_j']).all() and (scaled == 2.0 ** top).all()
    assert all((S.prep_ref(torch.ones(1, 70, 1, 1), torch.from_numpy(S.case_styles(c)[0]), c['demodulate'], None, c['x_bound'],
                           c['precision'])['e'] < -S.E_LIMIT).all() for c in S.tiny_cases() if c['gain_mode'] == 0)


def test_no_exponent_case_sits_near_a_power_of_two():
    """The GPU tests read the exponent off the kernel's output and compare it with the exact one: the fp32 peak (a relative error of a
    few 1e-6, and log2f's) must not be able to land on the other side of a power of two.  1e-4 relative is kept (1e-5 would do);
    the constructed cases are the exception, on purpose."""
    worst = 1.0
    cases = S.all_exponent_cases()
    for c in cases:
        if c['precision'] == S.CONV_FP32:
            continue
        dist = min(S.pow2_distance(float(p)) for p in S.case_peaks(c))
        if 'exact_j' in c:
            assert dist == 0.0
        else:
            worst = min(worst, dist)
            assert dist >= 1e-4, (c['id'], dist)
    print(f'{len(cases)} cases, closest peak to a power of two: {worst:.2e} relative')
    ids = [c['id'] for c in cases]
    assert len(set(ids)) == len(ids)


def test_cases_cover_what_the_issue_lists():
    cases = S.shape_cases()
    assert {c['I'] for c in cases} == set(S.PREP_I) and {c['O'] for c in cases} == set(S.PREP_O)
    for k in (1, 3):
        sub = [c for c in cases if c['k'] == k]
        assert {c['N'] for c in sub} == {1, 3} and {c['demodulate'] for c in sub} == {True, False}
        assert {c['gain_mode'] for c in sub} == {0, 1, 2, 3} and {c['bound_on_device'] for c in sub} == {True, False}
        assert {c['precision'] for c in sub} == (set(range(5)) if k == 3 else {0, 1, 2})
        assert {c['I'] for c in sub if c['O'] == 513} >= {1, 17, 64, 70, 257}              # the gy = 16 tail at many I
    assert all(c['I'] * c['O'] * c['k'] ** 2 <= S.MAX_WEIGHT_ELEMENTS for c in cases)
    assert any(c['I'] == 1024 and c['O'] == 1024 for c in cases)
    for sh in S.VARIATION_SHAPES:
        v = S.variation_cases(sh)
        combos = {(c['demodulate'], c['gain_mode'], c['precision'], c['bound_on_device']) for c in v}
        precs = 5 if sh[3] == 3 else 3
        assert len(combos) == len(v) == 2 * 4 * (1 + 2 * (precs - 1))
    for sh in S.MAGNITUDE_SHAPES:
        m = S.magnitude_cases(sh)
        assert {(c['style_scale'], c['weight_scale'], c['x_bound'], c['demodulate']) for c in m} == \
            {(a, b, float(np.float32(x)), d) for a in S.PREP_STYLE_SCALES for b in S.PREP_WEIGHT_SCALES for x in S.PREP_XBOUNDS for d in (True, False)}
        # the 1e-8 of the demodulation matters for the small sample: it moves d by more than the bound on d
        c = next(c for c in m if c['demodulate'] and c['style_scale'] == 1.0 and c['weight_scale'] == 1.0)
        s, gain = S.case_styles(c)
        r = S.prep_ref(torch.from_numpy(S.case_weights(c)), torch.from_numpy(s), True, None, 1.0, S.CONV_FP32)
        without = (r['d'] ** -2 - 1e-8).rsqrt()
        if sh[1] == 1:
            assert float(((without - r['d']).abs() / r['d'])[-1].min()) > 100 * S.prep_bounds(c['N'], c['I'], c['k'], True, True)[2]


def test_prep_bounds_stay_below_the_error_they_must_expose():
    """A 1e-5 relative error in a per-(n, o) scalar must exceed every bound (the largest shape has the loosest one)."""
    for k in (1, 3):
        for demod in (True, False):
            b = S.prep_bounds(3, 1024, k, demod, True)
            assert max(b) < 5e-6, b
    assert S.prep_bounds(3, 70, 3, False, False)[1] == 0.0            # plain styles pass through untouched


@pytest.mark.parametrize('w_dim', [64, 100])
def test_affine_ref_is_the_fully_connected_layer(w_dim):
    """affine_ref against FullyConnectedLayer.double(): exactly (1e-12) where weight_gain = 1 / sqrt(w_dim) is a power of two, so that
    fp32(weight * gain) is the float64 product too; within the two roundings that separate them (the gain to fp32, the product)
    elsewhere."""
    from models.stylegan3.networks_stylegan3 import FullyConnectedLayer
    torch.manual_seed(w_dim)
    for bias, post in ((True, 1.0), (False, 0.125), (True, 1 / np.sqrt(300.0))):
        fc = FullyConnectedLayer(w_dim, 37, bias=bias, bias_init=1.0)
        ws = torch.randn(5, w_dim)
        ref, bound = S.affine_ref(ws, fc.weight, fc.bias, fc.weight_gain, fc.bias_gain, post)
        mod = fc.double()(ws.double()).detach() * float(np.float32(post))
        if w_dim == 64:
            _close(ref, mod)
        else:
            slack = 2 * 2.0 ** -24 * (ws.double().abs() @ (fc.weight.detach().double() * fc.weight_gain).abs().t()) * abs(post) * 1.001
            assert bool(((ref - mod).abs() <= slack).all())
        assert bool((bound > 0).all()) and float((bound / ref.abs().clamp_min(1e-3)).median()) < 1e-5


@pytest.mark.parametrize('batched_user', [False, True])
def test_input_chain_is_the_synthesis_input(batched_user):
    """input_transform_chain + fourier_chain + the channel mix == SynthesisInput.forward in float64 (the module run with float64 as the
    default dtype, so that its identities are float64 too); `normalise` == SynthesisInput.transform_params."""
    from models.stylegan3.networks_stylegan3 import SynthesisInput
    torch.manual_seed(3)
    inp = SynthesisInput(w_dim=32, channels=12, size=[10, 7], sampling_rate=8.0, bandwidth=2.0)
    inp.affine.weight.data.normal_()
    user = torch.stack([S.rotation_user(20.0 * i + 5, 0.3 * i, -0.2) for i in range(3)]) if batched_user else S.rotation_user(-33.0, 4.0, -7.5)
    w = torch.randn(3, 32)
    with default_float64(), torch.no_grad():
        inp = inp.double()
        inp.transform = user.double()
        t_raw = inp.affine(w.double())
        t = inp.transform_params(w.double())
        x_mod = inp(None, t=t)
        grid = S.sampling_grid(10, 7, 8.0)
        assert grid.dtype == torch.float64 and tuple(grid.shape) == (7, 10, 2)
    for tt, normalise in ((t, False), (t_raw, True)):
        f, ph, am = S.input_transform_ref(tt, user, inp.freqs, inp.phases, 2.0, 8.0, normalise)
        assert f.dtype == torch.float64 and 0 < float(am.min()) and float(am.max()) <= 1
        x = S.fourier_ref(grid, f, ph, am)
        x = (x.permute(0, 2, 3, 1) @ (inp.weight.detach() / np.sqrt(12)).t()).permute(0, 3, 1, 2)
        assert float((x - x_mod).abs().max()) <= 1e-12 * float(x_mod.abs().max())


def test_input_transform_bound_holds_for_the_fp32_chain_on_the_cpu():
    """The element-wise bound is derived for the kernel's order of operations; the module's fp32 chain on the CPU is another fp32
    evaluation of the same short sums and stays inside it too -- a bound of the wrong size (a unit off, a missing term) shows here
    without a GPU.  The Fourier bound likewise."""
    f0, p0 = S.synth_freqs(257, 2.0, 1)
    t = torch.tensor([[0.6, -0.8, 50.0, -3.0], [3.0, 4.0, -20.0, 45.0], [-1e-3, 2e-3, 0.5, 0.25]])
    user = S.rotation_user(30.0, -50.0, 12.0)
    for normalise in (True, False):
        ref = S.input_transform_ref(t, user, f0, p0, 2.0, 16.0, normalise)
        got = S.input_transform_chain(t, user, f0, p0, 2.0, 16.0, normalise, torch.float32)
        for g, r, b, name in zip(got, ref, S.input_transform_bound(t, user, f0, p0, 2.0, 16.0, normalise), ('freqs', 'phases', 'amps')):
            ratio = float(((g.double() - r).abs() / b).max())
            print(f'normalise {normalise} {name}: fp32 chain error / bound = {ratio:.3f}')
            assert ratio <= 1.0
    f, ph, am = (a.float() for a in S.input_transform_ref(t[:2], user, f0, p0, 2.0, 16.0, True))
    grid = S.sampling_grid(17, 15, 16.0)
    ref = S.fourier_ref(grid, f, ph, am)
    got = S.fourier_chain(grid, f, ph, am, torch.float32)
    ratio = float(((got.double() - ref).abs() / S.fourier_bound(grid, f, ph, am, ref).clamp_min(1e-300)).max())
    print(f'fourier: fp32 chain error / bound = {ratio:.3f}, largest argument {float(ph.abs().max()):.0f} cycles')
    assert ratio <= 1.0 and float(ph.abs().max()) > 100
