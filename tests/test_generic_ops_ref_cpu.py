"""CPU: the float64 references of tests/generic_ops_ref.py pinned to the reference implementation's recorded results, and their
bounds to reality (no GPU, no libsg3hip kernel).

- `upfirdn_ref` / `bias_act_def` reproduce every upfirdn/* and bias_act/* vector of tests/golden/ops.npz: the reference's fp32
  results lie inside `upfirdn_bound`, resp. inside 2 e_formulas32 + 1e-7 max|ref|.
- `bias_act_formulas` evaluated in float64 equals `bias_act_def` (value, first and second derivative) to 1e-12 away from the cut-offs.
- The fp32 CPU run of the package's impl='ref' path stays inside `upfirdn_bound` for the GPU test's cases: the bound is not vacuous.
- The share conditions of the GPU test (elements left out of bias_act's gradient checks, clamped share) hold on its inputs.
"""
import numpy as np
import pytest
import torch

import generic_ops_ref as G
from golden_cases import BIAS_ACT_CASES, UPFIRDN_CASES, make_filter, rand
from helpers import golden, product_design


def _f(spec):
    f = make_filter(spec, product_design)
    return None if f is None else torch.from_numpy(f)


# ------------------------------------------------------------------------------------------------------------------ upfirdn2d

@pytest.mark.parametrize('name', sorted(UPFIRDN_CASES))
def test_upfirdn_ref_reproduces_the_golden_vectors(name):
    c = UPFIRDN_CASES[name]
    x = torch.from_numpy(rand(21, *c['shape']))
    kw = dict(up=c['up'], down=c['down'], padding=c['padding'], flip=c['flip'], gain=c['gain'])
    ref = G.upfirdn_ref(x, _f(c['f']), **kw)
    gold = torch.from_numpy(golden('ops')['upfirdn/' + name]).double()
    assert tuple(ref.shape) == tuple(gold.shape)
    r = G.ratio((gold - ref).abs(), G.upfirdn_bound(x, _f(c['f']), dtype=torch.float32, **kw))
    print(f'upfirdn/{name}: reference fp32 result, worst err/bound {r:.3f}')
    assert r <= 1.0


@pytest.mark.parametrize('name', sorted(G.UPFIRDN_BIG_CASES))
def test_fp32_cpu_run_stays_inside_upfirdn_bound(name):
    """The package's own impl='ref' path (a float32 convolution over the zero-stuffed image) on the GPU test's cases, forward and
    x.grad; the largest one is cropped to its first 200 rows to keep the zero-stuffed convolution short."""
    from torch_utils.ops import upfirdn2d
    c = G.UPFIRDN_BIG_CASES[name]
    x = G.upfirdn_input(name)
    if name == 'radial_dn2':
        x = x[:, :, :200].contiguous()
    f = _f(c['f'])
    if c.get('layout') == 'f_transposed':
        f = f.t().contiguous()
    for flip in c['flips']:
        for gain in c['gains']:
            kw = dict(up=c['up'], down=c['down'], padding=c['padding'], flip=flip, gain=gain)
            xs = x.clone().requires_grad_(True)
            y = upfirdn2d.upfirdn2d(xs, f, up=c['up'], down=c['down'], padding=c['padding'], flip_filter=flip, gain=gain, impl='ref')
            ref = G.upfirdn_ref(x, f, **kw)
            assert tuple(y.shape) == tuple(ref.shape)
            r = G.ratio((y.detach().double() - ref).abs(), G.upfirdn_bound(x, f, dtype=torch.float32, **kw))
            gy = torch.from_numpy(rand(7, *y.shape))
            (y * gy).sum().backward()
            # the adjoint: float64 autograd of the reference, equal to the reference run with the adjoint's geometry
            x64 = x.double().requires_grad_(True)
            (G.upfirdn_ref(x64, f, **kw) * gy.double()).sum().backward()
            aup, adown, apad, aflip = G.adjoint_geometry(tuple(x.shape[2:]), tuple(y.shape[2:]), f, c['up'], c['down'], c['padding'], flip)
            akw = dict(up=aup, down=adown, padding=apad, flip=aflip, gain=gain)
            adj = G.upfirdn_ref(gy, f, **akw)
            assert tuple(adj.shape) == tuple(x.shape)
            assert float((adj - x64.grad).abs().max()) <= 1e-13 * max(1.0, float(adj.abs().max()))
            ra = G.ratio((xs.grad.double() - adj).abs(), G.upfirdn_bound(gy, f, dtype=torch.float32, **akw))
            print(f'{name} flip={flip} gain={gain}: impl=ref fp32 on the CPU, worst err/bound forward {r:.3f} adjoint {ra:.3f}')
            assert r <= 1.0 and ra <= 1.0
            assert r >= 1e-3 or c['f'] is None                  # not vacuous: within three orders of what fp32 does on as few as six outputs


def test_upfirdn_bound_sees_float32_tap_staging_in_float64():
    """Taps scaled by a gain that is no power of two and rounded to fp32 before a float64 sum -- what the kernel did before it
    multiplied the sum by the gain -- lie far outside the float64 bound; with gain 4 they are exact."""
    c = UPFIRDN_CASES['asym_conv']
    x = torch.from_numpy(rand(21, *c['shape'])).double()
    f = _f(c['f'])
    for gain, outside in ((1.7, True), (4.0, False)):
        kw = dict(up=c['up'], down=c['down'], padding=c['padding'], flip=False)
        staged = (f * np.float32(gain)).float()
        got = G.upfirdn_ref(x, staged, gain=1.0, **kw)
        r = G.ratio((got - G.upfirdn_ref(x, f, gain=gain, **kw)).abs(), G.upfirdn_bound(x, f, gain=gain, dtype=torch.float64, **kw))
        assert (r > 1e6) if outside else (r <= 1.0), (gain, r)


# ------------------------------------------------------------------------------------------------------------------- bias_act

def _e(a, ref):
    return float((a.double() - ref).abs().max())


@pytest.mark.parametrize('name', sorted(BIAS_ACT_CASES))
def test_bias_act_def_reproduces_the_golden_vectors(name):
    c = BIAS_ACT_CASES[name]
    x = torch.from_numpy(rand(31, *c['shape']) * 2)
    b = torch.from_numpy(rand(32, c['shape'][c['dim']])) if c['bias'] else None
    kw = dict(dim=c['dim'], act=c['act'], alpha=c['alpha'], gain=c['gain'], clamp=c['clamp'])
    ref = G.bias_act_def(x, b, **kw)
    e_gold = _e(torch.from_numpy(golden('ops')['bias_act/' + name]), ref)
    e_f32 = _e(G.bias_act_formulas32(x, b, **kw), ref)
    print(f'bias_act/{name}: e_reference {e_gold:.3e}  e_formulas32 {e_f32:.3e}  max|ref| {float(ref.abs().max()):.3e}')
    assert e_gold <= 2 * e_f32 + 1e-7 * float(ref.abs().max())


@pytest.mark.parametrize('act', G.ACTS)
@pytest.mark.parametrize('gain', G.BIAS_ACT_GAINS)
def test_formulas_in_float64_equal_the_definition(act, gain):
    """y, gx, gb, ggx of the formulas in float64 against float64 autograd of the definition: 1e-12 relative to max|ref|, away from the
    cut-offs (|x + b| <= 30: no +-80 / 40 branch is taken and e^x stays far from the float64 range)."""
    r = np.random.RandomState(5)
    x = torch.from_numpy(r.randn(37, 41) * np.array([1e-3, 1.0, 8.0])[np.arange(37) % 3][:, None])
    b = torch.from_numpy(0.5 * r.randn(41))
    w, v1, v2 = torch.from_numpy(r.randn(37, 41)), torch.from_numpy(r.randn(37, 41)), torch.from_numpy(r.randn(41))
    clamp = None if act == 'linear' else G.BIAS_ACT_CLAMP
    got = G.bias_act_chain(x, b, 1, act, G.BIAS_ACT_ALPHA, gain, clamp, w, v1, v2, dtype=torch.float64)
    ref = G.bias_act_chain_def(x, b, 1, act, G.BIAS_ACT_ALPHA, gain, clamp, w, v1, v2)
    for nm, a, d in zip(('y', 'gx', 'gb', 'ggx'), got, ref):
        assert _e(a, d) <= 1e-12 * max(1.0, float(d.abs().max())), (act, nm, _e(a, d))


@pytest.mark.parametrize('shape', sorted(G.BIAS_ACT_SHAPES))
def test_bias_act_share_conditions(shape):
    """From the float64 definition alone, on the GPU test's inputs: the share of elements left out of the gradient checks is at most
    1e-4 (fp32) and 2e-3 (fp16), and between 15 % and 90 % of the elements are clamped for every activation and gain (the mask is
    exercised both ways)."""
    _, _, dim, _ = G.BIAS_ACT_SHAPES[shape]
    x, b, *_ = G.bias_act_inputs(shape)
    for dtype, cap in ((torch.float32, 1e-4), (torch.float16, 2e-3)):
        xd, bd = x.to(dtype), b.to(dtype)
        for act in G.ACTS:
            if act == 'linear':
                continue
            for gain in G.BIAS_ACT_GAINS:
                free = G.bias_act_def(xd, bd, dim, act, G.BIAS_ACT_ALPHA, gain, None)
                share = float(G.clamp_window(free, G.BIAS_ACT_CLAMP, dtype).double().mean())
                clamped = float((free.abs() >= G.BIAS_ACT_CLAMP).double().mean())
                assert share <= cap, (shape, dtype, act, gain, share)
                assert 0.15 <= clamped <= 0.9, (shape, act, gain, clamped)


# -------------------------------------------------------------------------------------------------------- filtered_lrelu_act_

def test_act_ref_and_codes_agree():
    x = torch.from_numpy(rand(3, 2, 3, 9, 21) * 2)
    for dtype in (torch.float32, torch.float64):
        v = G.act_ref(x, 1.5, 0.2, 1.0, dtype)
        code = G.act_codes(x, 1.5, 0.2, 1.0, dtype)
        assert v.dtype == dtype and code.dtype == torch.uint8
        assert bool(((code == 2) == (v.abs() == 1.0)).all()) and bool(((code == 1) == ((x < 0) & (v.abs() < 1.0))).all())
        assert bool((G.act_ref(x, 1.5, 0.2, None, dtype).abs() >= v.abs()).all())
        read = G.act_read_ref(torch.ones_like(x), code, 1.5, 0.2, dtype)
        want = torch.where(code == 2, 0.0, torch.where(code == 1, 1.5 * 0.2, 1.5)).to(dtype)
        assert float((read - want).abs().max()) <= 1e-7
        outside = G.act_read_ref(torch.ones_like(x), torch.full_like(code, 255), 1.5, 0.2, dtype)
        assert bool((outside == torch.tensor(G.f32(1.5), dtype=dtype)).all())


# ------------------------------------------------------------------------------------------- the generic flrelu composition

@pytest.mark.parametrize('name', sorted(n for n, c in G.FLRELU_GENERIC_CASES.items() if c['dtypes'] != ('float64',)))
def test_generic_flrelu_cases_have_no_fused_kernel(name):
    """Every fp32 / fp16 case of the GPU test is refused by the fused kernels, forward and adjoint (host-only query)."""
    from torch_utils import _sg3abi
    c = G.FLRELU_GENERIC_CASES[name]
    fu, fd = _f(c['fu']), _f(c['fd'])
    dims = lambda f: (1, 1) if f is None else ((int(f.shape[1]), int(f.shape[0])) if f.ndim == 2 else (int(f.shape[0]), 0))   # noqa: E731
    lib = _sg3abi.load()
    assert lib.sg3_filtered_lrelu_has_kernel(c['up'], c['down'], *dims(fu), *dims(fd)) == 0
    assert lib.sg3_filtered_lrelu_has_kernel(c['down'], c['up'], *dims(fd), *dims(fu)) == 0


def test_generic_counts_of_flrelu_ref():
    """The generic composition's rounding counts, on a case by hand, and the existing (fused) counts untouched by the new argument."""
    import flrelu_ref as R
    c = G.FLRELU_GENERIC_CASES['up3_dn2']
    ops = R.Ops(90, 140, _f(c['fu']), _f(c['fd']), 3, 2, c['padding'], False, 'cpu')
    assert ops.generic_u() == (1 + 2 * 3 + 2, 1 + 2)             # bias, ceil(9 / 3) taps per axis + 2; stores: x + b, two passes
    assert ops.generic_down() == (2 * 7 + 2, 1)
    assert ops.generic_adjoint() == (2 * 4 + 2, 2, 2 * 9 + 2, 1)
    c = G.FLRELU_GENERIC_CASES['both_2d']
    ops = R.Ops(60, 70, _f(c['fu']), _f(c['fd']), 2, 2, c['padding'], False, 'cpu')
    assert ops.generic_u() == (1 + 3 * 2 + 2, 2) and ops.generic_down() == (15 + 2, 0)
    x, b = G.flrelu_inputs('both_2d')
    kw = dict(up=2, down=2, padding=c['padding'], gain=c['gain'], slope=c['slope'], clamp=c['clamp'], flip=False)
    y64, _ = R.forward_ref(x, b, _f(c['fu']), _f(c['fd']), **kw)
    by, bu = R.forward_bounds(x, b, _f(c['fu']), _f(c['fd']), generic=True, **kw)
    by64, _ = R.forward_bounds(x, b, _f(c['fu']), _f(c['fd']), generic=True, unit=2.0 ** -53, **kw)
    assert float((by64 / by).max()) <= 2.0 ** -28 and float(by.min()) > 0
    # the package's fp32 CPU composition lies inside the generic bound
    from torch_utils.ops import filtered_lrelu as fl
    y = fl.filtered_lrelu(x, _f(c['fu']), _f(c['fd']), b, up=2, down=2, padding=c['padding'], gain=c['gain'], slope=c['slope'], clamp=c['clamp'], impl='ref')
    r = R.ratio((y.double() - y64).abs(), by)
    print(f'both_2d: impl=ref fp32 on the CPU against the generic bound: {r:.3f}')
    assert 0.0 < r <= 1.0
