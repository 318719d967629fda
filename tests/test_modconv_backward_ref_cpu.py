"""CPU: the float64 references of tests/modconv_backward_ref.py equal float64 autograd through the reference formulation
(`modulated_conv._composite`), and the abs-Jacobian bound of the modulation chain rule dominates the exact one."""
import itertools

import pytest
import torch

import modconv_backward_ref as R

CASES = [(k, pad, n, demod, gain) for k, pad, n, demod, gain in itertools.product(
    (1, 3), (0, 1, 2), (1, 2, 3), (True, False), (None, 'scalar', 'per_channel', 'per_sample')) if pad <= k - 1]


def _case(k, n, gain, seed):
    g = torch.Generator().manual_seed(seed)
    ci, co, h, w = 5, 4, 7, 6
    x = torch.randn([n, ci, h, w], generator=g, dtype=torch.float64)
    wt = torch.randn([co, ci, k, k], generator=g, dtype=torch.float64)
    s = torch.randn([n, ci], generator=g, dtype=torch.float64) + 1.0
    ig = {None: None, 'scalar': torch.tensor(0.7, dtype=torch.float64),
          'per_channel': torch.rand([ci], generator=g, dtype=torch.float64) + 0.5,
          'per_sample': torch.rand([n, ci], generator=g, dtype=torch.float64) + 0.5}[gain]
    return x, wt, s, ig, g


@pytest.mark.parametrize('k,pad,n,demod,gain', CASES)
def test_references_equal_autograd_through_the_composite(k, pad, n, demod, gain):
    from torch_utils.ops import modulated_conv as mc
    x, w, s, ig, g = _case(k, n, gain, seed=7 + 3 * k + pad + 11 * n)
    xr, wr, sr = (t.clone().requires_grad_(True) for t in (x, w, s))
    y = mc._composite(xr, wr, sr, demod, pad, ig)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dx_a, dw_a, ds_a = torch.autograd.grad(y, [xr, wr, sr], dy)
    w_eff = R.effective_weights64(w, s, demod, ig)
    # dW_eff: autograd of the last step of the composite (the grouped convolution) with respect to each sample's weights
    for j in range(n):
        we = w_eff[j].clone().requires_grad_(True)
        yj = mc._composite(x[j:j + 1], we, torch.ones([1, w.shape[1]], dtype=torch.float64), False, pad, None)
        (ref_j,) = torch.autograd.grad(yj, [we], dy[j:j + 1])
        assert torch.allclose(R.wgrad_ref(x, dy, k, pad)[j], ref_j, rtol=1e-12, atol=1e-12)
        # abs scale of the weight gradient: the same GEMMs on |x|, |dy|
        yj = mc._composite(x[j:j + 1].abs(), we, torch.ones([1, w.shape[1]], dtype=torch.float64), False, pad, None)
        (abs_j,) = torch.autograd.grad(yj, [we], dy[j:j + 1].abs())
        assert torch.allclose(R.abs_scale(x=x, dy=dy, k=k, pad=pad)[j], abs_j, rtol=1e-12, atol=1e-12)
    assert torch.allclose(R.dgrad_ref(dy, w_eff, k, pad), dx_a, rtol=1e-12, atol=1e-12)
    dw, ds = R.modgrad_ref(R.wgrad_ref(x, dy, k, pad), w, s, demod, ig)
    assert torch.allclose(dw, dw_a, rtol=1e-10, atol=1e-12) and torch.allclose(ds, ds_a, rtol=1e-10, atol=1e-12)
    # abs scale of the data gradient: autograd of the composite on |dy| with |w_eff|
    xa = x.clone().requires_grad_(True)
    ya = torch.cat([mc._composite(xa[j:j + 1], w_eff[j].abs(), torch.ones([1, w.shape[1]], dtype=torch.float64), False, pad, None)
                    for j in range(n)])
    (dx_abs,) = torch.autograd.grad(ya, [xa], dy.abs())
    assert torch.allclose(R.abs_scale(dy=dy, w_eff=w_eff, k=k, pad=pad), dx_abs, rtol=1e-12, atol=1e-12)
    # the window form used for the transform-domain kernel: the same plane with extra columns on both sides
    ext = R.dgrad_ref(dy, w_eff, k, pad, extra_cols=3)
    assert torch.allclose(ext[..., 3:-3], dx_a, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('demod,gain,n', [(True, 'scalar', 2), (True, 'per_sample', 3), (False, 'per_channel', 2), (True, None, 1)])
def test_modgrad_abs_dominates_the_exact_abs_jacobian(demod, gain, n):
    """modgrad_abs(a) >= |J|^T a for the exact Jacobian J of dW_eff -> (dw, ds): the stage-wise abs bound is a valid bound
    (and not a loose one: its sum within 4x of the exact abs-Jacobian product's)."""
    k = 3
    x, w, s, ig, g = _case(k, n, gain, seed=40 + n)
    a = torch.rand([n, w.shape[0], w.shape[1], k, k], generator=g, dtype=torch.float64)

    def f(wv, sv):
        return R.effective_weights64(wv, sv, demod, ig)
    jw, js = torch.autograd.functional.jacobian(f, (w, s))
    exact_w = torch.einsum('abcdeopqr,abcde->opqr', jw.abs(), a)
    exact_s = torch.einsum('abcdemi,abcde->mi', js.abs(), a)
    bw, bs = R.modgrad_abs(a, w, s, demod, ig)
    assert bool((bw >= exact_w * (1 - 1e-12)).all()) and bool((bs >= exact_s * (1 - 1e-12)).all())
    print(f'modgrad_abs / exact: dw {float(bw.sum() / exact_w.sum()):.2f}, ds {float(bs.sum() / exact_s.sum()):.2f} (sums)')
    assert float(bw.sum() / exact_w.sum()) <= 4 and float(bs.sum() / exact_s.sum()) <= 4


def test_wgrad_terms_counts_the_roundings_of_one_workgroup():
    # 1044 rows in 116 bands of 9 rows, 33 segments in 4 groups of 9 (288 columns): 3 MFMAs per 16 pixels + 16 + 464 partials
    assert R.wgrad_terms(1044, 1044, 3, 116, 4) == 3 * (9 * 288) // 16 + 16 + 464
    assert R.pow2_scale(32768.0) == 1.0 and R.pow2_scale(32769.0) == 0.5 and R.pow2_scale(3e-6) == 2.0 ** 33
