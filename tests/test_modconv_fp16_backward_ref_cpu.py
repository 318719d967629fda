"""CPU: the arithmetic of tests/modconv_fp16_backward_ref.py itself -- its references on fp16-rounded operands against float64 autograd
of `modulated_conv._composite`, the fp16 grid of its bounds against numpy.float16, its row table against the host-only dispatch query,
and its float64 network against the product's own CPU forward."""
import itertools

import numpy as np
import pytest
import torch

import modconv_backward_ref as R
import modconv_fp16_backward_ref as H


def _case(k, n, gain, seed, ci=5, co=4, h=7, w=6):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn([n, ci, h, w], generator=g) * 20).clamp(-256, 256).half()
    wt = torch.randn([co, ci, k, k], generator=g)
    s = torch.randn([n, ci], generator=g) + 1.0
    ig = {None: None, 'scalar': torch.tensor(0.7), 'per_channel': torch.rand([ci], generator=g) + 0.5,
          'per_sample': torch.rand([n, ci], generator=g) + 0.5}[gain]
    return x, wt, s, ig


@pytest.mark.parametrize('k,n,demod,gain,m', [c for c in itertools.product((1, 3), (1, 3), (True, False), (None, 'scalar', 'per_channel', 'per_sample'),
                                                                          H.MAGNITUDES)])
def test_references_on_fp16_operands_equal_float64_autograd_of_the_composite(k, n, demod, gain, m):
    from torch_utils.ops import modulated_conv as mc
    x, w, s, ig = _case(k, n, gain, seed=11 + k + 5 * n)
    pad = k - 1
    dy64 = H.lattice_dy([n, w.shape[0], x.shape[2] + k - 1, x.shape[3] + k - 1], seed=3) * m
    dy = dy64.half()
    assert torch.equal(dy.double(), dy64) and float(dy64.abs().max()) == m                # the sweep's gradients are fp16 values
    xr, sr = x.double().requires_grad_(True), s.double().requires_grad_(True)
    y = mc._composite(xr, w.double(), sr, demod, pad, None if ig is None else ig.double())
    dx_a, ds_a = torch.autograd.grad(y, [xr, sr], dy.double())
    dx = R.dgrad_ref(dy, R.effective_weights64(w, s, demod, ig), k, pad)
    assert torch.allclose(dx, dx_a, rtol=1e-12, atol=1e-12 * m)
    (_, b_dw), (ds, b_ds) = H.style_grad_refs(x, dy, w, s, demod, ig, k, pad, 256.0, m)
    assert torch.allclose(ds, ds_a, rtol=1e-10, atol=1e-12 * m)
    assert bool((b_ds > 0).all()) and bool((b_dw > 0).all()) and float((b_ds / ds_a.abs().max()).max()) < 1e-3


def test_half_spacing_is_numpy_float16_spacing():
    v = np.concatenate([np.exp2(np.arange(-30, 16, dtype=np.float64)), np.exp2(np.arange(-30, 15, dtype=np.float64)) * 1.75,
                        np.random.RandomState(0).uniform(-4, 4, 4096) * np.exp2(np.random.RandomState(1).randint(-26, 13, 4096)), [0.0, 65472.0]])
    got = H.f16_half_spacing(torch.from_numpy(v)).numpy()
    want = np.spacing(np.abs(v).astype(np.float16)).astype(np.float64) / 2
    # numpy's spacing is taken at the ROUNDED value, which for v just below a power of two is the binade above: never smaller
    down = np.abs(v).astype(np.float16).astype(np.float64) >= np.exp2(np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14))) + 1)
    assert np.array_equal(got[~down], want[~down]) and np.array_equal(2 * got[down], want[down])
    # the floor: half a step of the subnormal grid
    assert float(H.f16_half_spacing(torch.zeros(1, dtype=torch.float64))) == float(np.spacing(np.float16(0))) / 2 == 2.0 ** -25
    assert float(H.f16_half_spacing(torch.tensor([2.0 ** -14 * (1 - 2.0 ** -12)], dtype=torch.float64))) == 2.0 ** -25
    assert float(H.f16_half_spacing(torch.tensor([2.0 ** -14], dtype=torch.float64))) == 2.0 ** -25                # first normal binade: the same step
    assert float(H.f16_half_spacing(torch.tensor([2.0 ** -13], dtype=torch.float64))) == 2.0 ** -24
    # and it IS what a store can move a value by
    t = torch.from_numpy(v[np.abs(v) < 65504])
    assert bool(((t.half().double() - t).abs() <= H.f16_half_spacing(t)).all())


def test_dgrad_bound_scales_with_the_unit_and_ends_on_the_fp16_grid():
    ref = torch.from_numpy(np.random.RandomState(2).uniform(1.0, 3.5, [2, 3, 5, 5])) * torch.tensor([1.0, -1.0]).reshape(2, 1, 1, 1)
    b1, m1 = H.fp16_dgrad_bound(ref, 1.0)
    assert float(b1.min()) >= 4e-3 * 3.0 and float(b1.max()) <= 4e-3 * 3.5 + 2.0 ** -10 and m1 <= 4e-4 * 3.5 + 2.0 ** -10
    for m in (2.0 ** 10, 2.0 ** -10):                                   # m * ref stays in fp16's normal range: the bound is m x the bound at 1
        bm, mm = H.fp16_dgrad_bound(ref * m, m)
        assert torch.equal(bm, b1 * m) and mm == m1 * m
    m = 2.0 ** -20                                                      # m * ref <= 2^-18: what is left is the subnormal grid
    bm, mm = H.fp16_dgrad_bound(ref * m, m)
    rel = 4e-3 * m * float(ref.abs().max())
    assert torch.equal(bm, torch.full_like(bm, rel + 2.0 ** -25)) and mm == 4e-4 * m * float(ref.abs().max()) + 2.0 ** -25
    assert rel < 2.0 ** -25 / 2                                          # the relative part is a fraction of the grid there
    assert H.unit_of(1.0) == 1.0 and H.unit_of(1.999) == 1.0 and H.unit_of(3e-6) == 2.0 ** -19 and H.unit_of(2.0 ** -20) == 2.0 ** -20


@pytest.mark.parametrize('name', sorted(H.DGRAD_ROWS))
def test_row_table_names_the_plan_of_each_backward_launch(name):
    """Without a GPU: the exchanged-role call of every row takes the form, family and tile the table says, on a 256-CU device."""
    import torch  # noqa: F401  (loads torch's HIP runtime before the library)
    row, want = H.DGRAD_ROWS[name]
    assert H.host_plan(H.backward_call(row)) == want, (name, H.host_plan(H.backward_call(row)))


def test_row_table_covers_every_fp16_form_of_the_backward():
    got = {(w[0], w[1]) for _, w in H.DGRAD_ROWS.values()}
    assert got == {(H.CONV_F16, H.ROWS), (H.CONV_F16, H.FLAT), (H.CONV_F16, H.GEMM1), (H.CONV_F16_F23, H.F23)}
    torgb = [r for r, _ in H.DGRAD_ROWS.values() if r[2] == 3 and r[5] == 1 and not r[6]]
    assert torgb and all(H.backward_call(r)[1] == 3 for r in torgb)                       # K = 3 in the adjoint


@pytest.mark.parametrize('cfg', ['Tmini', 'Rmini'])
def test_float64_network_is_the_products_network(cfg):
    """`synthesis_fp64` against the product's own CPU forward and autograd (fp32, the same composite ops): an error of the float64
    restatement -- a missing gain, a transposed transform -- is of order one; fp32 rounding through 15 layers moves the image by order
    1e-6, and the gradient by more: it is discontinuous where a leaky-ReLU sign or a clamp decision flips under that rounding (the
    1x1 layers of config R, whose activations sit closer to zero, show 8e-4), so the gradient is held to 1e-2 only."""
    from helpers import build_product_generator
    from synth_weights import synth_ws
    G = build_product_generator(cfg)
    ws = torch.from_numpy(synth_ws(2, G.num_ws, G.w_dim, seed=3))
    g = torch.from_numpy(np.random.RandomState(5).randn(2, 3, 64, 64).astype(np.float32))
    w32 = ws.clone().requires_grad_(True)
    img32 = G.synthesis(w32, noise_mode='const', force_fp32=True)
    (g32,) = torch.autograd.grad((img32 * g).sum(), w32)
    w64 = ws.double().requires_grad_(True)
    img64 = H.synthesis_fp64(G.synthesis, w64)
    assert img64.dtype == torch.float64
    (g64,) = torch.autograd.grad((img64 * g.double()).sum(), w64)
    e_img = float((img32.detach().double() - img64.detach()).abs().max()) / float(img64.detach().abs().max())
    e_g = float((g32.double() - g64).abs().max()) / float(g64.abs().max())
    print(f'{cfg}: fp32 vs float64 network, relative to the largest entry: image {e_img:.2e}, d/dws {e_g:.2e}')
    assert e_img <= 1e-4 and e_g <= 1e-2 and float(g64.abs().max()) > 0
