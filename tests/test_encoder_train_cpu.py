"""CPU: the algebra and the host-side plan behind training the encoder trunk.  The residual unit's training backward, restated in
plain float64 tensor algebra the way `_ResidualUnit.backward_train` orders it (encoder_train_cases.unit_train_algebra), agrees with
float64 autograd of `_ResidualUnit.forward` in train mode; the K splits of sg3_conv2d_wgrad_sum cover every pixel exactly once."""
import pytest
import torch

import encoder_train_cases as cases


@pytest.mark.parametrize('kind', ['ir', 'ir_se'])
@pytest.mark.parametrize('in_channel,depth,stride', [(16, 16, 1), (16, 16, 2), (16, 32, 2), (16, 32, 1)])
def test_unit_training_backward_algebra_matches_autograd(kind, in_channel, depth, stride):
    """BatchNorm backward formulas, the slope gradient, the squeeze-and-excitation weight gradients and the three shortcut kinds
    (identity, strided identity, projection): 1e-12 relative to each tensor's maximum."""
    unit = cases.make_unit(kind, in_channel, depth, stride, seed=11 + stride, negative_slopes=True)
    x = cases.randn(5, 2, in_channel, 9, 7)
    oh, ow = cases.out_hw(9, 7, 3, stride)
    dout = cases.randn(6, 2, depth, oh, ow)
    out_r, dx_r, g_r = cases.unit_autograd(unit, x, dout)
    with torch.no_grad():
        out_a, dx_a, g_a = cases.unit_train_algebra(unit, x, dout)
    assert sorted(g_a) == sorted(g_r) == sorted(n for n, _ in unit.named_parameters())

    def close(a, b):
        return float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())

    assert close(out_a, out_r) and close(dx_a, dx_r)
    for name in g_r:
        assert g_a[name].shape == g_r[name].shape and close(g_a[name], g_r[name]), name
    if kind == 'ir_se':                                  # the gate's hidden ReLU is alive, so fc1 really receives a gradient
        assert float(g_r['res_layer.5.fc1.weight'].abs().max()) > 0


@pytest.mark.parametrize('n', [2, 3])
@pytest.mark.parametrize('k,stride,I,O,H,W', cases.WGRAD_SHAPES + [(3, 1, 64, 64, 256, 256), (3, 2, 256, 512, 32, 32), (1, 2, 256, 512, 32, 32)])
def test_wgrad_sum_splits_cover_every_pixel_once(n, k, stride, I, O, H, W):
    from torch_utils.ops import plain_conv_wgrad
    n_split, per, x_segs = plain_conv_wgrad.splits(n, I, O, H, W, k, stride)
    oh, ow = cases.out_hw(H, W, k, stride)
    assert x_segs == -(-ow // (32 // stride)) and n_split >= 1 and per >= 1
    assert (n_split - 1) * per < n * oh * x_segs <= n_split * per                  # no empty split, nothing left over
    assert bool((cases.split_cover(n, H, W, k, stride, n_split, per, x_segs) == 1).all())
    assert plain_conv_wgrad.splits(n, I, O, H, W, k, stride) == (n_split, per, x_segs)
