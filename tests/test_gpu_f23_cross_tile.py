"""The cross-tile pipeline of the transform-domain 3x3 convolution (csrc/sg3_modconv_f23.hip): a persistent workgroup's K loop runs
on from tile to tile -- the last iteration of a tile stages chunk 0 of the next one and requests its chunk 1, the output transform
runs with those requests in flight, and only the workgroup's first tile has a prologue.

Shape (n, ci, 80, 246, 218, pad 2): 7 column tiles with a ragged last one, 18 row tiles at TN = 7 with a ragged last one, 2 M tiles
of which the second has 16 real channels and one inactive M block: 252 tiles per sample.  Batch 4 is 1008 tiles, 3-4 per workgroup
on 256 CUs; batch 1 is 252 tiles, one per workgroup, i.e. only the first-tile prologue path.  ci = 16, 17, 48, 64 gives 1, 2, 3 and
4 chunks per tile: with one or two chunks a request two chunks ahead crosses one or two tile boundaries, and an odd chunk count
flips the buffer / register-set parity from tile to tile.

Tile heights: TN = 7 takes the cross-tile pipeline (its B image holds the 64 KB exchange area); TN = 4 / 5 and the fp16 form stay on
the per-tile flow, which runs through the same request cursors, so they are walked here as well.

Tolerance: relative max error vs the fp64 oracle <= 5e-6, the bound of test_gpu_f23.py; everything else is bit-identity."""
import functools

import numpy as np
import pytest
import torch

from golden_cases import rand
from helpers import maxabs
from test_gpu_f23 import DEV, T, _f23

pytestmark = pytest.mark.gpu

N, CO, H, W, PAD = 4, 80, 246, 218, 2
CIS = [16, 17, 48, 64]
KW = dict(demodulate=True, padding=PAD, x_bound=256.0)


@functools.lru_cache(maxsize=None)
def _inputs(ci):
    """Inputs of one case on the device, its fp64 reference, and the replacement for sample 0 of the leakage test: different data of
    100 x the magnitude, inside the same x_bound.  Computed once, shared, never modified."""
    from oracle import oracle as O
    x = np.clip(rand(71, N, ci, H, W) * 0.5, -2.56, 2.56).astype(np.float32)
    wt = rand(72, CO, ci, 3, 3); s = rand(73, N, ci) + 1
    ref = O.modulated_conv2d(x.astype(np.float64), wt.astype(np.float64), s.astype(np.float64), True, PAD, 0.8)
    big = np.clip(rand(74, 1, ci, H, W) * 50, -256, 256).astype(np.float32)
    return T(x), T(wt), T(s), ref, T(big)


@functools.lru_cache(maxsize=None)
def _run(ci, tn, n=N):
    """The demodulating call on the first n samples at tile height tn; computed once per case, shared, never modified."""
    x, wt, s, _, _ = _inputs(ci)
    with _f23('on', tn) as mc, torch.no_grad():
        return mc.modulated_conv2d(x[:n], wt, s[:n], input_gain=torch.tensor(0.8, device=DEV), **KW)


def _took_f23(ci, dtype=None):
    from torch_utils import _sg3abi as abi
    return abi.load().sg3_modconv_f23_supported(dtype or abi.SG3_F32, ci, CO, H, W, 3, PAD, 0) == 1


@pytest.mark.parametrize('tn', [7, 5, 4])
@pytest.mark.parametrize('ci', CIS)
def test_multi_tile_walk_matches_fp64(ci, tn):
    assert _took_f23(ci)
    ref = _inputs(ci)[3]
    y = _run(ci, tn)
    assert tuple(y.shape) == ref.shape
    err = maxabs(y.cpu().numpy(), ref) / max(1.0, float(np.abs(ref).max()))
    print(f'ci {ci} ({(ci + 15) // 16} chunks) TN {tn}: relative max error vs fp64 {err:.2e}')
    assert err <= 5e-6, err


@pytest.mark.parametrize('tn', [7, 5, 4])
@pytest.mark.parametrize('ci', CIS)
def test_batch_four_is_bit_identical_to_one_tile_per_workgroup(ci, tn):
    """both[k] of the batch-4 call (several tiles per workgroup) against the batch-1 call on sample k (252 tiles: one per workgroup,
    the first-tile prologue only).  demodulate=False here: the style normalisation of the demodulating call spans the batch."""
    x, wt, s, _, _ = _inputs(ci)
    with _f23('on', tn) as mc, torch.no_grad():
        both = mc.modulated_conv2d(x, wt, s, demodulate=False, padding=PAD, x_bound=256.0)
        for k in range(N):
            one = mc.modulated_conv2d(x[k:k + 1], wt, s[k:k + 1], demodulate=False, padding=PAD, x_bound=256.0)
            assert torch.equal(one[0], both[k]), k


@pytest.mark.parametrize('n', [4, 3])
@pytest.mark.parametrize('ci', CIS)
def test_no_leakage_between_tiles(ci, n):
    """Sample 0 replaced by other data of 100 x the magnitude: the other samples keep every bit.  With n = 4 each XCD's share of the
    tile order lies inside one sample; with n = 3 (756 tiles, 94-95 per XCD) the workgroups of one XCD walk from sample 0 into
    sample 1 and those of another from sample 1 into sample 2."""
    x, wt, s, _, big = _inputs(ci)
    before = _run(ci, 7, n)
    x2 = torch.cat([big, x[1:n]], dim=0)
    with _f23('on', 7) as mc, torch.no_grad():
        after = mc.modulated_conv2d(x2, wt, s[:n], input_gain=torch.tensor(0.8, device=DEV), **KW)
    assert not torch.equal(after[0], before[0])
    for k in range(1, n):
        assert torch.equal(after[k], before[k]), k


def test_fp16_form_walks_the_tiles():
    """The fp16 operand form comes from the same template (ci = 48: three chunks), against the direct fp16 kernel and the oracles with
    the bounds of test_f23_fp16_form_matches_the_direct_fp16_kernel_and_the_oracles."""
    from oracle import oracle as O
    from torch_utils import _sg3abi as abi
    ci = 48
    x = np.clip(rand(171, N, ci, H, W) * 40, -256, 256).astype(np.float16)
    wt = rand(172, CO, ci, 3, 3); s = (rand(173, N, ci) + 1).astype(np.float32)
    ref64 = O.modulated_conv2d(x.astype(np.float64), wt.astype(np.float64), s.astype(np.float64), True, PAD, 0.8)
    ref16 = O.modulated_conv2d_fp16(x, wt, s, True, PAD, 0.8).astype(np.float64)
    scale = max(1.0, float(np.abs(ref64).max()))
    kw = dict(input_gain=torch.tensor(0.8, device=DEV), **KW)
    assert _took_f23(ci, abi.SG3_F16)
    with _f23('on', 7) as mc:
        y = mc.modulated_conv2d(T(x), T(wt), T(s), **kw)
        one = mc.modulated_conv2d(T(x[1:2]), T(wt), T(s[1:2]), demodulate=False, padding=PAD, x_bound=256.0)
        both = mc.modulated_conv2d(T(x), T(wt), T(s), demodulate=False, padding=PAD, x_bound=256.0)
    with _f23('off') as mc:
        yd = mc.modulated_conv2d(T(x), T(wt), T(s), **kw)
    assert y.dtype == torch.float16 and tuple(y.shape) == ref64.shape and bool(torch.isfinite(y).all())
    assert torch.equal(one[0], both[1])
    y64, yd64 = y.float().cpu().numpy().astype(np.float64), yd.float().cpu().numpy().astype(np.float64)
    e23, ed, eo = maxabs(y64, ref64) / scale, maxabs(yd64, ref64) / scale, maxabs(ref16, ref64) / scale
    m23, md = float(np.abs(y64 - ref64).mean()) / scale, float(np.abs(yd64 - ref64).mean()) / scale
    print(f'vs fp64, relative to max |y|: transform-domain fp16 max {e23:.2e} mean {m23:.2e}; direct fp16 max {ed:.2e} mean {md:.2e}; fp16 oracle max {eo:.2e}')
    assert e23 <= 4e-3 and m23 <= 4e-4, (e23, m23)
    assert e23 <= 3.0 * max(ed, eo) + 2.5e-4 and m23 <= 3.0 * md + 1e-5, (e23, ed, eo, m23, md)
