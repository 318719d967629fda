"""CPU: which kernel, tile and grid the encoder's plain convolutions take -- sg3_conv2d, sg3_conv2d_dgrad, sg3_conv2d_wgrad_sum --, per
call, without a GPU.

tests/golden/conv2d_dispatch.json is a RECORDING of the launches (kernel name with template arguments, grid, workgroup, LDS bytes, the
tile geometry handed to the kernel) the library made for a fixed list of calls before the choice moved into csrc/sg3_conv2d_plan.h,
and of what sg3_conv2d_form and sg3_conv2d_wgrad_sum_splits answered then (made by tests/golden/make_conv2d_dispatch.py): every
convolution of the IR-SE50 BackboneEncoder at 256 x 256, of the identity loss, of the ResNet34 blocks and of LPIPS at batch 1, 4 and
16 with their data and weight gradients, every shape of the GPU tests' case lists, and the one choice that reads the CU count on both
sides of its threshold under two CU counts.  The host-only queries sg3_conv2d_dispatch, sg3_conv2d_dgrad_dispatch and
sg3_conv2d_wgrad_sum_dispatch -- the functions the launches themselves use -- must reproduce it."""
import ctypes
import json
import os

import pytest

from helpers import HERE

FORWARD, DGRAD, WGRAD_SUM = 0, 1, 2                   # `entry` of a table call
CUS = 256


def _lib():
    import torch  # noqa: F401  (loads torch's HIP runtime before ours)
    from torch_utils import _sg3abi
    return _sg3abi, _sg3abi.load()


@pytest.fixture(scope='module')
def table():
    with open(os.path.join(HERE, 'golden', 'conv2d_dispatch.json')) as f:
        t = json.load(f)
    t['calls'] = [dict(zip(t['call_columns'], r)) for r in t['rows']]
    t['plans'] = [dict(zip(t['plan_columns'], r[len(t['call_columns']):])) for r in t['rows']]
    return t


def _out_hw(c):
    return (c['H'] + 2 * c['pad'] - c['k']) // c['stride'] + 1, (c['W'] + 2 * c['pad'] - c['k']) // c['stride'] + 1


def _params(abi, c):
    """The parameter block of a call; tensors are placeholders (the queries follow no pointer).  Besides the table's columns a call may
    name `act`, an `OH` of its own, and the pointers to leave out (`null`)."""
    from torch_utils._hip_plugins import PLACEHOLDER
    null = c.get('null', ())
    if c['entry'] == FORWARD:
        p = abi.Conv2dParams()
        p.x = p.wPacked = p.out = p.rangeFlag = p.wScale = PLACEHOLDER
        p.pad, p.precision, p.act = c['pad'], c['precision'], c.get('act', 0)
    elif c['entry'] == DGRAD:
        p = abi.Conv2dDgradParams()
        p.dy = p.wPacked = p.dx = PLACEHOLDER
        p.OH, p.OW = _out_hw(c)
        p.OH = c.get('OH', p.OH)
    else:
        p = abi.Conv2dWgradSumParams()
        p.x = p.dy = p.dw = p.partial = PLACEHOLDER
    p.N, p.I, p.O, p.H, p.W, p.k, p.stride = c['N'], c['I'], c['O'], c['H'], c['W'], c['k'], c['stride']
    for name in c.get('set', ()):
        setattr(p, name, PLACEHOLDER)
    for name in null:
        setattr(p, name, None)
    return p


def _dispatch(abi, lib, c, params=True):
    """(rc, plan as a dict) of the entry point's query"""
    info = abi.Conv2dDispatchInfo()
    p = ctypes.byref(_params(abi, c)) if params else None
    if c['entry'] == FORWARD:
        rc = lib.sg3_conv2d_dispatch(p, c.get('cus', CUS), ctypes.byref(info))
    elif c['entry'] == DGRAD:
        rc = lib.sg3_conv2d_dgrad_dispatch(p, ctypes.byref(info))
    else:
        rc = lib.sg3_conv2d_wgrad_sum_dispatch(p, ctypes.byref(info))
    return rc, info.as_dict()


def _splits(lib, c):
    out = [ctypes.c_int() for _ in range(3)]
    rc = lib.sg3_conv2d_wgrad_sum_splits(c['N'], c['I'], c['O'], c['H'], c['W'], c['k'], c['stride'], *[ctypes.byref(v) for v in out])
    return (rc,) + tuple(v.value for v in out)


def test_dispatch_reproduces_the_recorded_table(table):
    abi, lib = _lib()
    import torch
    if torch.cuda.is_available():                      # sg3_conv2d_form asks the device; the table's forms hold for 256 CUs (and for no device)
        assert torch.cuda.get_device_properties(0).multi_processor_count == CUS
    assert len(table['rows']) > 500
    kernel = ('family', 'KS', 'STRIDE', 'WM', 'WN', 'TM', 'TN', 'CHAINS')
    for c, want in zip(table['calls'], table['plans']):
        rc, got = _dispatch(abi, lib, c)
        assert rc == want['rc'], (c, rc, lib.sg3_last_error())
        if c['entry'] == FORWARD:
            # the older query does not look at the grid: it names the form of a call too large to launch as well
            assert got['form'] == want['form'], (c, got)
            if c['cus'] == CUS:
                assert lib.sg3_conv2d_form(ctypes.byref(_params(abi, c))) == want['form'], c
        if rc != 0:
            assert rc == abi.SG3_BAD_ARG and 'grid too large' in lib.sg3_last_error().decode(), c
            continue
        for name in kernel + ('block', 'ldsBytes'):
            assert got[name] == want[name], (c, name, got, want)
        assert got['totalBlocks'] == want['grid'], (c, got, want)
        if c['entry'] == WGRAD_SUM:
            for name in ('outH', 'outW', 'xSegs', 'nChunks', 'nSplit', 'chunksPerSplit', 'oTiles', 'iTiles', 'reduceGrid'):
                assert got[name] == want[name], (c, name, got, want)
            assert _splits(lib, c) == (0, want['nSplit'], want['chunksPerSplit'], want['xSegs']) == (0, got['nSplit'], got['chunksPerSplit'], got['xSegs']), c
            assert got['form'] == -1 and got['totalBlocks'] == got['oTiles'] * got['iTiles'] * got['nSplit'], (c, got)
            assert got['nChunks'] == c['N'] * got['outH'] * got['xSegs'] and (got['nSplit'] - 1) * got['chunksPerSplit'] < got['nChunks'] <= got['nSplit'] * got['chunksPerSplit']
            assert got['reduceGrid'] == (-(-c['O'] * c['I'] * c['k'] ** 2 // 256) if got['nSplit'] > 1 else 0), (c, got)
        else:
            for name in ('nch', 'xTiles', 'yTiles', 'mTiles'):
                assert got[name] == want[name], (c, name, got, want)
            assert (got['outH'], got['outW']) == _out_hw(c), (c, got)
            reduced = c['O'] if c['entry'] == DGRAD else c['I']           # the K dimension: dy's channels | x's channels
            assert got['nch'] == -(-reduced // got['kc']) and got['kc'] == (16 if got['family'] == abi.SG3_CONV2D_F16X3 or c['k'] == 1 else 8), (c, got)
            assert got['classes'] == (c['stride'] ** 2 if c['entry'] == DGRAD else 0) and (c['entry'] == FORWARD or got['form'] == -1), (c, got)
            assert got['totalBlocks'] == got['xTiles'] * got['yTiles'] * got['mTiles'] * c['N'] * max(got['classes'], 1), (c, got)
    assert sum(p['rc'] != 0 for p in table['plans']) == 3


def test_the_cu_count_moves_one_choice(table):
    """3x3 stride 1 on the split kernel above 16 rows: the 4-row tile (form 20) below two eight-row tiles per CU, the 8-row tile (21)
    from there on.  The table holds a call just below and one exactly at the threshold of each CU count, each under both counts."""
    seen = {}
    for c, p in zip(table['calls'], table['plans']):
        if c['entry'] == FORWARD and p['form'] in (20, 21):
            tiles8 = c['N'] * -(-c['O'] // 64) * -(-_out_hw(c)[0] // 8) * -(-_out_hw(c)[1] // 32)
            assert p['form'] == (20 if tiles8 < 2 * c['cus'] else 21) and p['TN'] == p['form'] - 19, (c, p)
            seen.setdefault(c['cus'], set()).add(tiles8 - 2 * c['cus'])
    assert all({-1, 0} <= seen[cus] for cus in (256, 128)), seen
    abi, lib = _lib()
    call = dict(entry=FORWARD, N=64, I=16, O=64, H=64, W=32, k=3, stride=1, pad=1, precision=abi.SG3_CONV_F16X3)
    assert _dispatch(abi, lib, dict(call, cus=0))[1] == _dispatch(abi, lib, dict(call, cus=CUS))[1]      # no device, or an MI355X: 256


def _variants():
    """(family, KS, STRIDE, WM, WN, TM, TN, CHAINS) of every kernel instantiation the three launches hold: per (k, stride) the three
    tiles of the exact-fp32 forward with one accumulation chain and the two with four, the 4-row tile of the split forward (and its
    8-row tile for 3x3 stride 1), the two tiles of the data gradient, and the weight gradient -- 20 + 5 + 8 + 4."""
    out = set()
    for ks in (1, 3):
        for s in (1, 2):
            out |= {(0, ks, s) + tile + (1,) for tile in ((2, 2, 2, 2), (2, 2, 1, 1), (1, 4, 1, 1))}
            out |= {(0, ks, s) + tile + (4,) for tile in ((2, 2, 1, 1), (1, 4, 1, 1))}
            out.add((1, ks, s, 1, 4, 2, 1, 0))
            out |= {(2, ks, s) + tile + (0,) for tile in ((2, 2, 1, 1), (1, 4, 1, 1))}
            out.add((3, ks, s, 0, 0, 0, 0, 0))
    out.add((1, 3, 1, 1, 4, 2, 2, 0))
    return out


def _variant(p):
    return tuple(p[k] for k in ('family', 'KS', 'STRIDE', 'WM', 'WN', 'TM', 'TN', 'CHAINS'))


def test_table_reaches_every_kernel_variant(table):
    want = _variants()
    assert len(want) == 37
    got = {_variant(p) for p in table['plans'] if p['rc'] == 0}
    assert got == want, (sorted(want - got), sorted(got - want))


def test_gpu_case_lists_reach_every_kernel():
    """The case lists of the GPU tests against the kernels they are there to cover, by the plan of each case (at 256 CUs):
    DGRAD_SHAPES all eight data-gradient kernels, WGRAD_SHAPES the four weight-gradient kernels each with one split and with several,
    _form_cases() every form of the forward."""
    abi, lib = _lib()
    import encoder_train_cases
    import test_gpu_encoder_numerics as numerics
    import test_gpu_id_loss

    def plan(entry, n, i, o, h, w, k, s, pad=None, precision=0):
        rc, got = _dispatch(abi, lib, dict(entry=entry, N=n, I=i, O=o, H=h, W=w, k=k, stride=s, pad=k // 2 if pad is None else pad, precision=precision))
        assert rc == 0
        return got

    dgrad = {_variant(plan(DGRAD, 2, i, o, h, w, k, s)) for k, s, i, o, h, w in test_gpu_id_loss.DGRAD_SHAPES}
    assert dgrad == {v for v in _variants() if v[0] == abi.SG3_CONV2D_DGRAD} and len(dgrad) == 8
    wgrad = {(p['KS'], p['STRIDE'], p['nSplit'] > 1) for p in (plan(WGRAD_SUM, 2, i, o, h, w, k, s) for k, s, i, o, h, w in encoder_train_cases.WGRAD_SHAPES)}
    assert wgrad == {(k, s, several) for k in (1, 3) for s in (1, 2) for several in (False, True)}
    saved, numerics._cus = numerics._cus, lambda: CUS
    try:
        cases = numerics._form_cases()
        split_shapes = numerics._split_form_shapes()
    finally:
        numerics._cus = saved
    forms = {plan(FORWARD, n, ci, co, h, w, k, s, pad, prec)['form'] for n, ci, co, h, w, k, s, pad, *_ in cases for prec in (abi.SG3_CONV_FP32, abi.SG3_CONV_F16X3)}
    assert forms == set(range(12)) | {abi.SG3_CONV2D_FORM_F16X3 + j for j in range(6)}
    assert [plan(FORWARD, *c, precision=abi.SG3_CONV_F16X3)['form'] for c in split_shapes] == [abi.SG3_CONV2D_FORM_F16X3 + j for j in range(6)]


def test_dispatch_rejects_what_the_launch_rejects():
    abi, lib = _lib()
    shape = dict(N=2, I=40, O=70, H=13, W=9, k=3, stride=2, pad=1)
    good = {FORWARD: dict(shape, entry=FORWARD, precision=abi.SG3_CONV_F16X3), DGRAD: dict(shape, entry=DGRAD), WGRAD_SUM: dict(shape, entry=WGRAD_SUM)}
    bad = {FORWARD: [dict(k=2), dict(stride=3), dict(N=0), dict(precision=9), dict(null=('rangeFlag',)), dict(null=('wScale',)), dict(act=1), dict(pad=3),
                     dict(null=('x',)), dict(precision=abi.SG3_CONV_FP32, act=3)],
           DGRAD: [dict(k=2), dict(stride=3), dict(N=0), dict(OH=8), dict(set=('act',)), dict(null=('dx',))],
           WGRAD_SUM: [dict(k=2), dict(stride=3), dict(N=0), dict(set=('inScale',)), dict(set=('inShift',)), dict(null=('partial',)), dict(null=('dw',))]}
    for entry, call in good.items():
        rc, got = _dispatch(abi, lib, call)
        assert rc == 0 and got['totalBlocks'] > 0, (call, lib.sg3_last_error())
        for edit in bad[entry]:
            assert _dispatch(abi, lib, dict(call, **edit))[0] == abi.SG3_BAD_ARG, (entry, edit)
        assert _dispatch(abi, lib, call, params=False)[0] == abi.SG3_BAD_ARG
    # what an edit above takes away is all that was wrong with it
    assert _dispatch(abi, lib, dict(good[FORWARD], act=1, set=('slope',)))[0] == 0
    assert _dispatch(abi, lib, dict(good[DGRAD], set=('act', 'slope')))[0] == 0
    assert _dispatch(abi, lib, dict(good[WGRAD_SUM], set=('inScale', 'inShift')))[0] == 0
    assert lib.sg3_conv2d_form(ctypes.byref(_params(abi, dict(good[FORWARD], k=2)))) == abi.SG3_BAD_ARG
    assert lib.sg3_conv2d_dispatch(ctypes.byref(_params(abi, good[FORWARD])), CUS, None) == abi.SG3_BAD_ARG
    assert _splits(lib, dict(shape, k=2))[0] == abi.SG3_BAD_ARG and _splits(lib, dict(shape, N=0))[0] == abi.SG3_BAD_ARG
