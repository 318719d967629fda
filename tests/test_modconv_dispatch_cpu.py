"""CPU: which kernel, tile and grid sg3_modulated_conv2d takes, per layer, without a GPU.

tests/golden/modconv_dispatch.json is a RECORDING of the launches (kernel name with template arguments, grid, workgroup, LDS bytes)
the library made for a fixed list of calls on a 256-CU device before its dispatch moved into csrc/sg3_modconv_plan.h (made by
tests/golden/make_modconv_dispatch.py): every layer of T-1024 and R-1024 with its data-gradient call at batch 1, 4 and 8, every shape
of the modconv GPU tests.  The host-only query sg3_modconv_dispatch -- the function the launch itself uses -- must reproduce it."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from helpers import HERE

ROOT = os.path.dirname(HERE)


def _lib():
    import torch  # noqa: F401  (loads torch's HIP runtime before ours)
    from torch_utils import _sg3abi
    return _sg3abi, _sg3abi.load()


@pytest.fixture(scope='module')
def table():
    with open(os.path.join(HERE, 'golden', 'modconv_dispatch.json')) as f:
        t = json.load(f)
    t['calls'] = [dict(zip(t['call_columns'], r)) for r in t['rows']]
    t['plans'] = [dict(zip(t['plan_columns'], r[len(t['call_columns']):])) for r in t['rows']]
    return t


def _elems(c):
    return c['N'] * c['O'] * (c['H'] + 2 * c['pad'] - c['k'] + 1) * (c['W'] + 2 * c['pad'] - c['k'] + 1)


def _params(abi, c):
    """The parameter block of a table call; tensors are placeholders (the queries follow no pointer)."""
    p = abi.ModconvParams()
    p.dcoef = 16 if c['dcoef'] else None
    p.epilogueBias = 16 if c['bias'] else None
    p.dtype, p.precision, p.outRowStride = c['dtype'], c['precision'], c['outRowStride']
    p.N, p.I, p.O, p.H, p.W, p.k, p.pad = c['N'], c['I'], c['O'], c['H'], c['W'], c['k'], c['pad']
    if c['scratch']:
        p.splitScratch, p.splitScratchFloats = 16, 4 * _elems(c)        # at most four partial images
    return p


def _dispatch(abi, lib, c, cus=256):
    info = abi.ModconvDispatchInfo()
    if 'forcedRows' in c:                                   # a table call: the recorded sg3_modconv_f23_force_rows setting
        prev = lib.sg3_modconv_f23_force_rows(c['forcedRows'])
    try:
        rc = lib.sg3_modconv_dispatch(ctypes.byref(_params(abi, c)), cus, ctypes.byref(info))
    finally:
        if 'forcedRows' in c:
            lib.sg3_modconv_f23_force_rows(prev)
    assert rc == 0, (c, lib.sg3_last_error())
    return {n: getattr(info, n) for n, _ in info._fields_}


def test_dispatch_reproduces_the_recorded_table(table):
    abi, lib = _lib()
    assert table['cus'] == 256 and len(table['rows']) > 2000
    for c, want in zip(table['calls'], table['plans']):
        got = _dispatch(abi, lib, c)
        for name, v in want.items():
            if name == 'outPitch' and v < 0:
                continue                                   # the recorded launcher left the field unset: its kernel does not read it
            assert got[name] == v, (c, name, got, want)
        if got['family'] != abi.SG3_MODCONV_TORGB:
            assert got['totalBlocks'] == got['xTiles'] * got['yTiles'] * got['mTiles'] * c['N'] * got['kSplits']


def test_scratch_query_is_the_plan_with_scratch_on_offer(table):
    """sg3_modconv_split_scratch_floats = kSplits partial images where the table says the call splits, else 0 (whether or not the
    parameter block offers scratch).  The query takes the CU count of the device, so the table holds where that is 256 -- every
    MI355X, and a machine without a GPU."""
    abi, lib = _lib()
    import torch
    if torch.cuda.is_available():
        assert torch.cuda.get_device_properties(0).multi_processor_count == 256
    splits = {}
    key = lambda c: tuple(v for n, v in c.items() if n not in ('scratch', 'forcedRows'))
    for c, pl in zip(table['calls'], table['plans']):
        splits[key(c)] = max(splits.get(key(c), 1), pl['kSplits'])
    assert sum(1 for v in splits.values() if v > 1) >= 20
    for c in table['calls']:
        k = splits[key(c)]
        assert lib.sg3_modconv_split_scratch_floats(ctypes.byref(_params(abi, c))) == (k * _elems(c) if k > 1 else 0), c


def _variants():
    """(dtype, k, family, WM, WN, TM, TN, SPLIT, PACK, NBUF, M16) of every kernel instantiation a default environment can reach: 80 of
    the 96 convolution kernels of the library (102 modconv symbols less the four prep kernels and the two reduce kernels).  The other 16:
    the twelve double-buffered 1x1 kernels with M16 = 0 need SG3_CONV1_MFMA32=1 (test_knobs_change_the_plan_as_documented walks all
    twelve), and the four NBUF = 1, M16 = 1 kernels are instantiated by the launch's `M16 ? a : b` but chosen by no plan."""
    out = set()
    for t in (0, 1):
        for ks in (3, 1):
            for tile in ((2, 2, 2, 2), (1, 4, 3, 1), (1, 4, 2, 2), (1, 4, 1, 4)):
                out.add((t, ks, 0) + tile + (0, 0, 0, 0))
        out.add((t, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0))
        for sp in (1, 0):
            rows = [(1, 4, 4, 0), (1, 4, 4, 1), (2, 2, 5, 0), (2, 2, 4, 0), (2, 2, 4, 1)]
            if not sp:
                rows += [(1, 4, 5, 0), (1, 4, 5, 1), (2, 2, 6, 0), (2, 2, 6, 1)]          # the tall stacks of the plain fp16 form
            for wm, wn, tn, pk in rows:
                out.add((t, 3, 2, wm, wn, 1, tn, sp, pk, 0, 0))
            for tn in (2, 3, 4):
                out.add((t, 3, 3, 2, 2, 1, tn, sp, 0, 0, 0))
            out.add((t, 1, 4, 1, 8, 2, 1, sp, 0, 1, 0))
            for tile in ((1, 8, 2, 1), (2, 4, 4, 2), (2, 4, 2, 2)):
                out.add((t, 1, 4) + tile + (sp, 0, 2, 1))                                 # M16 = 0: test_knobs (SG3_CONV1_MFMA32)
        for tn in (4, 5, 7):
            out.add((t, 3, 5, 2, 4, 1, tn, 1 - t, 0, 0, 0))
    return out


def test_table_reaches_every_kernel_variant(table):
    got = {(c['dtype'], c['k'], p['family'], p['WM'], p['WN'], p['TM'], p['TN'], p['SPLIT'], p['PACK'], p['NBUF'], p['M16'])
           for c, p in zip(table['calls'], table['plans'])}
    want = _variants()
    assert len(want) == 80
    assert got == want, (sorted(want - got), sorted(got - want))
    assert any(p['kSplits'] == 4 and p['family'] == 3 for p in table['plans']) and any(p['kSplits'] == 4 and p['family'] == 4 for p in table['plans'])


def test_dispatch_rejects_what_the_launch_rejects():
    abi, lib = _lib()
    good = dict(dtype=0, N=1, I=64, O=64, H=30, W=30, k=3, pad=2, precision=abi.SG3_CONV_F16X3, outRowStride=0, dcoef=1, bias=0, scratch=0)
    info = abi.ModconvDispatchInfo()
    assert lib.sg3_modconv_dispatch(ctypes.byref(_params(abi, good)), 0, ctypes.byref(info)) == 0 and info.family == abi.SG3_MODCONV_FLAT
    for bad in (dict(k=2), dict(pad=3), dict(dcoef=0), dict(precision=9), dict(bias=1), dict(outRowStride=31), dict(precision=abi.SG3_CONV_F16X3_F23, W=31),
                dict(N=0), dict(dtype=2)):
        assert lib.sg3_modconv_dispatch(ctypes.byref(_params(abi, dict(good, **bad))), 256, ctypes.byref(info)) == abi.SG3_BAD_ARG, bad
        assert lib.sg3_modconv_split_scratch_floats(ctypes.byref(_params(abi, dict(good, **bad)))) == 0
    assert lib.sg3_modconv_dispatch(None, 256, ctypes.byref(info)) == abi.SG3_BAD_ARG


_CHILD = '''
import ctypes, json, sys
sys.path[:0] = {paths!r}
sys.path.insert(0, {tests!r})
import test_modconv_dispatch_cpu as t
abi, lib = t._lib()
print(json.dumps([t._dispatch(abi, lib, c) for c in json.loads(sys.argv[1])]))
'''

_F16X3 = dict(dtype=0, k=3, pad=2, precision=1, outRowStride=0, dcoef=1, bias=0, scratch=1)
# the three double-buffered 1x1 tiles (64, 128 and 256 channels) in both arithmetic forms and tensor types: with SG3_CONV1_MFMA32 these
# are the twelve M16 = 0 instantiations no default environment reaches
_GEMM1 = [dict(_F16X3, k=1, pad=0, N=2, I=i, O=o, H=20, W=w, dtype=t, precision=pr)
          for i, o, w in ((300, 64, 20), (300, 300, 20), (645, 406, 23)) for t in (0, 1) for pr in (1, 2)]
# (id, variable, value, calls, plan fields without it, plan fields with it): what the knob's comment in csrc/sg3_modconv_plan.h says
KNOBS = [
    ('conv3_rows', 'SG3_CONV3_ROWS', '1', [dict(_F16X3, N=8, I=512, O=512, H=36, W=36)], dict(family=3), dict(family=2)),     # narrow 3x3 layers stay on the row tile
    ('flat_splits_never', 'SG3_FLAT_SPLITS', '1', [dict(_F16X3, N=1, I=512, O=512, H=36, W=36)], dict(kSplits=4), dict(kSplits=1)),
    ('flat_splits_always', 'SG3_FLAT_SPLITS', '2', [dict(_F16X3, N=8, I=512, O=512, H=36, W=36)], dict(kSplits=1), dict(kSplits=2)),
    ('f16_rows4', 'SG3_CONV_F16_ROWS4', '1', [dict(_F16X3, dtype=1, precision=2, N=1, I=64, O=128, H=131, W=134)], dict(family=2, TN=6), dict(family=2, TN=4)),
    ('conv1_mfma32', 'SG3_CONV1_MFMA32', '1', _GEMM1, dict(family=4, NBUF=2, M16=1), dict(family=4, NBUF=2, M16=0)),
    ('f23_tn', 'SG3_F23_TN', '5', [dict(_F16X3, precision=3, N=2, I=64, O=64, H=30, W=30)], dict(family=5, TN=4), dict(family=5, TN=5)),
]


@pytest.mark.parametrize('variable,value,calls,without,with_it', [k[1:] for k in KNOBS], ids=[k[0] for k in KNOBS])
def test_knobs_change_the_plan_as_documented(variable, value, calls, without, with_it):
    """The A/B switches are read once per process, so each runs in a child of its own."""
    abi, lib = _lib()
    base = [_dispatch(abi, lib, c) for c in calls]
    env = dict(os.environ)
    env[variable] = value
    code = _CHILD.format(paths=[p for p in sys.path if p], tests=HERE)
    out = subprocess.run([sys.executable, '-c', code, json.dumps(calls)], env=env, check=True, capture_output=True, text=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    assert len(got) == len(calls)
    for c, b, g in zip(calls, base, got):
        assert {n: b[n] for n in without} == without, c
        assert {n: g[n] for n in with_it} == with_it, c
        # nothing but the named coordinates (and the geometry that follows from them) moved
        assert [n for n in ('family', 'WM', 'WN', 'TM', 'SPLIT', 'PACK', 'NBUF') if g[n] != b[n] and n not in with_it] == [], c
    if variable == 'SG3_CONV1_MFMA32':
        assert len({(c['dtype'], g['WM'], g['TM'], g['SPLIT']) for c, g in zip(calls, got)}) == 12
