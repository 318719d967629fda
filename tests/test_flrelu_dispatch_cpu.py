"""CPU: which kernel, how many launches and what grid sg3_filtered_lrelu takes, per call, without a GPU.

tests/golden/flrelu_dispatch.json is a RECORDING of the launches (kernel name with template arguments, grid, workgroup, the work
decomposition handed to the kernel) the library made for a fixed list of calls before the choice moved into csrc/sg3_flrelu_plan.h, and
of what its host queries answered then (made by tests/golden/make_flrelu_dispatch.py): every layer of T-1024 and R-1024 at batch 1, 4
and 8 in fp32 and fp16 -- plain, sign-writing and the adjoint call --, every filtered_lrelu shape of the GPU tests, the A/B knobs, and
the calls the library refuses.  The host-only query sg3_filtered_lrelu_dispatch -- the function the launch itself uses -- must
reproduce it."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

from helpers import HERE

ROOT = os.path.dirname(HERE)
STREAM_COORDS = ('U', 'D', 'VPH', 'RADIAL', 'SIGNS', 'G', 'WIDE')
DENSE, CHANNELS_LAST, EVERY_SECOND_SAMPLE = 0, 1, 2                 # `layout` of a table call
KNOB_NONE, KNOB_NOPACK, KNOB_SLOWACT, KNOB_UP4_WIDE = 0, 1, 2, 3    # `knob` of a table call


def _lib():
    import torch  # noqa: F401  (loads torch's HIP runtime before ours)
    from torch_utils import _sg3abi
    return _sg3abi, _sg3abi.load()


def _load_table():
    """The table, one entry per call: calls that differ in the tensor type or in the adjoint's partials alone and were recorded with the
    same result share a row (`dtypes` / `partials`: the values as bits); a row ends after the launches it has, and the second launch
    names only what differs from the first (make_flrelu_dispatch.py::compact)."""
    with open(os.path.join(HERE, 'golden', 'flrelu_dispatch.json')) as f:
        t = json.load(f)
    nc, nq, nl = len(t['call_columns']), len(t['query_columns']), len(t['launch_columns'])
    t['calls'], t['queries'], t['launches'] = [], [], []
    for r in t['rows']:
        row, q = dict(zip(t['call_columns'], r)), dict(zip(t['query_columns'], r[nc:]))
        assert len(r) == nc + nq + (nl if q['launches'] else 0) + (len(t['second_launch_columns']) if q['launches'] == 2 else 0), r
        launches = [dict(zip(t['launch_columns'], r[nc + nq:]))] if q['launches'] else []
        if q['launches'] == 2:
            launches.append(dict(launches[0], **dict(zip(t['second_launch_columns'], r[nc + nq + nl:]))))
        dtypes, partials = row.pop('dtypes'), row.pop('partials')
        assert 1 <= dtypes <= 3 and 1 <= partials <= 3, r
        for dtype in (d for d in (0, 1) if dtypes >> d & 1):
            for part in (v for v in (0, 1) if partials >> v & 1):
                t['calls'].append(dict(row, dtype=dtype, partials=part))
                t['queries'].append(q)
                t['launches'].append(launches)
    return t


@pytest.fixture(scope='module')
def table():
    return _load_table()


def _params(c):
    """The parameter block of a table call, filled as the binding fills it; tensors are placeholders (the queries follow no pointer)."""
    from torch_utils._hip_plugins import PLACEHOLDER, dense_strides, filtered_lrelu_params
    n, ch = c['N'], c['C']
    xs, ys = dense_strides(n, ch, c['xH'], c['xW']), dense_strides(n, ch, c['yH'], c['yW'])
    if c['layout'] == CHANNELS_LAST:
        xs, ys = (xs[0], 1, c['xW'] * ch, ch), (ys[0], 1, c['yW'] * ch, ch)
    elif c['layout'] == EVERY_SECOND_SAMPLE:
        xs = (2 * xs[0],) + xs[1:]
    p = filtered_lrelu_params(c['dtype'], (n, ch, c['xH'], c['xW']), (c['yH'], c['yW']), xs, ys, c['up'], c['down'], (c['fuW'], c['fuH']), (c['fdW'], c['fdH']),
                              c['px0'], c['py0'], c['gain'], c['slope'], c['clamp'], c['flip'], write_signs=c['writeSigns'], read_signs=c['readSigns'],
                              s_hw=(c['sH'], c['sWbytes']), sx=c['sx'], sy=c['sy'], fd_mirror=c['fdMirror'], fd=PLACEHOLDER + (4 if c['fdOdd'] else 0),
                              s=None if c['sNull'] else PLACEHOLDER)
    if c['partials']:
        p.ySumPartial = p.yAbsMaxPartial = PLACEHOLDER
    return p


class _knob:
    """The A/B setting of a table call, for the calls inside the block.  SG3_FLRELU_NOPACK is read once per process: its rows run in a
    child (test_nopack_rows_in_a_process_of_their_own)."""
    def __init__(self, lib, knob):
        self.lib, self.knob = lib, knob

    def __enter__(self):
        assert self.knob != KNOB_NOPACK
        self.slow = os.environ.pop('SG3_FLRELU_SLOWACT', None)
        if self.knob == KNOB_SLOWACT:
            os.environ['SG3_FLRELU_SLOWACT'] = '1'
        self.wide = self.lib.sg3_filtered_lrelu_force_up4_wide(int(self.knob == KNOB_UP4_WIDE))

    def __exit__(self, *exc):
        self.lib.sg3_filtered_lrelu_force_up4_wide(self.wide)
        os.environ.pop('SG3_FLRELU_SLOWACT', None)
        if self.slow is not None:
            os.environ['SG3_FLRELU_SLOWACT'] = self.slow


def _check_row(abi, lib, c, q, launches):
    """One table call against the library: the plan field by field, and the three older queries against the plan and the recording."""
    p = _params(c)
    info = abi.FilteredLreluDispatchInfo()
    rc = lib.sg3_filtered_lrelu_dispatch(ctypes.byref(p), ctypes.byref(info))
    assert rc == q['rc'], (c, rc, lib.sg3_last_error())
    got = info.as_dict()
    assert got['launches'] == q['launches'] and len(launches) == q['launches'], (c, got, q)
    if rc == abi.SG3_NO_KERNEL:
        assert got['kind'] == abi.SG3_FLRELU_NONE, (c, got)
    for want, la in zip(launches, got['launch']):
        assert got['kind'] == want['kind'], (c, got, want)
        if want['kind'] == abi.SG3_FLRELU_POINTWISE:
            assert la['totalBlocks'] == want['totalBlocks'], (c, got, want)
            continue
        for name in STREAM_COORDS + ('nStrips', 'TW', 'ox0Base', 'wideBlocks', 'totalBlocks'):
            assert la[name] == want[name], (c, name, got, want)
        assert (got['nChunks'], got['chunkRows'], got['fastAct']) == (q['gridChunks'], q['gridChunkRows'], want['fastAct']), (c, got, want)
    # the older queries: as recorded from the library before the plan existed, and as the plan implies
    ppw = lib.sg3_filtered_lrelu_planes_per_wave(ctypes.byref(p))
    g = [ctypes.c_int() for _ in range(5)]
    ok = lib.sg3_filtered_lrelu_stream_grid(ctypes.byref(p), *[ctypes.byref(v) for v in g])
    grid = tuple(v.value for v in g)
    assert ppw == q['planesPerWave'] and ok == q['gridOk'], (c, ppw, ok, q)
    assert grid == (q['gridStrips'], q['gridStripW'], q['gridFullStrips'], q['gridChunks'], q['gridChunkRows']), (c, grid, q)
    stream = got['kind'] == abi.SG3_FLRELU_STREAM
    assert ok == int(stream) and ppw == (got['planesPerWave'] if stream else 0), (c, got)
    if stream:
        mixed = got['planesPerWave'] == 3
        full = info.nStrips[0]
        assert grid == (full + mixed, info.TW[0], full if mixed else 0, got['nChunks'], got['chunkRows']), (c, grid, got)
        assert got['planesPerWave'] == (2 if not mixed and info.G[0] == 2 else 3 if mixed else 1)
        if rc == 0:
            assert mixed == (info.wideBlocks[0] > 0 or got['launches'] == 2), (c, got)
        # every readSigns call is cut into equal strips, which is what sg3_filtered_lrelu_sum_slots counts on
        slots = lib.sg3_filtered_lrelu_sum_slots(c['N'], c['C'], c['yH'], c['yW'], c['down'])
        assert got['sumSlots'] == (slots if c['readSigns'] else 0) and (not c['readSigns'] or slots == grid[0] * grid[3]), (c, got, slots)
    assert lib.sg3_filtered_lrelu_has_kernel(c['up'], c['down'], c['fuW'], c['fuH'], c['fdW'], c['fdH']) >= int(got['kind'] != abi.SG3_FLRELU_NONE)
    return got


def test_dispatch_reproduces_the_recorded_table(table):
    abi, lib = _lib()
    assert len(table['calls']) > 2000
    seen = 0
    for c, q, launches in zip(table['calls'], table['queries'], table['launches']):
        if c['knob'] == KNOB_NOPACK:
            continue
        with _knob(lib, c['knob']):
            _check_row(abi, lib, c, q, launches)
        seen += 1
    assert seen > 2000
    rcs = [q['rc'] for q in table['queries']]
    assert rcs.count(abi.SG3_NO_KERNEL) >= 20 and rcs.count(abi.SG3_BAD_ARG) >= 1
    assert sum(q['launches'] == 2 for q in table['queries']) >= 50


_CHILD = '''
import json, sys
sys.path[:0] = {paths!r}
sys.path.insert(0, {tests!r})
import test_flrelu_dispatch_cpu as t
abi, lib = t._lib()
table = t._load_table()
n = 0
for c, q, launches in zip(table['calls'], table['queries'], table['launches']):
    if c['knob'] == t.KNOB_NOPACK:
        t._check_row(abi, lib, c, q, launches)
        n += 1
print(n)
'''


def test_nopack_rows_in_a_process_of_their_own(table):
    """SG3_FLRELU_NOPACK=1 is read once per process: the rows recorded under it run in a child that has it set."""
    rows = [(c, q) for c, q in zip(table['calls'], table['queries']) if c['knob'] == KNOB_NOPACK]
    assert len(rows) >= 50 and all(q['planesPerWave'] in (0, 1) for _, q in rows)
    env = dict(os.environ, SG3_FLRELU_NOPACK='1')
    env.pop('SG3_FLRELU_SLOWACT', None)
    code = _CHILD.format(paths=[p for p in sys.path if p], tests=HERE)
    out = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    assert int(out.stdout.strip().splitlines()[-1]) == len(rows)


def test_knobs_change_the_plan_as_documented(table):
    """Per knob: the same call without it is in the table too, and only what the knob's comment in csrc/sg3_flrelu_plan.h names moved."""
    key = lambda c: tuple(v for n, v in c.items() if n != 'knob')       # noqa: E731
    base = {key(c): (q, la) for c, q, la in zip(table['calls'], table['queries'], table['launches']) if c['knob'] == KNOB_NONE}
    moved = {KNOB_NOPACK: 0, KNOB_SLOWACT: 0, KNOB_UP4_WIDE: 0}
    for c, q, la in zip(table['calls'], table['queries'], table['launches']):
        if c['knob'] == KNOB_NONE:
            continue
        q0, la0 = base[key(c)]
        assert q['rc'] == q0['rc']
        if c['knob'] == KNOB_NOPACK:
            assert q['planesPerWave'] == min(q0['planesPerWave'], 1) and all(l['G'] == 1 for l in la if l['kind'] == 2), c
            moved[c['knob']] += q != q0
        else:
            name = 'fastAct' if c['knob'] == KNOB_SLOWACT else 'WIDE'
            assert q == q0 and [{k: v for k, v in l.items() if k != name} for l in la] == [{k: v for k, v in l.items() if k != name} for l in la0], c
            if c['knob'] == KNOB_SLOWACT:
                assert all(l['fastAct'] == 0 for l in la)
            else:
                assert all(l['WIDE'] == int(l['kind'] == 2 and l['U'] == 4 and l['RADIAL'] == 0 and l['SIGNS'] == 0) for l in la), c
            moved[c['knob']] += la != la0
    assert all(v >= 10 for v in moved.values()), moved


def _library_kernels():
    """(dtype, U, D, VPH, RADIAL, SIGNS, G, WIDE) of every flrelu_stream_kernel instantiation in the built library."""
    from torch_utils import _sg3abi
    sym = subprocess.run(['nm', '-D', '--defined-only', _sg3abi.LIB_PATH], capture_output=True, text=True)
    if sym.returncode != 0 or 'flrelu_stream_kernel' not in sym.stdout:
        sym = subprocess.run(['nm', '--defined-only', _sg3abi.LIB_PATH], check=True, capture_output=True, text=True)
    out = set()
    # _ZN3sg320flrelu_stream_kernelI<f | DF16_>Li<U>ELi<D>E...EEvNS_12StreamParamsE (host stubs carry a prefix in front of the name)
    for m in re.finditer(r'flrelu_stream_kernelI(f|DF16_)((?:Li\d+E){7})', sym.stdout):
        out.add((0 if m.group(1) == 'f' else 1,) + tuple(int(v) for v in re.findall(r'Li(\d+)E', m.group(2))))
    return out


def test_table_reaches_every_kernel_of_the_library(table):
    """Every instantiation the library holds is chosen by a row of the table.  The eight WIDE = 1 kernels (the earlier form of the up-4
    separable plain forward: two tensor types x two vertical phases x one | two planes per wave) are reached with
    sg3_filtered_lrelu_force_up4_wide(1) / SG3_FLRELU_UP4_WIDE=1 only; every other one in a default environment."""
    built = _library_kernels()
    assert len(built) == 164, len(built)
    reached = {False: set(), True: set()}
    for c, launches in zip(table['calls'], table['launches']):
        for la in launches:
            if la['kind'] == 2:
                reached[c['knob'] != KNOB_NONE].add((c['dtype'],) + tuple(la[k] for k in STREAM_COORDS))
    need_a_knob = {k for k in built if k[7] == 1}
    assert len(need_a_knob) == 8
    assert reached[False] == built - need_a_knob, (sorted(built - need_a_knob - reached[False]), sorted(reached[False] - built))
    assert need_a_knob <= reached[True]


def test_pinned_resource_coordinates_are_layer_calls(table):
    """The instantiations whose registers and occupancy tests/test_flrelu_up4_resources_cpu.py pins (UP4, UP2, the wide form) against the
    calls of the T-1024 / R-1024 layers.  Every layer of one up factor has the same vertical phase (VPH 1 at up 4, 0 at up 2), so the
    layers take the pinned kernels of that phase -- the wide form with its knob -- and the other phase is met only where a caller moves
    the top padding (the rows of the table made for that)."""
    import test_flrelu_up4_resources_cpu as res
    from oracle import oracle as O
    from synth_weights import CONFIGS
    layer_calls = set()
    for cfg in ('T1024', 'R1024'):
        for L in O.layer_schedule(**CONFIGS[cfg])['layers']:
            side = L['in_size'] + L['conv_kernel'] - 1
            layer_calls.add((L['out_channels'], side, side, L['up'], L['down'], L['padding'][0], L['padding'][2]))
    by_layers, by_any = {}, set()
    for c, launches in zip(table['calls'], table['launches']):
        for la in launches:
            if la['kind'] == 2:
                coords = ('float' if c['dtype'] == 0 else 'half',) + tuple(la[k] for k in STREAM_COORDS)
                by_any.add(coords)
                if (c['C'], c['xH'], c['xW'], c['up'], c['down'], c['px0'], c['py0']) in layer_calls and c['N'] in (1, 4, 8) and c['layout'] == DENSE:
                    by_layers.setdefault(coords, set()).add(c['knob'])
    layer_vph = {4: 1, 2: 0}
    pinned = res.UP4 + res.UP2 + [k[:7] + (1,) for k in res.UP4]
    assert len(pinned) == 12
    for coords in pinned:
        assert coords in by_any, coords
        if coords[3] == layer_vph[coords[1]]:
            assert (KNOB_UP4_WIDE if coords[7] else KNOB_NONE) in by_layers[coords], coords
        else:
            assert coords not in by_layers, coords


def test_dispatch_rejects_what_the_launch_rejects(table):
    abi, lib = _lib()
    good = dict(table['calls'][0])
    info = abi.FilteredLreluDispatchInfo()
    assert lib.sg3_filtered_lrelu_dispatch(ctypes.byref(_params(good)), ctypes.byref(info)) == table['queries'][0]['rc'] == 0
    for bad in (dict(N=0), dict(C=0), dict(xH=0), dict(yW=0), dict(up=0), dict(dtype=2), dict(writeSigns=1, readSigns=1)):
        assert lib.sg3_filtered_lrelu_dispatch(ctypes.byref(_params(dict(good, **bad))), ctypes.byref(info)) == abi.SG3_BAD_ARG, bad
    assert lib.sg3_filtered_lrelu_dispatch(None, ctypes.byref(info)) == abi.SG3_BAD_ARG
    assert lib.sg3_filtered_lrelu_dispatch(ctypes.byref(_params(good)), None) == abi.SG3_BAD_ARG
