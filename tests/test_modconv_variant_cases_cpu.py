"""CPU: the table of tests/modconv_variant_cases.py against the host-only plan query (sg3_modconv_dispatch at 256 CUs) and against
its own rules.  Every row maps to exactly the kernel variant it is filed under; the variants filed are the reachable set of
test_modconv_dispatch_cpu._variants() plus, in a child process with SG3_CONV1_MFMA32=1, the twelve M16 = 0 kernels; every row is
ragged and spanning (or says why not) and small."""
import collections
import json
import os
import subprocess
import sys

import modconv_variant_cases as mv
from helpers import HERE
from test_modconv_dispatch_cpu import _CHILD, _dispatch, _lib, _variants

BY_KIND = collections.defaultdict(list)
for _e in mv.ENTRIES:
    BY_KIND[_e['kind']].append(_e)
M16_VARIANTS = {v[:10] + (0,) for v in _variants() if v[2] == mv.GEMM1 and v[9] == 2}


def test_every_row_maps_to_the_variant_it_is_filed_under():
    abi, lib = _lib()
    assert len({e['id'] for e in mv.ENTRIES}) == len(mv.ENTRIES)
    for e in mv.ENTRIES:
        if e['kind'] == 'm16':
            continue                                        # needs the knob: test_m16_rows_map_to_the_twelve_kernels_behind_the_knob
        plan = _dispatch(abi, lib, e)
        assert mv.variant_of(e, plan) == e['variant'], (e['id'], plan)
        assert plan['kSplits'] == (e['kSplits'] if e['kind'] == 'ksplit' else 1), (e['id'], plan)
        assert (plan['reduceGrid'] > 0) == (e['kind'] == 'ksplit'), (e['id'], plan)


def test_the_variants_filed_are_the_reachable_set():
    want = _variants()
    filed = [e['variant'] for e in BY_KIND['variant']]
    assert len(want) == 80 and len(filed) == 80 and set(filed) == want, (sorted(want - set(filed)), sorted(set(filed) - want))
    assert {e['variant'] for e in mv.ENTRIES if e['kind'] != 'm16'} == want              # the extra rows add calls, not kernels
    crossed = [v for v in filed if mv.crossed(v)]
    assert len(crossed) == 28 and all(mv.sibling(e)['variant'] in want for e in BY_KIND['variant'] if mv.crossed(e['variant']))
    # what torch_utils.ops.modulated_conv._choose_form can reach: fp32 tensors never take SPLIT = 0 of the direct forms, fp16 never SPLIT = 1
    assert len(want) - len(crossed) == 52


def test_m16_rows_map_to_the_twelve_kernels_behind_the_knob():
    """SG3_CONV1_MFMA32 is read once per process: the rows are planned in a child (as test_knobs_change_the_plan_as_documented does)."""
    abi, lib = _lib()
    rows = BY_KIND['m16']
    assert len(M16_VARIANTS) == 12 and not (M16_VARIANTS & _variants())
    assert sorted(e['variant'] for e in rows) == sorted(M16_VARIANTS)
    for e in rows:                                          # without the knob: the M16 = 1 twin
        assert mv.variant_of(e, _dispatch(abi, lib, e)) == e['variant'][:10] + (1,), e['id']
    env = dict(os.environ)
    env[mv.M16_ENV[0]] = mv.M16_ENV[1]
    code = _CHILD.format(paths=[p for p in sys.path if p], tests=HERE)
    out = subprocess.run([sys.executable, '-c', code, json.dumps(rows)], env=env, check=True, capture_output=True, text=True).stdout
    plans = json.loads(out.strip().splitlines()[-1])
    assert len(plans) == len(rows)
    for e, plan in zip(rows, plans):
        assert mv.variant_of(e, plan) == e['variant'] and plan['kSplits'] == 1, (e['id'], plan)


def test_rows_are_ragged_and_spanning_or_say_why():
    for e in mv.ENTRIES:
        assert mv.ragged_violations(e) == [], (e['id'], mv.ragged_violations(e))
        assert bool(mv.spanning_violations(e) or e['N'] != 2) == bool(e['exempt']), (e['id'], mv.spanning_violations(e), e['exempt'])
    # the only shapes without a second M tile: the tiles the plan takes for O <= 64 alone
    assert {e['variant'][2:7] for e in mv.ENTRIES if e['exempt']} == {(mv.FP32_MFMA, 1, 4, 2, 2), (mv.GEMM1, 1, 8, 2, 1)}
    assert all(mv.spanning_violations(e) == ['O'] and 32 < e['O'] <= 64 and e['N'] == 2 for e in mv.ENTRIES if e['exempt'])
    # tall stacks of the plain fp16 form: 128 output rows or more
    tall = [e for e in mv.ENTRIES if e['variant'][2] == mv.ROWS and e['variant'][3:7] in ((1, 4, 1, 5), (2, 2, 1, 6))]
    assert len(tall) == 16 and all(mv.out_hw(e)[0] >= 128 and e['variant'][7] == 0 for e in tall)


def test_rows_are_small():
    sizes = sorted((mv.macs(e), e['id']) for e in mv.ENTRIES)
    print('largest row: %d multiply-adds (%s); median %d' % (sizes[-1] + (sizes[len(sizes) // 2][0],)))
    assert sizes[-1][0] <= mv.MAX_MACS


def test_the_extra_rows_cover_what_the_module_promises():
    variants = _variants()
    by = lambda kind: collections.Counter(e['variant'] for e in BY_KIND[kind])
    # padding 0 of every 3x3 ROWS / FLAT / FP32_MFMA variant, on the same output plane
    assert by('pad0') == collections.Counter(v for v in variants if v[1] == 3 and v[2] in (mv.ROWS, mv.FLAT, mv.FP32_MFMA))
    first = {e['variant']: e for e in BY_KIND['variant']}
    for e in BY_KIND['pad0'] + BY_KIND['padalt']:
        assert e['pad'] == 0 and first[e['variant']]['pad'] == 2 and mv.out_hw(e) == mv.out_hw(first[e['variant']]), e['id']
    assert sorted((v[0], v[2]) for v in by('padalt')) == [(0, mv.F23), (1, mv.F23)]
    # K splits: the flat kernel for every (tensor type, SPLIT), the 1x1 GEMM for fp32 tensors and each SPLIT; 2 and 4 workgroups per tile
    ks = {(e['variant'][2], e['dtype'], e['variant'][7], e['kSplits']) for e in BY_KIND['ksplit']}
    assert ks == {(mv.FLAT, t, sp, n) for t in (0, 1) for sp in (0, 1) for n in (2, 4)} | {(mv.GEMM1, 0, sp, n) for sp in (0, 1) for n in (2, 4)}
    assert all(e['scratch'] == 1 for e in BY_KIND['ksplit']) and all(e['scratch'] == 0 for e in mv.ENTRIES if e['kind'] != 'ksplit')
    assert {e['dtype'] for e in BY_KIND['ksplit']} == {0, 1}                               # both instantiations of the reduce kernel
    # ToRGB: four pixels per thread (H W divisible by 4) and one, per tensor type
    torgb = {(e['dtype'], e['H'] * e['W'] % 4 == 0) for e in mv.ENTRIES if e['variant'][2] == mv.TORGB and e['demodulate']}
    assert torgb == {(t, vec) for t in (0, 1) for vec in (False, True)}
    # demodulation off, styles x 1000: one fp32-tensor row per family
    assert sorted(e['variant'][2] for e in BY_KIND['nodemod']) == list(range(6)) and all(e['dtype'] == 0 and not e['demodulate'] for e in BY_KIND['nodemod'])
    assert all(e['demodulate'] for e in mv.ENTRIES if e['kind'] != 'nodemod')
    # transform-domain rows force their rows per wave; nobody else does
    assert all((e['forcedRows'] == e['variant'][6]) if e['variant'][2] == mv.F23 else e['forcedRows'] == 0 for e in mv.ENTRIES)
