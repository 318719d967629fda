#!/usr/bin/env python3
"""Search the rows of tests/modconv_variant_cases.py: for every kernel variant the launch plan can choose, the smallest ragged,
spanning call (rules: that module's docstring) that sg3_modconv_dispatch(..., cus=256) maps to it.  Host only: runs without a GPU.

    python tools/find_modconv_variant_cases.py            # prints the literal TABLE rows

The plan of the 3x3 direct forms and of the 1x1 GEMM reads the tensor type nowhere (but in the K-split gate of the GEMM) and the
padding only through the output plane, so those are searched once, on fp32 tensors at full padding, and the rows of the other tensor
type and of padding 0 are derived -- and checked against the query like every other row before they are printed.  The M16 = 0 rows
are the M16 = 1 rows of the double-buffered 1x1 tiles: SG3_CONV1_MFMA32 is read once per process, so the CPU test checks them in a
child process."""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import torch  # noqa: E402,F401  (loads torch's HIP runtime before ours)
from torch_utils import _sg3abi as abi  # noqa: E402
import modconv_variant_cases as mv  # noqa: E402

CUS = 256
lib = abi.load()
_p, _info = abi.ModconvParams(), abi.ModconvDispatchInfo()
_FIELDS = ('family', 'WM', 'WN', 'TM', 'TN', 'SPLIT', 'PACK', 'NBUF', 'M16')


def plan(e):
    """(variant, kSplits) of call `e` at 256 CUs, or None where the ABI refuses the call."""
    p = _p
    p.dcoef = 16
    p.dtype, p.precision, p.outRowStride = e['dtype'], e['precision'], 0
    p.N, p.I, p.O, p.H, p.W, p.k, p.pad = e['N'], e['I'], e['O'], e['H'], e['W'], e['k'], e['pad']
    oh, ow = mv.out_hw(e)
    p.splitScratch, p.splitScratchFloats = (16, 4 * e['N'] * e['O'] * oh * ow) if e['scratch'] else (None, 0)
    prev = lib.sg3_modconv_f23_force_rows(e['forcedRows'])
    rc = lib.sg3_modconv_dispatch(ctypes.byref(p), CUS, ctypes.byref(_info))
    lib.sg3_modconv_f23_force_rows(prev)
    if rc != 0:
        return None
    return (e['dtype'], e['k']) + tuple(getattr(_info, n) for n in _FIELDS), _info.kSplits


def call(**kw):
    e = dict(kind='variant', dtype=0, N=2, k=3, pad=2, precision=mv.CONV_F16X3, demodulate=1, scratch=0, forcedRows=0, kSplits=1, exempt='')
    e.update(kw)
    return e


def search(base, Ns, Is, Os, outHs, outWs, want_splits=None):
    """best[variant (, kSplits)] = the candidate with the fewest multiply-adds, N = 2 first, among the ragged spanning ones; where a
    variant has none, among the ragged ones (the exemption is worked out by the caller)."""
    best = {}
    k, pad = base['k'], base['pad']
    for n in Ns:
        for i in Is:
            for o in Os:
                for oh in outHs:
                    for ow in outWs:
                        e = dict(base, N=n, I=i, O=o, H=oh - 2 * pad + k - 1, W=ow - 2 * pad + k - 1)
                        if e['H'] <= 0 or e['W'] <= 0:
                            continue
                        got = plan(e)
                        if got is None:
                            continue
                        e['variant'], e['kSplits'] = got
                        if want_splits is not None and got[1] not in want_splits:
                            continue
                        if mv.ragged_violations(e) or mv.macs(e) > mv.MAX_MACS:
                            continue
                        key = got if want_splits is not None else got[0]
                        rank = (len(mv.spanning_violations(e)), n != 2, mv.macs(e), n, i, o, oh, ow)
                        if key not in best or rank < best[key][0]:
                            best[key] = (rank, e)
    return {key: e for key, (rank, e) in best.items()}


def exemption(e):
    miss = mv.spanning_violations(e)
    why = []
    if 'O' in miss:
        why.append('the plan takes this tile for O <= %d only: one M tile' % mv.tile(e['variant'])[0])
    if [m for m in miss if m != 'O']:
        why.append('no spanning shape along ' + ', '.join(m for m in miss if m != 'O'))
    if e['N'] != 2:
        why.append('the plan needs N = %d' % e['N'])
    return '; '.join(why)


def main():
    rows = []
    found = {}

    def keep(e, kind=None):
        e = dict(e, kind=kind or e['kind'])
        got = plan(e)
        assert got is not None and got[0] == e['variant'] and (e['kind'] != 'ksplit' or got[1] == e['kSplits']), (e, got)
        if e['kind'] != 'ksplit':
            e['kSplits'] = 0                              # not part of what the row is filed under
        e['exempt'] = exemption(e)
        rows.append(e)
        return e

    # exact fp32 products: the M tile follows O alone
    for dtype in (0, 1):
        for k in (3, 1):
            got = search(call(dtype=dtype, k=k, pad=k - 1, precision=mv.CONV_FP32), (2,), (17, 21), range(5, 260), range(3, 20), (33, 34, 35))
            for v, e in sorted(got.items()):
                keep(e)
                if k == 3:
                    keep(dict(e, pad=0, H=e['H'] + 4, W=e['W'] + 4), 'pad0')
        # ToRGB: 17 channels -> 3, two workgroups per sample, one pixel per thread (33 x 33) and four (34 x 34)
        t = call(dtype=dtype, k=1, pad=0, precision=mv.CONV_FP32, I=17, O=3, H=33, W=33)
        t['variant'] = plan(t)[0]
        keep(t)
        keep(dict(t, H=34, W=34), 'torgb')

    # 3x3 direct forms (ROWS, FLAT): searched on fp32 tensors, rows of fp16 tensors and padding 0 derived
    for prec in (mv.CONV_F16X3, mv.CONV_F16):
        narrow = search(call(precision=prec), (2, 1, 4, 8), (17, 21), [33, 65, 97, 129] + [64 * m + 1 for m in range(3, 41)], range(3, 60), list(range(3, 70)) + [101, 102])
        tall = search(call(precision=prec), (2,), (17, 21), (33, 65, 97, 129), range(128, 142), (33, 34, 35)) if prec == mv.CONV_F16 else {}
        for v, e in sorted({**tall, **narrow}.items()):
            for dtype in (0, 1):
                d = keep(dict(e, dtype=dtype, variant=(dtype,) + v[1:]))
                keep(dict(d, pad=0, H=d['H'] + 4, W=d['W'] + 4), 'pad0')
        # K splits of the flat kernel
        got = search(call(precision=prec, scratch=1, kind='ksplit'), (2, 1), (117, 245), (65, 97, 129), range(3, 40), range(3, 40), want_splits=(2, 4))
        for (v, ks), e in sorted(got.items()):
            if v[2] == mv.FLAT:
                found.setdefault((prec, ks), e)
        for ks in (2, 4):
            e = found[(prec, ks)]
            for dtype in (0, 1):
                keep(dict(e, dtype=dtype, variant=(dtype,) + e['variant'][1:]))

    # 1x1 GEMM
    for prec in (mv.CONV_F16X3, mv.CONV_F16):
        base = call(k=1, pad=0, precision=prec)
        planes = [(h, w) for h in range(2, 24) for w in range(h, 140) if h * w % 2 == 0 and 256 < h * w < 1200]
        got = {}
        for h, w in planes:
            for v, e in search(base, (2,), (33, 257), (33, 65, 129, 130, 257, 385), (h,), (w,)).items():
                rank = (len(mv.spanning_violations(e)), mv.macs(e))
                if v not in got or rank < got[v][0]:
                    got[v] = (rank, e)
        for v, (_, e) in sorted(got.items()):
            for dtype in (0, 1):
                d = keep(dict(e, dtype=dtype, variant=(dtype,) + v[1:]))
                if v[9] == 2:                             # double-buffered tiles: the M16 = 0 twin under SG3_CONV1_MFMA32=1
                    assert v[10] == 1
                    tw = dict(d, kind='m16', variant=d['variant'][:10] + (0,), exempt=exemption(d), kSplits=0)
                    rows.append(tw)
        # K splits (fp32 tensors only: the gate of the plan)
        ks_found = {}
        for h, w in [(h, w) for h in range(2, 24) for w in range(h, 60) if h * w % 2 == 0 and 256 < h * w < 700]:
            for (v, ks), e in search(dict(base, scratch=1, kind='ksplit'), (2, 1), (261, 517), (65, 129, 130, 257), (h,), (w,), want_splits=(2, 4)).items():
                rank = (len(mv.spanning_violations(e)), e['N'] != 2, mv.macs(e))
                if ks not in ks_found or rank < ks_found[ks][0]:
                    ks_found[ks] = (rank, e)
        for ks in (2, 4):
            keep(ks_found[ks][1])

    # transform-domain 3x3: rows per wave forced (the cost model takes 4 on every grid of at most 256 workgroups)
    for dtype, prec in ((0, mv.CONV_F16X3_F23), (1, mv.CONV_F16_F23)):
        for tn in (4, 5, 7):
            got = search(call(dtype=dtype, precision=prec, forcedRows=tn), (2,), (21,), (65,), (2 * tn + 1, 2 * tn + 2), (34,))
            (v, e), = got.items()
            keep(e)
            if tn == 4:
                keep(dict(e, pad=0, H=e['H'] + 4, W=e['W'] + 4), 'padalt')

    # demodulation off, styles x 1000: one fp32-tensor row per family, on its first variant row
    # (the SPLIT = 1 variant where the family has one: the rescale of the split operands is what these rows are about)
    seen = set()
    for e in sorted(rows, key=lambda e: e['variant']):
        fam = e['variant'][2]
        if e['kind'] == 'variant' and e['dtype'] == 0 and fam not in seen and (fam in (mv.FP32_MFMA, mv.TORGB) or e['variant'][7] == 1):
            seen.add(fam)
            rows.append(dict(e, kind='nodemod', demodulate=0))
    assert len(seen) == 6

    order = {'variant': 0, 'm16': 1, 'pad0': 2, 'padalt': 3, 'ksplit': 4, 'torgb': 5, 'nodemod': 6}
    rows.sort(key=lambda e: (order[e['kind']], e['variant'][2], e['variant'], e['kSplits']))
    for e in rows:
        print('    ' + repr(tuple(e[c] for c in mv.COLUMNS)) + ',')
    print('# %d rows; largest %d multiply-adds' % (len(rows), max(mv.macs(e) for e in rows)), file=sys.stderr)


if __name__ == '__main__':
    main()
