"""Regenerates tests/golden/modconv_dispatch.json: what sg3_modulated_conv2d launches for a fixed list of calls on a 256-CU device.

The table is RECORDED, not computed by the code it pins: csrc/sg3_modconv.hip and csrc/sg3_modconv_f23.hip are compiled with
modconv_dispatch_recorder.h force-included (the launch macro and the attribute call write down kernel name with template arguments,
grid, workgroup, LDS bytes) and linked with modconv_dispatch_recorder.cpp; this script makes the list of calls, runs that program and
stores the result.  The committed table came from the commit BEFORE the dispatch moved into csrc/sg3_modconv_plan.h.

    hipcc -O1 -std=c++17 -fPIC --offload-arch=gfx950 -include tests/golden/modconv_dispatch_recorder.h -c <csrc>/sg3_modconv.hip -o a.o
    (the same for sg3_modconv_f23.hip -> b.o, and -x hip -c tests/golden/modconv_dispatch_recorder.cpp -> m.o)
    hipcc -rdynamic m.o a.o b.o -ldl -o recorder
    python tests/golden/make_modconv_dispatch.py recorder            # needs the built library for the form selector of the op
"""
import json
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)

CALL_COLUMNS = ['dtype', 'N', 'I', 'O', 'H', 'W', 'k', 'pad', 'precision', 'outRowStride', 'dcoef', 'bias', 'scratch', 'forcedRows']
PLAN_COLUMNS = ['family', 'WM', 'WN', 'TM', 'TN', 'SPLIT', 'PACK', 'NBUF', 'M16', 'nch', 'xTiles', 'yTiles', 'mTiles', 'kSplits',
                'gridX', 'gridY', 'block', 'ldsBytes', 'outPitch', 'reduceGrid']
FP32, F16X3, F16, F16X3_F23, F16_F23 = range(5)       # SG3_CONV_*
F32, F16T = 0, 1                                      # SG3_F32, SG3_F16


def calls():
    """The list: rows of CALL_COLUMNS.  `scratch` = 1 offers what sg3_modconv_split_scratch_floats asks for."""
    import torch
    from oracle import oracle as O
    from synth_weights import CONFIGS
    from torch_utils.ops import modulated_conv as mc
    from golden_cases import MODCONV_CASES
    out = []

    def add(dtype, n, ci, co, h, w, k, pad, prec, dcoef, bias=0, pitches=False):
        strides = [0]
        ow = w + 2 * pad - k + 1
        if pitches and k == 3 and prec != FP32 and ow >= 128:          # modulated_conv.py::_launch, align_rows
            per_line = 128 // (4 if dtype == F32 else 2)
            strides.append((ow + per_line - 1) // per_line * per_line)
        for stride in strides:
            for rows in ((0, 4, 5, 7) if prec in (F16X3_F23, F16_F23) else (0,)):
                for scratch in (0, 1):
                    out.append([dtype, n, ci, co, h, w, k, pad, prec, stride, dcoef, bias, scratch, rows])

    def forms(ci, co, h, w, k, pad):
        """(dtype, precision) a call takes: fp32 with a bound, fp16, fp32 without a bound"""
        return [(F32, mc._choose_form(torch.float32, k, pad, ci, co, h, w, True)), (F16T, mc._choose_form(torch.float16, k, pad, ci, co, h, w, True)),
                (F32, FP32)]

    # every layer of T-1024 and R-1024 (input mix and ToRGB included) and its data-gradient call
    for cfg in ('T1024', 'R1024'):
        sched = O.layer_schedule(**CONFIGS[cfg])
        c0, s0 = sched['input']['channels'], sched['input']['size']
        layers = [(c0, c0, s0, 1, False, False)] + [(L['in_channels'], L['out_channels'], L['in_size'], L['conv_kernel'], not L['is_torgb'], L['is_torgb'])
                                                    for L in sched['layers']]
        for n in (1, 4, 8):
            for ci, co, h, k, demod, torgb in layers:
                pad = k - 1
                for dtype, prec in forms(ci, co, h, h, k, pad):
                    add(dtype, n, ci, co, h, h, k, pad, prec, int(demod or prec != FP32), pitches=True)
                    if torgb:
                        add(dtype, n, ci, co, h, h, k, pad, prec, 0, bias=1)
                oh = h + 2 * pad - k + 1
                for dtype, prec in forms(co, ci, oh, oh, k, k - 1 - pad)[:2]:      # dy always comes with its maximum as the bound
                    add(dtype, n, co, ci, oh, oh, k, k - 1 - pad, prec, 1)

    # every shape of the modconv tests: (n, ci, co, h, w, k) with the paddings the tests use, in every form the library takes
    shapes = []
    for n, ci, co, h, k in [(2, 323, 203, 22, 3), (1, 128, 81, 40, 3), (2, 51, 32, 70, 3), (1, 32, 3, 64, 1), (2, 512, 512, 12, 3), (2, 100, 161, 30, 1),
                            (1, 64, 64, 33, 1), (1, 203, 128, 37, 3), (3, 81, 51, 50, 3), (4, 16, 832, 36, 3), (8, 96, 100, 36, 3), (2, 70, 512, 52, 3),
                            (1, 64, 64, 35, 3), (8, 512, 512, 36, 3), (2, 645, 406, 20, 1), (1, 1024, 1024, 12, 1), (2, 161, 102, 70, 1), (3, 102, 64, 50, 1),
                            (1, 17, 200, 9, 1), (2, 203, 128, 37, 3), (1, 81, 51, 50, 3), (1, 64, 128, 131, 3), (1, 51, 32, 140, 3), (1, 81, 51, 127, 3),
                            (1, 33, 70, 150, 3), (1, 32, 32, 126, 3)]:
        shapes.append((n, ci, co, h, h + 3, k))                        # test_gpu_ops.py: h x (h + 3) planes
    for n, ci, co, h in [(2, 51, 32, 150), (1, 81, 51, 278), (1, 64, 70, 131), (2, 64, 70, 150), (1, 128, 96, 278)]:
        shapes.append((n, ci, co, h, h, 3))                            # aligned row pitch
    for n, ci, co, h, k in [(1, 512, 512, 36, 3), (2, 256, 130, 50, 3), (1, 512, 512, 52, 3), (1, 1024, 1024, 36, 1), (2, 645, 406, 40, 1)]:
        shapes.append((n, ci, co, h, h, k))                            # K split on small grids
    shapes += [(1, 16, 32, 2960, 2960, 3), (1, 16, 64, 2400, 2400, 1), (1, 16, 32, 300, 300, 3), (1, 16, 64, 300, 300, 1)]
    for n, ci, co, h, w in [(2, 64, 64, 30, 30), (1, 323, 203, 22, 26), (2, 81, 51, 40, 70), (1, 512, 512, 20, 36), (3, 17, 130, 35, 34), (1, 16, 96, 9, 10),
                            (1, 64, 64, 20, 31), (3, 32, 200, 118, 90), (1, 512, 512, 84, 84), (1, 323, 203, 60, 60), (1, 192, 96, 48, 48)]:
        shapes.append((n, ci, co, h, w, 3))                            # test_gpu_f23.py, smoke()
    shapes += [(c['n'], c['ci'], c['co'], c['h'], c['w'], c['k']) for c in MODCONV_CASES.values()]
    # tile variants none of the above reaches: the double-buffered 64- and 128-channel 1x1 tiles, the ten-row 3x3 tile (a plane too
    # wide for the flat kernel; also test_gpu_ops.py) and the eight-row 64-channel tile of the plain fp16 form
    shapes += [(1, 300, 64, 20, 20, 1), (1, 300, 300, 20, 20, 1), (1, 16, 640, 96, 99, 3), (1, 64, 128, 100, 200, 3)]
    lib = mc.abi.load()
    for n, ci, co, h, w, k in shapes:
        for pad in sorted({k - 1, 0}):
            for dtype in (F32, F16T):
                add(dtype, n, ci, co, h, w, k, pad, FP32, 1, pitches=True)
                if k == 3 or (h * w) % 2 == 0:
                    add(dtype, n, ci, co, h, w, k, pad, F16X3, 1, pitches=True)
                    add(dtype, n, ci, co, h, w, k, pad, F16, 1, pitches=True)
                if lib.sg3_modconv_f23_supported(dtype, ci, co, h, w, k, pad, 0):
                    add(dtype, n, ci, co, h, w, k, pad, F16X3_F23 if dtype == F32 else F16_F23, 1, pitches=True)
    seen, uniq = set(), []
    for c in out:
        if tuple(c) not in seen:
            seen.add(tuple(c)); uniq.append(c)
    return uniq


KERNELS = {   # kernel -> (family, template parameter names; T = tensor type)
    'modconv_mfma_kernel': (0, ['T', 'KS', 'WM', 'WN', 'TM', 'TN']),
    'modconv_1x1_small_kernel': (1, ['T', 'OMAX']),
    'modconv_f16x3_kernel': (2, ['T', 'WM', 'WN', 'TN', 'SPLIT', 'PACK']),
    'modconv_flat_kernel': (3, ['T', 'TN', 'SPLIT']),
    'modconv1_f16x3_kernel': (4, ['T', 'WM', 'WN', 'TM', 'TN', 'SPLIT', 'NBUF', 'M16']),
    'modconv_f23_kernel': (5, ['TN', 'T']),
}


def plan_row(rec):
    """One recorded call -> a row of PLAN_COLUMNS (-1: the launch does not say)."""
    call = dict(zip(CALL_COLUMNS, rec['call']))
    assert rec['rc'] == 0 and 1 <= len(rec['launches']) <= 2, rec
    la = rec['launches'][0]
    name, args = re.search(r'(modconv\w*_kernel)<([^>]*)>', la['kernel']).groups()
    family, names = KERNELS[name]
    t = dict(zip(names, [a.strip() for a in args.split(',')]))
    assert t.pop('T') == ('float' if call['dtype'] == F32 else 'half'), rec
    val = {k: {'true': 1, 'false': 0}.get(v, v) for k, v in t.items()}
    row = dict.fromkeys(PLAN_COLUMNS, 0)
    row.update({k: int(v) for k, v in val.items() if k in row})
    if family == 0:
        assert int(val['KS']) == call['k']
    if family == 3:
        row.update(WM=2, WN=2)                                          # 64 channels x 2 pixel groups
    if family == 5:
        row.update(WM=2, WN=4, SPLIT=int(call['dtype'] == F32))          # 2 M blocks x 4 transform points
    if family in (2, 3, 5):
        row['TM'] = 1
    row['family'] = family
    for k in ('nch', 'xTiles', 'yTiles', 'mTiles'):
        row[k] = la[k]
    row['outPitch'] = la['outPitch'] if family in (2, 3, 5) else -1     # the other launchers leave the field unset
    gx, gy, gz = la['grid']
    assert gz == 1 and la['attr'] in (0, la['lds'])
    tiles = row['xTiles'] * row['yTiles'] * row['mTiles'] * call['N']
    row['kSplits'] = gx // tiles if family in (3, 4) else 1
    assert family not in (3, 4) or gx == tiles * row['kSplits']
    row.update(gridX=gx, gridY=gy, block=la['block'], ldsBytes=la['lds'])
    if len(rec['launches']) == 2:
        red = rec['launches'][1]
        assert 'modconv_split_reduce_kernel' in red['kernel'] and row['kSplits'] > 1 and red['block'] == 256
        row['reduceGrid'] = red['grid'][0]
    else:
        assert row['kSplits'] == 1
    return [row[k] for k in PLAN_COLUMNS]


def main():
    recorder = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, 'modconv_dispatch.json')
    cs = calls()
    with tempfile.NamedTemporaryFile('w', suffix='.txt', delete=False) as f:
        f.write(''.join(' '.join(str(v) for v in c) + '\n' for c in cs))
    env = dict(os.environ, REC_CUS='256')
    recs = [json.loads(line) for line in subprocess.run([recorder, f.name], check=True, capture_output=True, text=True, env=env).stdout.splitlines()]
    os.unlink(f.name)
    assert [r['call'] for r in recs] == cs
    rows = []
    for r in recs:
        if r['call'][CALL_COLUMNS.index('scratch')] and r['need'] == 0:
            continue                                                    # nothing was offered: the same call as without scratch
        rows.append(r['call'] + plan_row(r))
    with open(out, 'w') as f:
        f.write('{"cus": 256, "call_columns": %s, "plan_columns": %s, "rows": [\n' % (json.dumps(CALL_COLUMNS), json.dumps(PLAN_COLUMNS)))
        f.write(',\n'.join(json.dumps(r, separators=(',', ':')) for r in rows))
        f.write('\n]}\n')
    print(f'{len(rows)} rows -> {out}')


if __name__ == '__main__':
    main()
