"""Regenerates tests/golden/flrelu_dispatch.json: what sg3_filtered_lrelu launches for a fixed list of calls.

The table is RECORDED, not computed by the code it pins: the host side, csrc/sg3_flrelu_host.hip, is compiled with
modconv_dispatch_recorder.h force-included (the launch macro writes down kernel name with template arguments, grid, workgroup and the
work decomposition of the parameter block) and linked with the kernel file (csrc/sg3_filtered_lrelu.hip in one piece, every part: its
host stubs are what the recorder names) and flrelu_dispatch_recorder.cpp; this script makes the list of calls, runs that program and
stores the result.  The committed table came from the commit BEFORE the choice moved into csrc/sg3_flrelu_plan.h.

    hipcc -O1 -std=c++17 -fPIC --offload-arch=gfx950 -fno-honor-nans -Iinclude -I<csrc> -include tests/golden/modconv_dispatch_recorder.h \
          -c <csrc>/sg3_flrelu_host.hip -o a.o
    hipcc -O1 -std=c++17 -fPIC --offload-arch=gfx950 -fno-honor-nans -Iinclude -I<csrc> -c <csrc>/sg3_filtered_lrelu.hip -o k.o
    hipcc -O1 -std=c++17 --offload-arch=gfx950 -x hip -c tests/golden/flrelu_dispatch_recorder.cpp -o m.o
    hipcc -rdynamic m.o a.o k.o -ldl -o recorder
    python tests/golden/make_flrelu_dispatch.py recorder            # needs the built library for sg3_filtered_lrelu_shape
"""
import ctypes
import json
import math
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)

CALL_COLUMNS = ['dtype', 'N', 'C', 'xH', 'xW', 'yH', 'yW', 'up', 'down', 'fuW', 'fuH', 'fdW', 'fdH', 'px0', 'py0', 'sH', 'sWbytes', 'sx', 'sy',
                'gain', 'slope', 'clamp', 'flip', 'writeSigns', 'readSigns', 'partials', 'fdMirror', 'layout', 'fdOdd', 'sNull', 'knob']
QUERY_COLUMNS = ['rc', 'planesPerWave', 'gridOk', 'gridStrips', 'gridStripW', 'gridFullStrips', 'gridChunks', 'gridChunkRows', 'launches']
LAUNCH_COLUMNS = ['kind', 'U', 'D', 'VPH', 'RADIAL', 'SIGNS', 'G', 'WIDE', 'grid', 'block', 'nStrips', 'TW', 'ox0Base', 'wideBlocks', 'nChunks',
                  'chunkRows', 'totalBlocks', 'fastAct']
F32, F16 = 0, 1                                                     # SG3_F32, SG3_F16
NONE, POINTWISE, STREAM = 0, 1, 2                                   # SG3_FLRELU_*: `kind`
DENSE, CHANNELS_LAST, EVERY_SECOND_SAMPLE = 0, 1, 2                 # `layout` (flrelu_dispatch_recorder.cpp)
KNOB_NONE, KNOB_NOPACK, KNOB_SLOWACT, KNOB_UP4_WIDE = 0, 1, 2, 3    # `knob`
KNOB_ENV = {KNOB_NOPACK: {'SG3_FLRELU_NOPACK': '1'}}                # read once per process: a run of its own (the recorder sets the others per call)

# (x shape, up, taps of fu, padding, radial down filter) of the GPU tests, all down 2 with 12 taps: tests/test_gpu_ops.py,
# tests/test_gpu_flrelu_fast_activation.py
TEST_GEOMETRIES = [
    ((1, 2, 150, 150), 2, 12, [9, 8, 9, 8], False), ((2, 3, 86, 86), 4, 24, [-6, -9, -6, -9], False), ((1, 1, 278, 278), 4, 24, [-6, -9, -6, -9], False),
    ((1, 2, 534, 300), 2, 12, [9, 8, 9, 8], False), ((1, 1, 130, 1046), 2, 12, [-11, -12, -11, -12], False), ((3, 5, 38, 38), 2, 12, [9, 8, 9, 8], False),
    ((1, 2, 148, 148), 2, 12, [11, 10, 11, 10], True), ((2, 3, 84, 84), 4, 24, [-2, -5, -2, -5], True), ((1, 1, 276, 300), 4, 24, [-2, -5, -2, -5], True),
    ((1, 2, 532, 200), 2, 12, [11, 10, 11, 10], True),
    ((2, 2, 86, 86), 4, 24, [-6, -9, -6, -9], False), ((1, 1, 278, 130), 2, 12, [9, 8, 9, 8], False), ((1, 1, 120, 278), 4, 24, [-6, -9, -6, -9], False),
    ((1, 2, 84, 150), 2, 12, [11, 10, 11, 10], True), ((2, 2, 84, 84), 4, 24, [-2, -5, -2, -5], True), ((1, 1, 150, 276), 4, 24, [-2, -5, -2, -5], True),
    ((1, 2, 86, 86), 4, 24, [-6, -9, -6, -9], False), ((1, 2, 84, 84), 4, 24, [-2, -5, -2, -5], True),
    ((1, 3, 150, 150), 2, 12, [9, 8, 9, 8], False), ((1, 3, 86, 86), 4, 24, [-6, -9, -6, -9], False), ((1, 3, 148, 148), 2, 12, [11, 10, 11, 10], True),
    # two planes per wave, and only where it applies
    ((8, 6, 38, 38), 2, 12, [9, 8, 9, 8], False), ((2, 4, 38, 38), 4, 24, [-6, -9, -6, -9], False), ((1, 2, 54, 54), 2, 12, [9, 8, 9, 8], False),
    ((3, 2, 41, 56), 2, 12, [9, 8, 9, 8], False), ((1, 4, 30, 39), 2, 12, [8, 8, 9, 8], False), ((2, 2, 33, 27), 4, 24, [-5, -8, -6, -9], False),
    ((2, 4, 36, 36), 2, 12, [11, 10, 11, 10], True), ((1, 2, 36, 36), 4, 24, [-2, -5, -2, -5], True),
    ((2, 3, 38, 38), 2, 12, [9, 8, 9, 8], False), ((1, 3, 38, 38), 2, 12, [9, 8, 9, 8], False), ((2, 2, 38, 38), 2, 12, [9, 8, 9, 8], False),
    ((1, 2, 38, 60), 2, 12, [9, 8, 9, 8], False),
    # full strips + packed remainder
    ((2, 2, 150, 150), 2, 12, [9, 8, 9, 8], False), ((1, 4, 86, 86), 4, 24, [-6, -9, -6, -9], False), ((1, 2, 60, 278), 4, 24, [-6, -9, -6, -9], False),
    ((1, 2, 100, 150), 2, 12, [11, 10, 11, 10], True), ((1, 3, 60, 84), 4, 24, [-2, -5, -2, -5], True),
    # fast activation
    ((2, 6, 38, 38), 2, 12, [9, 8, 9, 8], False), ((1, 4, 150, 150), 2, 12, [9, 8, 9, 8], False), ((1, 2, 1046, 1046), 2, 12, [9, 8, 9, 8], False),
    ((1, 3, 84, 84), 4, 24, [-2, -5, -2, -5], True),
]
# (n, c, x side, up, down, fu taps, fd taps, (pad lo, pad hi), read, write): tests/test_abi.py::test_filtered_lrelu_stream_grid
ABI_GRID_CALLS = [(1, 32, 1046, 2, 2, 12, 12, (-11, -12), 0, 1), (4, 32, 1046, 2, 2, 12, 12, (-11, -12), 0, 1), (1, 512, 150, 2, 2, 12, 12, (9, 8), 0, 0),
                  (1, 512, 150, 2, 2, 12, 12, (9, 8), 0, 1), (1, 32, 1024, 2, 4, 12, 24, (20, 35), 1, 0), (1, 3, 1024, 1, 1, 1, 1, (0, 0), 0, 0)]


def _shape(lib, x_hw, up, down, fu, fd, pads):
    """(yH, yW, sH, sWbytes) of sg3_filtered_lrelu_shape; fu / fd = (W, H), H = 0 separable"""
    out = [ctypes.c_int() for _ in range(5)]
    rc = lib.sg3_filtered_lrelu_shape(x_hw[0], x_hw[1], up, down, fu[0], fu[1], fd[0], fd[1], *pads, *[ctypes.byref(o) for o in out])
    assert rc == 0, (x_hw, up, down, fu, fd, pads)
    return tuple(o.value for o in out[:4])


def f32(v):
    """the shortest decimal that names the float32 the parameter block holds"""
    import numpy as np
    return float(str(np.float32(v)))


def calls():
    """The list: rows of CALL_COLUMNS."""
    import torch
    from oracle import oracle as O
    from synth_weights import CONFIGS
    from torch_utils import _sg3abi
    from torch_utils.ops import filtered_lrelu as fl
    lib = _sg3abi.load()
    out = []

    def row(dtype, n, c, x_hw, y_hw, up, down, fu, fd, px0, py0, s_hw, sx, sy, gain, slope, clamp, flip, write, read, partials=0, mirror=0,
            layout=DENSE, fd_odd=0, s_null=0, knob=KNOB_NONE):
        signs = write or read
        out.append([dtype, n, c, x_hw[0], x_hw[1], y_hw[0], y_hw[1], up, down, fu[0], fu[1], fd[0], fd[1], px0, py0, s_hw[0] if signs else 0,
                    s_hw[1] if signs else 0, sx, sy, f32(gain), f32(slope), f32(clamp), int(flip), int(write), int(read), partials, mirror, layout,
                    fd_odd, s_null, knob])

    def op(dtype, n, c, x_hw, up, down, fu, fd, pads, gain, slope, clamp, modes=('plain', 'write', 'adjoint'), flips=(0,), mirrors=(0,), **kw):
        """One op (separable filters: fu / fd = (taps, 0); full: (W, H)) as the plain forward, the sign-writing forward and the adjoint call
        filtered_lrelu.py::_adjoint derives from it (with and without the per-workgroup partials)."""
        yh, yw, sh, swb = _shape(lib, x_hw, up, down, fu, fd, pads)
        for flip in flips:
            for mirror in mirrors:
                if 'plain' in modes:
                    row(dtype, n, c, x_hw, (yh, yw), up, down, fu, fd, pads[0], pads[2], (0, 0), 0, 0, gain, slope, clamp, flip, 0, 0, mirror=mirror, **kw)
                if 'write' in modes:
                    row(dtype, n, c, x_hw, (yh, yw), up, down, fu, fd, pads[0], pads[2], (sh, swb), 0, 0, gain, slope, clamp, flip, 1, 0, mirror=mirror, **kw)
            if 'adjoint' in modes:
                cfg = fl._setup(up, down, list(pads), gain, slope, None if math.isinf(clamp) else clamp, bool(flip))
                shape_of = lambda f: torch.empty([f[1], f[0]] if f[1] else [f[0]])           # noqa: E731  (_adjoint reads the shapes alone)
                adj, sx, sy = fl._adjoint(cfg, shape_of(fu), shape_of(fd), x_hw, (yh, yw), 0, 0)
                back = _shape(lib, (yh, yw), adj.up, adj.down, fd, fu, (adj.px0, adj.px1, adj.py0, adj.py1))
                assert back[:2] == tuple(x_hw), (back, x_hw)
                for partials in (1, 0):
                    row(dtype, n, c, (yh, yw), x_hw, adj.up, adj.down, fd, fu, adj.px0, adj.py0, (sh, swb), sx, sy, adj.gain, adj.slope, adj.clamp, adj.flip,
                        0, 1, partials=partials, **kw)

    # every layer of T-1024 and R-1024, ToRGB's pointwise call included
    layers = {}
    for cfg in ('T1024', 'R1024'):
        layers[cfg] = []
        for L in O.layer_schedule(**CONFIGS[cfg])['layers']:
            side = L['in_size'] + L['conv_kernel'] - 1
            if L['is_torgb']:
                layers[cfg].append((L['out_channels'], side, 1, 1, (1, 1), (1, 1), L['padding'], 1.0, 1.0, False))
            else:
                fd = (L['down_taps'], L['down_taps'] if L['down_radial'] else 0)
                layers[cfg].append((L['out_channels'], side, L['up'], L['down'], (L['up_taps'], 0), fd, L['padding'], math.sqrt(2), 0.2, L['down_radial']))
        for n in (1, 4, 8):
            for dtype in (F32, F16):
                for c, side, up, down, fu, fd, pads, gain, slope, radial in layers[cfg]:
                    op(dtype, n, c, (side, side), up, down, fu, fd, pads, gain, slope, 256.0, flips=(0, 1) if radial else (0,), mirrors=(0, 1) if radial else (0,))
    # tests/test_gpu_flrelu_up4_occupancy.py: the up-4 layers of T-1024 at batch 2 as well
    for c, side, up, down, fu, fd, pads, gain, slope, radial in layers['T1024']:
        if up == 4:
            op(F32, 2, c, (side, side), up, down, fu, fd, pads, gain, slope, 256.0, modes=('plain',))

    # the shapes of the GPU tests
    for (n, c, h, w), up, taps, pads, radial in TEST_GEOMETRIES:
        for dtype in (F32, F16):
            op(dtype, n, c, (h, w), up, 2, (taps, 0), (12, 12 if radial else 0), pads, math.sqrt(2), 0.2, 256.0, flips=(0, 1) if radial else (0,),
               mirrors=(0, 1) if radial else (0,))
    for clamp, slope in ((4.0, 0.2), (math.inf, 0.2), (256.0, 0.0), (8.0, 1.0), (0.7, 0.2), (1.5, 0.2)):      # the non-linearity cases of the tests
        for (n, c, h, w), up, taps, pads, radial in TEST_GEOMETRIES[:1] + TEST_GEOMETRIES[6:8]:
            op(F32, n, c, (h, w), up, 2, (taps, 0), (12, 12 if radial else 0), pads, math.sqrt(2), slope, clamp)
    # Every layer of the networks has the same vertical phase per (up, down) -- VPH = (py0 - (up - 1)) mod down -- so half of the kernels
    # (three quarters of the down-4 adjoints) are met only with the top padding moved: by 0 .. 3 rows, on planes that pack and planes that
    # do not (58 .. 70 columns out), in every filter form
    for up, taps, pads, radial in ((2, 12, [9, 8, 9, 8], False), (4, 24, [-6, -9, -6, -9], False), (2, 12, [11, 10, 11, 10], True), (4, 24, [-2, -5, -2, -5], True)):
        for k in range(up):
            moved = pads[:2] + [pads[2] + k, pads[3] - k]
            narrow = 36 if radial else 38
            for w in ((narrow, 60 if up == 2 else 45) if k < 2 else (narrow,)):
                for dtype in (F32, F16):
                    op(dtype, 1, 2, (30, w), up, 2, (taps, 0), (12, 12 if radial else 0), moved, math.sqrt(2), 0.2, 256.0, flips=(0, 1) if radial else (0,),
                       mirrors=(0, 1) if radial else (0,), modes=('plain', 'write', 'adjoint') if k < 2 else ('adjoint',))
                    if up == 4 and not radial and k < 2:
                        op(dtype, 1, 2, (30, w), up, 2, (taps, 0), (12, 0), moved, math.sqrt(2), 0.2, 256.0, modes=('plain',), knob=KNOB_UP4_WIDE)
    for n, c, side, up, down, fu, fd, pad, read, write in ABI_GRID_CALLS:
        yh, yw, sh, swb = _shape(lib, (side, side), up, down, (fu, 0), (fd, 0), pad * 2)
        row(F32, n, c, (side, side), (yh, yw), up, down, (fu, 0), (fd, 0), pad[0], pad[0], (sh, swb), 0, 0, 1.4142135, 0.2, 256.0, 0, write, read)
    # a row-padded view (dense over (n, c): packs) is a matter of xStride[2] alone; x[::2] and a channels-last tensor are not dense
    op(F32, 2, 4, (38, 38), 2, 2, (12, 0), (12, 0), (9, 8, 9, 8), math.sqrt(2), 0.2, 256.0, modes=('plain',), layout=EVERY_SECOND_SAMPLE)
    op(F32, 2, 4, (150, 150), 2, 2, (12, 0), (12, 0), (9, 8, 9, 8), math.sqrt(2), 0.2, 256.0, modes=('plain',), layout=EVERY_SECOND_SAMPLE)
    op(F32, 2, 4, (38, 38), 2, 2, (12, 0), (12, 0), (9, 8, 9, 8), math.sqrt(2), 0.2, 256.0, layout=CHANNELS_LAST)

    # knobs, on a subset: the narrow, remainder and wide layers of both configurations at batch 1 and 8, and the small test shapes
    for knob in (KNOB_NOPACK, KNOB_SLOWACT, KNOB_UP4_WIDE):
        for cfg in ('T1024', 'R1024'):
            for n in (1, 8):
                for dtype in ((F32, F16) if knob == KNOB_UP4_WIDE else (F32,)):
                    for c, side, up, down, fu, fd, pads, gain, slope, radial in layers[cfg]:
                        op(dtype, n, c, (side, side), up, down, fu, fd, pads, gain, slope, 256.0, modes=('plain', 'write') if n == 1 else ('plain',),
                           mirrors=(1,) if radial else (0,), knob=knob)
        for (n, c, h, w), up, taps, pads, radial in TEST_GEOMETRIES[:10]:
            op(F32, n, c, (h, w), up, 2, (taps, 0), (12, 12 if radial else 0), pads, math.sqrt(2), 0.2, 256.0, modes=('plain',), knob=knob)

    # refusals
    op(F32, 1, 4, (38, 38), 3, 2, (18, 0), (12, 0), (9, 8, 9, 8), math.sqrt(2), 0.2, 256.0, modes=('plain', 'write'))                 # up 3
    op(F32, 1, 4, (38, 38), 2, 4, (12, 0), (24, 0), (20, 35, 20, 35), math.sqrt(2), 0.2, 256.0, modes=('plain', 'write'))             # down 4 without readSigns
    yh, yw, sh, swb = _shape(lib, (38, 38), 2, 2, (12, 12), (12, 0), (9, 8, 9, 8))
    for write in (0, 1):                                                                                                              # 2-D fu without readSigns
        row(F32, 1, 4, (38, 38), (yh, yw), 2, 2, (12, 12), (12, 0), 9, 9, (sh, swb), 0, 0, math.sqrt(2), 0.2, 256.0, 0, write, 0)
    (n, c, h, w), up, taps, pads = (2, 4, 36, 36), 2, 12, [11, 10, 11, 10]
    op(F32, n, c, (h, w), up, 2, (taps, 0), (12, 12), pads, math.sqrt(2), 0.2, 256.0, modes=('plain', 'write'), fd_odd=1)             # 2-D fd not 16-byte aligned
    op(F32, n, c, (h, w), up, 2, (taps, 0), (12, 0), pads, math.sqrt(2), 0.2, 256.0, modes=('plain',), fd_odd=1)                      # (a separable one may be)
    op(F32, n, c, (h, w), up, 2, (taps, 0), (12, 0), pads, math.sqrt(2), 1.5, 256.0)                                                  # slope 1.5
    op(F32, n, c, (h, w), up, 2, (taps, 0), (12, 0), pads, math.sqrt(2), 0.2, -1.0, modes=('plain', 'write'))                         # clamp -1
    op(F32, n, c, (h, w), up, 2, (taps, 0), (12, 0), pads, math.sqrt(2), 0.2, 256.0, modes=('write', 'adjoint'), s_null=1)            # signs without a tensor
    # a grid past 2^31 - 1 workgroups: 1.43e9 planes of two strips.  (The second check of the launch, on the one-launch mixed form, cannot
    # trip once the first has passed: planes x (nFull + 1/2) < planes x (nFull + 1) workgroups.)
    op(F32, 65536, 21846, (38, 150), 2, 2, (12, 0), (12, 0), (9, 8, 9, 8), math.sqrt(2), 0.2, 256.0, modes=('plain', 'write'))

    seen, uniq = set(), []
    for c in out:
        if tuple(c) not in seen:
            seen.add(tuple(c)); uniq.append(c)
    return uniq


def launch_row(call, la):
    """One recorded launch -> a row of LAUNCH_COLUMNS"""
    (gx, gy, gz), block = la['grid'], la['block']
    assert gy == 1 and gz == 1 and la['lds'] == 0
    m = re.search(r'flrelu_stream_kernel<([^>]*)>', la['kernel'])
    if m is None:
        assert re.search(r'flrelu_pointwise_kernel<(float|half)>', la['kernel']).group(1) == ('float' if call[0] == F32 else 'half'), la
        return [POINTWISE] + [0] * 7 + [gx, block] + [0] * 6 + [gx, 0]
    args = [a.strip() for a in m.group(1).split(',')]
    assert args[0] == ('float' if call[0] == F32 else 'half') and len(args) == 8 and block == 64 and gx == la['totalBlocks'], la
    return [STREAM] + [int(a) for a in args[1:]] + [gx, block] + [la[k] for k in ('nStrips', 'TW', 'ox0Base', 'wideBlocks', 'nChunks', 'CH', 'totalBlocks', 'fastAct')]


def main():
    recorder = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, 'flrelu_dispatch.json')
    cs = calls()
    rows = {}
    knob_col = CALL_COLUMNS.index('knob')
    for env_knob in (None, KNOB_NOPACK):
        part = [i for i, c in enumerate(cs) if (c[knob_col] == KNOB_NOPACK) == (env_knob == KNOB_NOPACK)]
        with tempfile.NamedTemporaryFile('w', suffix='.txt', delete=False) as f:
            f.write(''.join(' '.join(repr(v) if isinstance(v, float) else str(v) for v in cs[i]) + '\n' for i in part))
        env = {k: v for k, v in os.environ.items() if not k.startswith('SG3_FLRELU_')}
        env.update(KNOB_ENV.get(env_knob, {}))
        recs = [json.loads(line) for line in subprocess.run([recorder, f.name], check=True, capture_output=True, text=True, env=env).stdout.splitlines()]
        os.unlink(f.name)
        assert len(recs) == len(part)
        for i, r in zip(part, recs):
            assert len(r['launches']) <= 2 and (r['rc'] == 0) == (len(r['launches']) > 0), (cs[i], r)
            launches = [launch_row(cs[i], la) for la in r['launches']] + [[0] * len(LAUNCH_COLUMNS)] * (2 - len(r['launches']))
            rows[i] = cs[i] + [r['rc'], r['ppw']] + r['grid'] + [len(r['launches'])] + launches[0] + launches[1]
    packed = compact([rows[i] for i in range(len(cs))])
    with open(out, 'w') as f:
        f.write('{"call_columns": %s, "query_columns": %s, "launch_columns": %s, "second_launch_columns": %s, "rows": [\n'
                % tuple(json.dumps(c) for c in (PACKED_CALL_COLUMNS, QUERY_COLUMNS, PACKED_LAUNCH_COLUMNS, SECOND_LAUNCH_COLUMNS)))
        f.write(',\n'.join(json.dumps(r, separators=(',', ':')) for r in packed))
        f.write('\n]}\n')
    print(f'{len(cs)} calls in {len(packed)} rows -> {out}')


# The committed form of the table.  Calls that differ in the tensor type alone, or in whether the adjoint's partials are asked for, and
# were recorded with the same result share a row: `dtypes` / `partials` are sets of the values as bits (1 << value).  A row ends after
# the launches it has; what a launch repeats is left out after being checked here: grid == totalBlocks, 64 | 256 threads, the row
# chunks of the stream_grid query, and in the second launch every template coordinate of the first but G.
# tests/test_flrelu_dispatch_cpu.py::_load_table undoes all of it.
PACKED_CALL_COLUMNS = ['dtypes' if c == 'dtype' else c for c in CALL_COLUMNS]
PACKED_LAUNCH_COLUMNS = ['kind', 'U', 'D', 'VPH', 'RADIAL', 'SIGNS', 'G', 'WIDE', 'nStrips', 'TW', 'ox0Base', 'wideBlocks', 'totalBlocks', 'fastAct']
SECOND_LAUNCH_COLUMNS = ['G', 'nStrips', 'TW', 'ox0Base', 'wideBlocks', 'totalBlocks']


def compact(rows):
    nc, nq, nl = len(CALL_COLUMNS), len(QUERY_COLUMNS), len(LAUNCH_COLUMNS)
    out = []
    for r in rows:
        call, q = list(r[:nc]), dict(zip(QUERY_COLUMNS, r[nc:nc + nq]))
        las = [dict(zip(LAUNCH_COLUMNS, r[nc + nq + i * nl:])) for i in range(q['launches'])]
        row = call + r[nc:nc + nq]
        for i, la in enumerate(las):
            assert la['grid'] == la['totalBlocks'] and la['block'] == (64 if la['kind'] == STREAM else 256), r
            if la['kind'] == STREAM:
                assert q['gridOk'] == 1 and (la['nChunks'], la['chunkRows']) == (q['gridChunks'], q['gridChunkRows']), r
            if i == 1:
                assert all(la[k] == las[0][k] for k in LAUNCH_COLUMNS if k not in SECOND_LAUNCH_COLUMNS + ['grid']), r
            row += [la[k] for k in (PACKED_LAUNCH_COLUMNS if i == 0 else SECOND_LAUNCH_COLUMNS)]
        out.append(row)
    for col in ('dtype', 'partials'):
        i = CALL_COLUMNS.index(col)
        merged = {}
        for r in out:
            key = tuple(r[:i] + r[i + 1:])
            merged.setdefault(key, r[:i] + [0] + r[i + 1:])[i] |= 1 << r[i]
        out = list(merged.values())
    return out


if __name__ == '__main__':
    main()
