"""Regenerates tests/golden/conv2d_dispatch.json: what sg3_conv2d, sg3_conv2d_dgrad and sg3_conv2d_wgrad_sum launch for a fixed list of
calls, and what sg3_conv2d_form and sg3_conv2d_wgrad_sum_splits answer for them.

The table is RECORDED, not computed by the code it pins: csrc/sg3_conv2d.hip, csrc/sg3_conv2d_dgrad.hip and csrc/sg3_conv2d_wgrad_sum.hip
are compiled with modconv_dispatch_recorder.h force-included (the launch macro writes down kernel name with template arguments, grid,
workgroup, LDS bytes and the tile geometry of the parameter block) and linked with conv2d_dispatch_recorder.cpp; this script makes the
list of calls, runs that program and stores the result.  The committed table came from the commit BEFORE the choice moved into
csrc/sg3_conv2d_plan.h.

    hipcc -O1 -std=c++17 -fPIC --offload-arch=gfx950 -Iinclude -I<csrc> -include tests/golden/modconv_dispatch_recorder.h -c <csrc>/sg3_conv2d.hip -o a.o
    (the same for sg3_conv2d_dgrad.hip -> b.o and sg3_conv2d_wgrad_sum.hip -> c.o, and -x hip -c tests/golden/conv2d_dispatch_recorder.cpp -> m.o)
    hipcc -rdynamic m.o a.o b.o c.o -ldl -o recorder
    python tests/golden/make_conv2d_dispatch.py recorder
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

CALL_COLUMNS = ['entry', 'N', 'I', 'O', 'H', 'W', 'k', 'stride', 'pad', 'precision', 'cus']
# what the launch says (0 where a kernel has none), `form` of sg3_conv2d_form (-1: not a forward) and `nSplit`, `chunksPerSplit`, `xSegs` of
# sg3_conv2d_wgrad_sum_splits
PLAN_COLUMNS = ['rc', 'family', 'form', 'KS', 'STRIDE', 'WM', 'WN', 'TM', 'TN', 'CHAINS', 'nch', 'xTiles', 'yTiles', 'mTiles', 'outH', 'outW',
                'xSegs', 'nChunks', 'nSplit', 'chunksPerSplit', 'oTiles', 'iTiles', 'reduceGrid', 'grid', 'block', 'ldsBytes']
FORWARD, DGRAD, WGRAD_SUM = 0, 1, 2                   # `entry`
FP32, F16X3, FP32_CHAINS = 0, 1, 5                    # SG3_CONV_*
FP32_MFMA, FAMILY_F16X3, FAMILY_DGRAD, FAMILY_WGRAD_SUM = range(4)      # SG3_CONV2D_*: `family`
CUS, OTHER_CUS = 256, 128
BATCHES = (1, 4, 16)


def conv_shapes(net, parts, side, input_nc):
    """(I, O, H, W, k, stride, pad) of every Conv2d under `parts` of `net` outside the squeeze-and-excitation gates, in call order, from
    forward hooks on a CPU forward of one side x side image."""
    import torch
    from models.setgan.encoder.encoders.helpers import SEModule
    gates = {id(c) for m in net.modules() if isinstance(m, SEModule) for c in m.modules()}
    out, hooks = [], []

    def hook(mod, inp, _):
        assert mod.kernel_size[0] == mod.kernel_size[1] and mod.stride[0] == mod.stride[1] and mod.padding[0] == mod.padding[1]
        out.append((mod.in_channels, mod.out_channels, int(inp[0].shape[2]), int(inp[0].shape[3]), mod.kernel_size[0], mod.stride[0], mod.padding[0]))

    for part in parts:
        for m in part.modules():
            if isinstance(m, torch.nn.Conv2d) and id(m) not in gates:
                hooks.append(m.register_forward_hook(hook))
    with torch.no_grad():
        net.eval()(torch.zeros([1, input_nc, side, side]))
    for h in hooks:
        h.remove()
    return out


def calls():
    """The list: rows of CALL_COLUMNS."""
    import math
    import torch
    from criteria.lpips.networks import get_network
    from models.setgan.encoder.encoders.model_irse import Backbone
    from models.setgan.encoder.encoders.restyle_psp_encoders import BackboneEncoder, ResNetBackboneEncoder
    from torch_utils.ops import lpips_ops
    import encoder_train_cases
    import id_loss_cases
    import test_gpu_encoder_numerics as numerics
    import test_gpu_id_loss
    out = []

    def forward(n, i, o, h, w, k, s, pad, precisions, cus=CUS):
        for prec in precisions:
            out.append([FORWARD, n, i, o, h, w, k, s, pad, prec, cus])

    def grad(entry, n, i, o, h, w, k, s):
        out.append([entry, n, i, o, h, w, k, s, k // 2, FP32, CUS])

    # IR-SE50 BackboneEncoder at 256 x 256, input_nc = 6: stem, every unit's two convolutions and the projection shortcuts under both
    # eval precisions and as the recorded training forward (four chains), their data and weight gradients (training the trunk), and level 1
    # of all style heads: one stride-2 convolution over the strip image (_StyleHeadEncoder._forward_kernels)
    enc = BackboneEncoder(50, 'ir_se')
    trunk = conv_shapes(enc, (enc.input_layer, enc.body), 256, 6)
    assert len(trunk) == 1 + 24 * 2 + 3                 # stem, two per unit, three projections
    heads, sw = len(enc.styles), 16
    for n in BATCHES:
        for i, o, h, w, k, s, pad in trunk:
            assert pad == k // 2
            forward(n, i, o, h, w, k, s, pad, (F16X3, FP32, FP32_CHAINS))
            grad(DGRAD, n, i, o, h, w, k, s)
            grad(WGRAD_SUM, n, i, o, h, w, k, s)
        forward(1, 512, heads * 512, 16, (sw + 2 - (sw & 1)) * n, 3, 2, 1, (F16X3, FP32))
    # the identity loss: the IR-SE50 Backbone at 112 x 112, forward and the data gradient back to the image
    net = Backbone(112, 50, mode='ir_se', drop_ratio=0.6)
    for n in BATCHES:
        for i, o, h, w, k, s, pad in conv_shapes(net, (net.input_layer, net.body), 112, 3):
            forward(n, i, o, h, w, k, s, pad, (F16X3, FP32))
            grad(DGRAD, n, i, o, h, w, k, s)
    # the 16 blocks of ResNetBackboneEncoder
    res = ResNetBackboneEncoder()
    blocks = conv_shapes(res, (res.body,), 256, 6)
    assert len(res.body) == 16 and len(blocks) == 2 * 16 + 3
    for n in BATCHES:
        for i, o, h, w, k, s, pad in blocks:
            forward(n, i, o, h, w, k, s, pad, (F16X3, FP32))
    # LPIPS at 256 x 256: the first layer as a 3x3 convolution over the pixel-unshuffled canvas of lpips_ops.prepare, then the three 3x3
    # layers of AlexNet, exact fp32, with their data gradients (criteria/lpips/lpips.py::_operands)
    alex = get_network('alex')
    oh, ow = lpips_ops.conv1_out_size(256, 256)
    lpips = [(48, alex.layers[0].out_channels, oh + 2, ow + 2, 3, 1, 0)] + [c for c in conv_shapes(alex, (alex.layers,), 256, 3) if c[4] == 3]
    assert len(lpips) == 4
    for n in BATCHES:
        for i, o, h, w, k, s, pad in lpips:
            forward(n, i, o, h, w, k, s, pad, (FP32,))
            grad(DGRAD, n, i, o, h, w, k, s)                 # (the valid first layer: the pad-1 transpose of dy in a frame of zeros)

    # the case lists of the GPU tests, for 256 CUs
    numerics._cus = lambda: CUS
    for n, ci, co, h, w, k, s, pad, *_ in numerics._form_cases():
        forward(n, ci, co, h, w, k, s, pad, (FP32, F16X3))
    for n, ci, co, h, w, k, s, pad in numerics._split_form_shapes():
        forward(n, ci, co, h, w, k, s, pad, (FP32, F16X3))
    for k, s, i, o, h, w in test_gpu_id_loss.DGRAD_SHAPES:
        grad(DGRAD, 2, i, o, h, w, k, s)
    for cin, depth, s, h, w in id_loss_cases.UNIT_SHAPES:           # one residual unit: conv1, conv2, the projection
        unit = [(cin, depth, h, w, 3, 1), (depth, depth, h, w, 3, s)] + ([(cin, depth, h, w, 1, s)] if cin != depth else [])
        for i, o, uh, uw, k, us in unit:
            forward(2, i, o, uh, uw, k, us, k // 2, (FP32, F16X3))
            grad(DGRAD, 2, i, o, uh, uw, k, us)
    for n in (2, 3):
        for k, s, i, o, h, w in encoder_train_cases.WGRAD_SHAPES + [(3, 1, 64, 64, 256, 256), (3, 2, 256, 512, 32, 32), (1, 2, 256, 512, 32, 32)]:
            grad(WGRAD_SUM, n, i, o, h, w, k, s)
    grad(WGRAD_SUM, 3, 40, 20, 5, 70, 3, 1)                         # tests/test_gpu_encoder_train.py, besides WGRAD_SHAPES
    # the one branch that reads the CU count: 3x3 stride 1 f16x3 above 16 rows with 2 cus - 1 and with 2 cus eight-row tiles, each
    # under both CU counts
    for cus in (CUS, OTHER_CUS):
        for n, h in {CUS: ((73, 56), (64, 64)), OTHER_CUS: ((85, 24), (32, 64))}[cus]:
            assert n * math.ceil(h / 8) in (2 * cus - 1, 2 * cus) and h > 16
            for c in (CUS, OTHER_CUS):
                forward(n, 16, 64, h, 32, 3, 1, 1, (F16X3,), cus=c)
    # kernels none of the above reaches: four chains on the 32-channel tile, and on the 64-channel tile for 1x1 stride 1 (the trunk's
    # recorded training forward has no convolution that narrow, and 1x1 only with stride 2)
    for k in (1, 3):
        for s in (1, 2):
            forward(1, 37, 70, 13, 9, k, s, k // 2, (FP32_CHAINS,))
            forward(3, 9, 29, 23, 35, k, s, k // 2, (FP32_CHAINS,))
    # grids past 2^31 - 1 workgroups
    forward(1 << 20, 8, 1 << 17, 8, 8, 1, 1, 0, (F16X3, FP32))
    grad(DGRAD, 1 << 30, 1, 1, 1, 1, 1, 2)

    seen, uniq = set(), []
    for c in out:
        if tuple(c) not in seen:
            seen.add(tuple(c)); uniq.append(c)
    return uniq


KERNELS = {   # kernel -> (family, template parameter names)
    'conv2d_mfma_kernel': (FP32_MFMA, ['KS', 'STRIDE', 'WM', 'WN', 'TM', 'TN', 'CHAINS']),
    'conv2d_f16x3_kernel': (FAMILY_F16X3, ['KS', 'STRIDE', 'WM', 'WN', 'TM', 'TN']),
    'conv2d_dgrad_kernel': (FAMILY_DGRAD, ['KS', 'STRIDE', 'WM', 'WN', 'TM', 'TN']),
    'conv2d_wgrad_sum_kernel': (FAMILY_WGRAD_SUM, ['KS', 'STRIDE']),
}


def plan_row(call, rec):
    """One recorded call -> a row of PLAN_COLUMNS"""
    c = dict(zip(CALL_COLUMNS, call))
    row = dict.fromkeys(PLAN_COLUMNS, 0)
    row['rc'] = rec['rc']
    row['form'] = rec['form'] if c['entry'] == FORWARD else -1
    if c['entry'] == WGRAD_SUM:
        assert rec['splits'][0] == rec['rc'] == 0, (call, rec)
        row['nSplit'], row['chunksPerSplit'], row['xSegs'] = rec['splits'][1:]
    if rec['rc'] != 0:
        assert not rec['launches'] and rec['rc'] == -2, (call, rec)
        return [row[k] for k in PLAN_COLUMNS]
    la = rec['launches'][0]
    name, args = re.search(r'(conv2d\w*_kernel)<([^>]*)>', la['kernel']).groups()
    row['family'], names = KERNELS[name]
    assert row['family'] == {FORWARD: FAMILY_F16X3 if c['precision'] == F16X3 else FP32_MFMA, DGRAD: FAMILY_DGRAD, WGRAD_SUM: FAMILY_WGRAD_SUM}[c['entry']], (call, rec)
    row.update(dict(zip(names, [int(a) for a in args.split(',')])))
    assert (row['KS'], row['STRIDE']) == (c['k'], c['stride'])
    (gx, gy, gz), lds = la['grid'], la['lds']
    assert gy == 1 and gz == 1 and la['attr'] == (lds if lds > 64 * 1024 else 0), (call, rec)
    row.update(grid=gx, block=la['block'], ldsBytes=lds)
    if row['family'] == FAMILY_WGRAD_SUM:
        for k in ('xSegs', 'nChunks', 'chunksPerSplit', 'oTiles', 'iTiles'):
            assert k not in ('xSegs', 'chunksPerSplit') or row[k] == la[k], (call, rec)
            row[k] = la[k]
        row['outH'], row['outW'] = la['OH'], la['OW']
        assert (len(rec['launches']) == 2) == (row['nSplit'] > 1), (call, rec)
        if row['nSplit'] > 1:
            red = rec['launches'][1]
            assert 'conv2d_wgrad_sum_reduce_kernel' in red['kernel'] and red['block'] == 256
            row['reduceGrid'] = red['grid'][0]
    else:
        assert len(rec['launches']) == 1 and la['totalBlocks'] == gx, (call, rec)
        for k in ('nch', 'xTiles', 'yTiles', 'mTiles'):
            row[k] = la[k]
    return [row[k] for k in PLAN_COLUMNS]


def main():
    recorder = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, 'conv2d_dispatch.json')
    cs = calls()
    rows = {}
    for cus in (CUS, OTHER_CUS):                                        # the recorder reads the CU count once per process
        part = [i for i, c in enumerate(cs) if c[-1] == cus]
        with tempfile.NamedTemporaryFile('w', suffix='.txt', delete=False) as f:
            f.write(''.join(' '.join(str(v) for v in cs[i][:-1]) + '\n' for i in part))
        env = dict(os.environ, REC_CUS=str(cus))
        recs = [json.loads(line) for line in subprocess.run([recorder, f.name], check=True, capture_output=True, text=True, env=env).stdout.splitlines()]
        os.unlink(f.name)
        assert len(recs) == len(part)
        for i, r in zip(part, recs):
            rows[i] = cs[i] + plan_row(cs[i], r)
    with open(out, 'w') as f:
        f.write('{"call_columns": %s, "plan_columns": %s, "rows": [\n' % (json.dumps(CALL_COLUMNS), json.dumps(PLAN_COLUMNS)))
        f.write(',\n'.join(json.dumps(rows[i], separators=(',', ':')) for i in range(len(cs))))
        f.write('\n]}\n')
    print(f'{len(cs)} rows -> {out}')


if __name__ == '__main__':
    main()
