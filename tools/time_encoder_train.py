"""Time the trunk of `BackboneEncoder(50, 'ir_se')` in train mode, forward + backward, at 2 x 6 x 256 x 256 (the ReStyle coach's
shape; seeded weights from tests/encoder_train_cases.py, kernel time does not depend on their values):

  (a) the native node (`native_training = True`: batch-statistic BatchNorm, weight and data gradients on libsg3hip) and (b) the
      same modules under torch autograd (`_trunk_torch`, the library's convolutions, MIOpen enabled and warmed) on the same GPU, the
      two alternated inside one timed loop so clock drift hits both alike;
  the native node's forward and backward apart, and its ABI calls per step;
  the native kernels alone on the tensors of one 64 -> 64 unit at 128 x 128 and one 512 -> 512 unit at 16 x 16.

Device events around each call, `--warmup` untimed rounds, `--reps` timed rounds; median, min and max are reported.  The clock is
whatever the device runs at under this load (not pinned).  Prints one JSON line.
    python tools/time_encoder_train.py [--reps 20] [--warmup 5] [--size 256] [--precision fp32]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests'), ROOT, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import torch  # noqa: E402

import encoder_train_cases as cases  # noqa: E402
from time_clip_encoder import alternate  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--precision', default='fp32', choices=['fp32', 'f16x3'])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_encoder_train.py measures on a GPU; none is visible')
    from models.setgan.encoder.encoders.restyle_psp_encoders import _TrunkTrain
    from torch_utils import _sg3abi as abi
    from torch_utils.ops import batchnorm_train as bt
    from torch_utils.ops import plain_conv
    from torch_utils.ops.plain_conv_wgrad import wgrad
    enc = cases.make_encoder(7).float().to(DEV).train()
    enc.native_training = True
    enc.native_training_precision = plain_conv.precision = a.precision          # the unit kernels timed alone follow the module-wide one
    params = [p for _, p in cases.trunk_named_parameters(enc)]
    x = cases.randn(1, 2, 6, a.size, a.size).float().to(DEV)
    cot = cases.randn(2, 2, 512, a.size // 16, a.size // 16).float().to(DEV) * 1e-3
    res = {'box': torch.cuda.get_device_name(0), 'model': 'BackboneEncoder(50, ir_se) trunk, train mode, seeded weights', 'size': a.size, 'batch': 2,
           'reps': a.reps, 'warmup': a.warmup, 'clock': 'not pinned', 'ms': '[median, min, max] per call', 'forward_precision': a.precision}

    def native():
        torch.autograd.grad(_TrunkTrain.apply(enc, x, *params), params, cot)

    def library():
        torch.autograd.grad(enc._trunk_torch(x), params, cot)

    native()                                     # packs
    before = abi.launch_count
    native()
    res['hip_calls_per_step'] = abi.launch_count - before
    with torch.backends.cudnn.flags(enabled=True):
        library()
        hip, lib = alternate(native, library, a.reps, a.warmup)
    res['hip_fwd_bwd_ms'], res['torch_fp32_fwd_bwd_ms'], res['hip_over_torch_time'] = hip, lib, hip[0] / lib[0]

    state = {}

    def fwd():
        state['out'] = _TrunkTrain.apply(enc, x, *params)

    def bwd():
        torch.autograd.grad(state['out'], params, cot, retain_graph=True)

    fwd()
    res['hip_forward_ms'], res['hip_backward_ms'] = alternate(fwd, bwd, a.reps, a.warmup)

    # the kernels of one unit alone
    res['kernel_us'] = {}
    with torch.no_grad():
        for label, idx, c, hw in (('unit_64ch_128px', 1, 64, a.size // 2), ('unit_512ch_16px', 22, 512, a.size // 16)):
            unit = enc.body[idx]
            xin = cases.randn(3, 2, c, hw, hw).float().to(DEV)
            dout = cases.randn(4, 2, c, hw, hw).float().to(DEV)
            _, saved = unit.forward_train_record(xin)
            xs, st1, pre, h1, c2, st2, rs, mean, _, _, slope, tp = saved
            bn1, bn2 = unit.res_layer[0], unit.res_layer[4]
            db, dg = bt.backward_reduce(dout, c2, st2)
            kernels = {
                'bn_stats': lambda: bt.stats(xs, bn1.weight, bn1.bias, bn1.eps),
                'conv1_affine': lambda: tp['conv1'].run(xs, in_scale=st1.a, in_shift=st1.b),
                'prelu': lambda: bt.apply(pre, tp['one'], tp['zero'], slope=slope),
                'conv2': lambda: tp['conv2'].run(h1),
                'bn_apply': lambda: bt.apply(c2, st2.a, bn2.bias, centre=st2.mean, centre_lo=st2.mean_lo),
                'bn_bwd_reduce': lambda: bt.backward_reduce(dout, c2, st2),
                'bn_bwd_apply': lambda: bt.backward_apply(dout, c2, st2, db, dg),
                'wgrad2': lambda: wgrad(h1, dout, 3, 1),
                'dgrad2': lambda: tp['dgrad2'].run(dout, (hw, hw)),
                'slope_grad_mask': lambda: bt.slope_grad(dout, pre, slope),
                'wgrad1_affine': lambda: wgrad(xs, dout, 3, 1, in_scale=st1.a, in_shift=st1.b),
                'dgrad1': lambda: tp['dgrad1'].run(dout, (hw, hw)),
            }
            res['kernel_us'][label] = {}
            for name, fn in kernels.items():
                t, _ = alternate(fn, lambda: None, a.reps, a.warmup)
                res['kernel_us'][label][name] = [v * 1e3 for v in t]

    def rnd(v):
        if isinstance(v, float):
            return round(v, 4)
        if isinstance(v, list):
            return [rnd(q) for q in v]
        return {k: rnd(q) for k, q in v.items()} if isinstance(v, dict) else v
    print(json.dumps({k: rnd(v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
