"""Time forward plus backward of the identity loss (IR-SE50, seeded weights from tests/id_loss_cases.py; kernel time does not depend
on the weights' values) from 1024 x 1024 images at batch 2, as the mapper coach calls it: `id_loss(x_hat, x, x)[0].backward()`.

  (a) the package's own composite under autograd (face_pool fused for both, the network on torch's convolutions; a facenet whose
      parameters record a gradient takes it) and (b) the HIP path, recording forward and hand-written backward, on the same GPU,
      the two alternated inside one timed loop so clock drift hits both alike;
  the image preparation alone, forward plus adjoint: the fused kernel against the torch pools it replaces;
  the HIP path's parts alone: the no_grad forward, the recording forward, and the backward through the trunk, and four
  of its data-gradient shapes alone against torch's convolution backward on the same operands.

Device events around each call, `--warmup` untimed rounds, `--reps` timed rounds; median, min and max are reported.  The clock is
whatever the device runs at under this load (not pinned).  Prints one JSON line.
    python tools/time_id_loss.py [--batch 2] [--reps 20] [--warmup 5] [--size 1024]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests'), ROOT, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import id_loss_cases as cases  # noqa: E402
from time_clip_encoder import alternate  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--size', type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_id_loss.py measures on a GPU; none is visible')
    from criteria.id_loss import IDLoss
    from torch_utils import _sg3abi as abi
    from torch_utils.ops import face_pool as fp
    from torch_utils.ops.plain_conv_grad import PackedDgrad
    net = cases.build_backbone(DEV)
    net_torch = cases.build_backbone(DEV)
    net_torch.output_layer[4].bias.requires_grad_(True)            # a parameter that records a gradient: IDLoss takes the composite
    loss_hip, loss_torch = IDLoss(facenet=net), IDLoss(facenet=net_torch)
    b = a.batch
    x = cases.images(b, a.size, seed=1).to(DEV)
    x_hat = cases.perturbed(x.cpu(), seed=2).to(DEV).requires_grad_(True)
    assert loss_hip.uses_hip(x_hat) and not loss_torch.uses_hip(x_hat)
    res = {'box': torch.cuda.get_device_name(0), 'model': 'IR-SE50, seeded weights', 'size': a.size, 'batch': b, 'reps': a.reps, 'warmup': a.warmup,
           'clock': 'not pinned', 'ms': '[median, min, max] per call of id_loss(x_hat, x, x)[0].backward()'}

    def step(fn):
        x_hat.grad = None
        with torch.backends.cudnn.flags(enabled=True):
            fn(x_hat, x, x)[0].backward()

    step(loss_torch)
    step(loss_hip)                              # packs the weights: launches of their own, once
    before = abi.launch_count
    step(loss_hip)
    res['hip_calls'] = abi.launch_count - before
    hip, comp = alternate(lambda: step(loss_hip), lambda: step(loss_torch), a.reps, a.warmup)
    res['hip_ms'], res['torch_fp32_ms'], res['hip_over_torch_time'] = hip, comp, hip[0] / comp[0]

    dy = torch.ones([b, 3, 112, 112], device=DEV)

    def prep(fn):
        x_hat.grad = None
        fn(x_hat).backward(dy)

    fused, pools = alternate(lambda: prep(fp.face_pool), lambda: prep(fp.composite), a.reps, a.warmup)
    res['face_pool_fused_ms'], res['face_pool_torch_ms'] = fused, pools

    img = fp.face_pool(x_hat.detach())
    state = {}

    def fwd_plain():
        with torch.no_grad():
            net._forward_record(img, False)

    def fwd_record():
        with torch.no_grad():
            state['rec'] = net._forward_record(img, True)

    fwd_record()
    d = torch.randn([b, 512, 7, 7], device=DEV) * 1e-4

    def bwd():
        _, act, saved = state['rec']
        net._trunk_backward(net._packed, act, saved, d)

    res['trunk_forward_ms'], res['trunk_forward_record_ms'] = alternate(fwd_plain, fwd_record, a.reps, a.warmup)
    res['trunk_backward_ms'], _ = alternate(bwd, fwd_plain, a.reps, a.warmup)
    for name, (k, s, i, o, h) in {'conv2_s1_256_14': (3, 1, 256, 256, 14), 'conv2_s2_256_28': (3, 2, 256, 256, 28),
                                  'shortcut_s2_128_256_28': (1, 2, 128, 256, 28), 'conv1_s1_64_56': (3, 1, 64, 64, 56)}.items():
        r = np.random.RandomState(i + h)
        w = torch.from_numpy((r.randn(o, i, k, k) / np.sqrt(i * k * k)).astype(np.float32)).to(DEV)
        pd = PackedDgrad(w, stride=s)
        dyk = torch.from_numpy(r.randn(b, o, *pd.out_size(h, h)).astype(np.float32)).to(DEV)
        t_hip, t_lib = alternate(lambda: pd.run(dyk, (h, h)), lambda: torch.nn.grad.conv2d_input([b, i, h, h], w, dyk, stride=s, padding=k // 2), a.reps, a.warmup)
        flop = 2.0 * b * i * o * k * k * dyk.shape[2] * dyk.shape[3]
        res[f'dgrad_{name}'] = {'hip_us': [v * 1e3 for v in t_hip], 'torch_us': [v * 1e3 for v in t_lib], 'hip_tflops': flop / t_hip[0] / 1e9}

    def rnd(v):
        if isinstance(v, float):
            return round(v, 4)
        if isinstance(v, list):
            return [rnd(q) for q in v]
        return {k: rnd(q) for k, q in v.items()} if isinstance(v, dict) else v
    print(json.dumps({k: rnd(v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
