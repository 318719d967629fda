"""Time forward plus backward of the CLIP loss at the full ViT-B/32 size (seeded weights, tests/clip_cases.py 'b32'; kernel time
does not depend on the weights' values), from 1024 x 1024 images.

  CLIPLoss(image, text).mean().backward() at batches 1, 8 and 32: (a) the float16-weight 'torch' composite under autograd (library
  GEMMs; the image preparation is the fused kernel for both, so the difference is the tower) and (b) the HIP path, forward and
  backward on the transformer kernels, on the same GPU, the two alternated inside one timed loop so clock drift hits both alike;
  the image preparation alone, forward plus adjoint: the fused kernel against the two torch modules it replaces;
  the four data-gradient GEMM shapes of a block at M = 50 x batch alone: the kernel (with the epilogue the backward uses) against
  torch.matmul in float16 on the same operands (matmul only).

Device events around each call, `--warmup` untimed rounds, `--reps` timed rounds; median, min and max are reported.  The clock is
whatever the device runs at under this load (not pinned).  Prints one JSON line.
    python tools/time_clip_loss.py [--batches 1 8 32] [--reps 20] [--warmup 5] [--size 1024]"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import clip_cases as cases  # noqa: E402
from time_clip_encoder import alternate  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', nargs='+', type=int, default=[1, 8, 32])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--size', type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_clip_loss.py measures on a GPU; none is visible')
    import types
    from criteria.clip_loss import CLIPLoss
    from models.clip import convert_weights
    from torch_utils import _sg3abi as abi
    from torch_utils.ops import clip_resample
    from torch_utils.ops import clip_transformer as ct
    m = cases.build('b32', device=DEV)
    mh = convert_weights(copy.deepcopy(m))
    mh.impl = 'torch'                       # the yardstick is the composite under autograd
    opts = types.SimpleNamespace(stylegan_size=a.size, clip_checkpoint_path=None)
    loss_hip, loss_half = CLIPLoss(opts, model=m), CLIPLoss(opts, model=mh)
    text = torch.from_numpy(cases.tokens('b32', 1)).to(DEV)
    res = {'box': torch.cuda.get_device_name(0), 'model': 'ViT-B/32, 12 layers, seeded weights', 'stylegan_size': a.size, 'reps': a.reps,
           'warmup': a.warmup, 'clock': 'not pinned', 'ms': '[median, min, max] per call of loss.mean().backward()'}
    k = a.size // 32
    for b in a.batches:
        r = np.random.RandomState(b)
        image = torch.from_numpy(r.randn(min(b, 2), 3, a.size, a.size).astype(np.float32)).to(DEV).repeat((b + 1) // 2, 1, 1, 1)[:b].contiguous().requires_grad_(True)

        def step(fn):
            image.grad = None
            with torch.backends.cudnn.flags(enabled=fn is loss_hip):      # the composite's patch convolution on torch's im2col + GEMM path:
                fn(image, text).mean().backward()                         # through MIOpen its backward is compiled per batch size at first use

        before = abi.launch_count
        step(loss_hip)
        res[f'b{b}_hip_launches'] = abi.launch_count - before
        hip, half = alternate(lambda: step(loss_hip), lambda: step(loss_half), a.reps, a.warmup)
        res[f'b{b}_hip_ms'], res[f'b{b}_torch_fp16_ms'], res[f'b{b}_hip_over_torch_fp16_time'] = hip, half, hip[0] / half[0]
        # the image preparation alone, forward + adjoint
        dy = torch.ones([b, 3, a.size * 7 // k, a.size * 7 // k], device=DEV)

        def prep(fn):
            image.grad = None
            fn(image, 7, k).backward(dy)

        fused, modules = alternate(lambda: prep(clip_resample.nearest_up_avg_pool), lambda: prep(clip_resample.composite), a.reps, a.warmup)
        res[f'b{b}_resample_fused_ms'], res[f'b{b}_resample_torch_ms'] = fused, modules
        # the data-gradient GEMMs of one block, alone
        M = 50 * b
        for name, K, N, epi in (('c_proj_T', 768, 3072, abi.SG3_CLIP_EPI_DQUICKGELU_F16), ('c_fc_T', 3072, 768, abi.SG3_CLIP_EPI_F32),
                                ('out_proj_T', 768, 768, abi.SG3_CLIP_EPI_F16), ('qkv_T', 2304, 768, abi.SG3_CLIP_EPI_F32)):
            r = np.random.RandomState(K + N)
            stream = epi != abi.SG3_CLIP_EPI_F32                      # these two read the float32 gradient stream
            A = torch.from_numpy(r.randn(M, K)).to(DEV).float()
            A = A if stream else A.half()
            A16 = A.half()
            W = torch.from_numpy(r.randn(N, K) / np.sqrt(K)).to(DEV).half()
            out = torch.zeros([M, N], device=DEV, dtype=ct._OUT_DTYPE[epi])
            aux = torch.zeros([M, N], device=DEV, dtype=torch.float16) if epi == abi.SG3_CLIP_EPI_DQUICKGELU_F16 else None
            Wt = W.t()
            hip, lib = alternate(lambda: ct.gemm(A, W, None, out, epi, M, aux=aux), lambda: torch.matmul(A16, Wt), a.reps, a.warmup)
            flop = 2.0 * M * K * N
            res[f'gemm_{name}_M{M}_K{K}_N{N}'] = {'hip_us': [v * 1e3 for v in hip], 'matmul_fp16_us': [v * 1e3 for v in lib],
                                                  'hip_tflops': flop / hip[0] / 1e9, 'matmul_tflops': flop / lib[0] / 1e9,
                                                  'hip_over_matmul_time': hip[0] / lib[0]}

    def rnd(v):
        if isinstance(v, float):
            return round(v, 4)
        if isinstance(v, list):
            return [rnd(q) for q in v]
        return {k: rnd(q) for k, q in v.items()} if isinstance(v, dict) else v
    print(json.dumps({k: rnd(v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
