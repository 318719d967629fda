"""Time the native CLIP image encoder at the full ViT-B/32 size (seeded weights, tests/clip_cases.py 'b32'; kernel time does not
depend on the weights' values).

  encode_image at batches 1, 8, 32 and 128: images per second of (a) the 'torch' composite with float16 weights (library GEMMs,
  about a dozen launches per block) and (b) the HIP kernels (seven launches per block), on the same GPU, the two alternated
  inside one timed loop so clock drift hits both alike;
  every GEMM shape of a block at M = 50 x batch alone: the kernel (with the epilogue the block uses) against torch.matmul in
  float16 on the same operands (matmul only: the library's time excludes the bias, activation and residual it would need).

Device events around each call, `--warmup` untimed rounds, `--reps` timed rounds; median, min and max are reported.  The clock is
whatever the device runs at under this load (not pinned; the min / max spread shows how steady it was).  Prints one JSON line.
    python tools/time_clip_encoder.py [--batches 1 8 32 128] [--reps 20] [--warmup 5]"""
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

DEV = 'cuda:0'


def alternate(fa, fb, reps, warmup):
    """Milliseconds per call of fa and fb, alternated: ([median, min, max] of fa, the same of fb)."""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record(); fa(); e[1].record(); fb(); e[2].record()
    torch.cuda.synchronize()
    ta, tb = [e[0].elapsed_time(e[1]) for e in ev], [e[1].elapsed_time(e[2]) for e in ev]
    return [float(np.median(ta)), min(ta), max(ta)], [float(np.median(tb)), min(tb), max(tb)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', nargs='+', type=int, default=[1, 8, 32, 128])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_clip_encoder.py measures on a GPU; none is visible')
    from models.clip import convert_weights
    from torch_utils import _sg3abi as abi
    from torch_utils.ops import clip_transformer as ct
    m = cases.build('b32', device=DEV)
    mh = convert_weights(copy.deepcopy(m))
    res = {'box': torch.cuda.get_device_name(0), 'model': 'ViT-B/32 image tower, 12 layers, seeded weights', 'reps': a.reps, 'warmup': a.warmup,
           'clock': 'not pinned', 'ms': '[median, min, max] per call'}
    with torch.no_grad():
        for b in a.batches:
            x = torch.from_numpy(cases.images('b32', min(b, 8))).to(DEV).repeat((b + 7) // 8, 1, 1, 1)[:b].contiguous()
            hip, half = alternate(lambda: m.encode_image(x, impl='hip'), lambda: mh.encode_image(x, impl='torch'), a.reps, a.warmup)
            res[f'b{b}_hip_ms'], res[f'b{b}_torch_fp16_ms'] = hip, half
            res[f'b{b}_hip_img_per_s'], res[f'b{b}_torch_fp16_img_per_s'] = b * 1e3 / hip[0], b * 1e3 / half[0]
        # the GEMM shapes of one block, alone
        for b in a.batches:
            M = 50 * b
            for name, K, N, epi in (('qkv', 768, 2304, abi.SG3_CLIP_EPI_F16), ('out_proj', 768, 768, abi.SG3_CLIP_EPI_RESIDUAL),
                                    ('c_fc', 768, 3072, abi.SG3_CLIP_EPI_QUICKGELU_F16), ('c_proj', 3072, 768, abi.SG3_CLIP_EPI_RESIDUAL)):
                r = np.random.RandomState(K + N)
                A = torch.from_numpy(r.randn(M, K)).to(DEV).half()
                W = torch.from_numpy(r.randn(N, K) / np.sqrt(K)).to(DEV).half()
                bias = torch.zeros(N, device=DEV)
                out = torch.zeros([M, N], device=DEV, dtype=ct._OUT_DTYPE[epi])
                Wt = W.t()
                hip, lib = alternate(lambda: ct.gemm(A, W, bias, out, epi, M), lambda: torch.matmul(A, Wt), a.reps, a.warmup)
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
