"""Time the StyleCLIP delta_i_c sweep on seeded T-1024 / R-1024 weights with the stand-in image encoder of the tests
(tests/delta_i_c_cases.py; its share is the stand-in's, not ViT-B/32's) or, with --encoder clip, with the package's own CLIP at
the full ViT-B/32 size on seeded weights (tests/clip_cases.py 'b32'; the kernels' time does not depend on the weights' values).

Per configuration and num_samples in {1, 8}: channels per second over a window of consecutive channels through
`compute_clip_features` (host clock around work that ends in a device synchronise), and the split of device time between synthesis,
preprocessing and the encoder (device events around the three stages of the same batches).  Then the fused preprocessing op
against the torch composite at B in {1, 32} from 1024 x 1024, alternating the two in one timed loop.  From the measured rates the
time of a full sweep at num_samples 1 and 300 is extrapolated (channels x 2 x num_samples images at the measured images per
second) and labelled as such.  Prints one JSON line.
    python tools/time_delta_i_c.py [--configs T1024 R1024] [--channels 128] [--reps 3] [--encoder stand-in|clip]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import delta_i_c_cases as cases  # noqa: E402
from helpers import build_product_generator  # noqa: E402

DEV = 'cuda:0'
MAX_BATCH = 32


def op_times(b, reps=50):
    """(fused us, composite us) per call at [b,3,1024,1024] -> 224 x 224, the two alternated inside the timed loop."""
    from torch_utils.ops.clip_preprocess import clip_preprocess, composite
    x = torch.from_numpy(cases.noise((b, 3, 1024, 1024), 1.0)).to(DEV)
    out = torch.empty([b, 3, 224, 224], device=DEV)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for _ in range(5):
        clip_preprocess(x, out=out)
        composite(x)
    torch.cuda.synchronize()
    for e in ev:
        e[0].record()
        clip_preprocess(x, out=out)
        e[1].record()
        composite(x)
        e[2].record()
    torch.cuda.synchronize()
    fused = float(np.median([e[0].elapsed_time(e[1]) for e in ev])) * 1e3
    comp = float(np.median([e[1].elapsed_time(e[2]) for e in ev])) * 1e3
    return fused, comp


def stage_split(G, latents, ends, encoder, first, channels, **kw):
    """Device milliseconds in (synthesis, preprocessing, encoder) over the batches of `channels` channels from `first`."""
    from editing.styleclip_global_directions.preprocess.create_delta_i_c import sweep_items
    from torch_utils.ops.clip_preprocess import clip_preprocess
    n = int(latents['input'].shape[0])
    marks = []
    with torch.no_grad():
        for i0 in range(first * 2 * n, (first + channels) * 2 * n, MAX_BATCH):
            s = sweep_items(latents, ends, i0, min(i0 + MAX_BATCH, (first + channels) * 2 * n))
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            img = G.synthesis(None, all_s=s, noise_mode='const', **kw)
            e[1].record()
            pre = clip_preprocess(img)
            e[2].record()
            encoder(pre)
            e[3].record()
            marks.append(e)
    torch.cuda.synchronize()
    return [sum(e[k].elapsed_time(e[k + 1]) for e in marks) for k in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', nargs='+', default=['T1024', 'R1024'])
    ap.add_argument('--channels', type=int, default=128, help='channels in the timed window at num_samples 1 (an eighth of it at 8)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--force-fp32', action='store_true')
    ap.add_argument('--encoder', choices=['stand-in', 'clip'], default='stand-in', help="clip: the native ViT-B/32 (models/clip) on seeded weights")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_delta_i_c.py measures on a GPU; none is visible')
    from editing.styleclip_global_directions.preprocess.create_delta_i_c import _endpoints, compute_clip_features
    from editing.styleclip_global_directions.preprocess.s_statistics import compute_stats
    kw = dict(force_fp32=True) if a.force_fp32 else {}
    res = {'box': torch.cuda.get_device_name(0), 'max_batch': MAX_BATCH, 'force_fp32': bool(a.force_fp32),
           'encoder': 'stand-in (8x8 pool, 192x16 matrix)' if a.encoder == 'stand-in' else 'native ViT-B/32, 12 layers, seeded weights, HIP kernels'}
    for b in (1, 32):
        fused, comp = op_times(b)
        res[f'preprocess_b{b}_fused_us'], res[f'preprocess_b{b}_composite_us'] = fused, comp
    if a.encoder == 'clip':
        import clip_cases
        encoder = clip_cases.build('b32', device=DEV).encode_image
    else:
        encoder = cases.StandInEncoder()
    for cfg in a.configs:
        G = build_product_generator(cfg, device=DEV)
        _, all_s, (_, mean, std) = compute_stats(G, random_state=3, num_images=64, batch=16)
        total = sum(int(v.shape[1]) for v in all_s.values())
        res[f'{cfg}_channels'] = total
        first = total // 3                                        # a window inside the sweep: earlier channels already at + strength
        for n in (1, 8):
            latents = {k: torch.from_numpy(v[:n]).to(DEV) for k, v in all_s.items()}
            channels = max(MAX_BATCH // (2 * n), a.channels // n)

            def run():
                return compute_clip_features(G, latents, mean, std, encoder, max_batch=MAX_BATCH, channel_range=(first, first + channels), **kw)
            run()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter()
                run()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t)
            t = float(np.median(ts))
            split = stage_split(G, latents, _endpoints(latents, mean, std, 5), encoder, first, channels, **kw)
            key = f'{cfg}_n{n}'
            res[f'{key}_window_channels'], res[f'{key}_window_s'], res[f'{key}_window_s_min_max'] = channels, t, [min(ts), max(ts)]
            res[f'{key}_channels_per_s'] = channels / t
            res[f'{key}_images_per_s'] = channels * 2 * n / t
            res[f'{key}_device_ms_synthesis_preprocess_encoder'] = split
            res[f'{key}_share_synthesis_preprocess_encoder'] = [v / sum(split) for v in split]
        res[f'{cfg}_extrapolated_full_sweep_s_n1'] = total / res[f'{cfg}_n1_channels_per_s']
        res[f'{cfg}_extrapolated_full_sweep_h_n300'] = total * 600 / res[f'{cfg}_n8_images_per_s'] / 3600
        del G
        torch.cuda.empty_cache()

    def rnd(v):
        return round(v, 4) if isinstance(v, float) else ([rnd(q) for q in v] if isinstance(v, list) else v)
    print(json.dumps({k: rnd(v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
