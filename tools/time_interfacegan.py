"""Time the InterFaceGAN editing path at the README command's shape on seeded R-1024 weights:
N = 4 images, age / smile / pose x range(-5, 5), [4,3,3] landmark transforms, resize_outputs on and off.

Per batch: ReStyle inversion (5 steps), the three batched edit sweeps (120 images, mixed precision), and the finishing of the
strips on the device (`to_uint8`), against the reference's CPU finishing of the same images (tensor2im + PIL resize).  Then the
finishing kernel alone at B = 120 (1024 -> 256 and 1024 -> 1024, GB/s counted on input bytes) and one `pose` animation
(8 segments x 25 frames = 200 frames) batched against the reference's batch-1 loop.  Prints one JSON line.
    python tools/time_interfacegan.py [--reps 3] [--skip-reference-animation]"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import interfacegan_cases as cases  # noqa: E402
from helpers import build_restyle_pair  # noqa: E402

DEV = 'cuda:0'


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--skip-reference-animation', action='store_true')
    a = ap.parse_args()
    from editing.interfacegan.edit_synthetic import get_result_from_vecs, prepare_animation
    from editing.interfacegan.face_editor import FaceEditor
    from inversion.scripts import inference_editing as ie
    from torch_utils.ops.image_finish import to_uint8
    from utils.common import tensor2im
    res = {'box': torch.cuda.get_device_name(0), 'shape': 'N=4, age/smile/pose x range(-5,5), R-1024'}
    net, opts, *_ = build_restyle_pair('R1024', device=DEV, n_iters=5)
    opts = types.SimpleNamespace(**vars(opts))
    opts.edit_directions, opts.factor_ranges = ['age', 'smile', 'pose'], ['(-5_5)'] * 3
    editor = FaceEditor(net.decoder, directions=cases.directions(512, scale=0.5), max_batch=16)
    x = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, size=(4, 3, 256, 256)).astype(np.float32)).to(DEV)
    lm = torch.from_numpy(np.concatenate([cases.landmarks(), cases.landmarks()])).to(DEV)
    with torch.no_grad():
        avg = ie.get_average_image(net)
        t_inv, (y_hat, latents) = timed(lambda: ie.get_inversions_on_batch(x, net, avg, opts, landmarks_transform=lm), a.reps)
        y_hat = torch.stack(y_hat).float()

        def sweep():
            return [editor.edit_tensors(latents, d, factor_range=(-5, 5), user_transforms=lm, apply_user_transformations=True)[0]
                    for d in opts.edit_directions]
        t_render, edits = timed(sweep, a.reps)
        res['inversion_ms'] = t_inv * 1e3
        res['render_ms'] = t_render * 1e3
        for resize in (True, False):
            s = 256 if resize else 1024

            def finish():
                out = []
                for imgs in edits:
                    strip = torch.empty([4, s, 12 * s, 3], dtype=torch.uint8, device=DEV)
                    to_uint8(x, (s, s), out=strip[:, :, :s])
                    to_uint8(y_hat, (s, s), out=strip[:, :, s:2 * s])
                    for k in range(10):
                        to_uint8(imgs[k], (s, s), out=strip[:, :, (2 + k) * s:(3 + k) * s])
                    out.append(strip.cpu())
                return out
            t_fin, _ = timed(finish, a.reps)
            xc, yc, ec = x.cpu(), y_hat.cpu(), [e.cpu() for e in edits]

            def cpu_finish():                                   # inference_editing.py:73-85 of the reference, per image
                for imgs in ec:
                    for i in range(4):
                        tiles = [tensor2im(xc[i]), tensor2im(yc[i])] + [tensor2im(imgs[k, i]) for k in range(10)]
                        np.concatenate([np.array(t.resize((s, s))) for t in tiles], axis=1)
            t = time.perf_counter()
            cpu_finish()
            t_cpu = time.perf_counter() - t
            key = 'resize' if resize else 'noresize'
            res[f'finish_device_ms_{key}'] = t_fin * 1e3
            res[f'finish_cpu_ms_{key}'] = t_cpu * 1e3
        # the kernel alone, B = 120
        big = torch.cat([e.reshape(40, 3, 1024, 1024) for e in edits])
        for size in ((256, 256), (1024, 1024)):
            out = torch.empty([120, size[1], size[0], 3], dtype=torch.uint8, device=DEV)
            to_uint8(big, size, out=out)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = 20
            e0.record()
            for _ in range(n):
                to_uint8(big, size, out=out)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / n
            res[f'kernel_b120_{size[0]}_us'] = ms * 1e3
            res[f'kernel_b120_{size[0]}_GBps'] = big.numel() * 4 / (ms * 1e-3) / 1e9
        # one pose animation: 9 factors -> 8 segments x 25 frames
        net.decoder.synthesis.input.transform = lm[0]              # one image: one [3,3] transform (the sweeps left [4,3,3])
        _, pose_lat = editor.edit_tensors(latents[:1], 'pose', factor_range=(-4, 5))
        t_anim, frames = timed(lambda: prepare_animation(pose_lat, net.decoder), 1)
        res['animation_frames'] = len(frames)
        res['animation_batched_s'] = t_anim
        if not a.skip_reference_animation:
            def ref_anim():                                     # edit_synthetic.py:112-120 of the reference: batch-1 calls
                out = []
                for i in range(1, len(pose_lat)):
                    for alpha in np.linspace(0, 1, 25).tolist():
                        out.append(np.array(tensor2im(get_result_from_vecs(net.decoder, pose_lat[i - 1], pose_lat[i], alpha)[0])))
                return out
            t = time.perf_counter()
            ref_anim()
            res['animation_reference_loop_s'] = time.perf_counter() - t
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
