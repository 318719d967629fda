"""Golden fixture of the CLIP loss, produced by running the REFERENCE's own models/styleganxl/feature_networks/clip/model.py in
float64 on the CPU with the seeded `small` weights of tests/clip_cases.py (loaded with strict=True) at w_scale 1 and 3, through
the three torch modules of the reference's criteria/clip_loss.py `forward`, written out here because that file imports the `clip`
package, which is not installed:

    image = AvgPool2d(kernel_size=stylegan_size // 32)(Upsample(scale_factor=7)(image));  loss = 1 - model(image, text)[0] / 100

  w<s>/loss<size>   the loss [batch, 3] for the images of tests/clip_loss_cases.py at stylegan_size 64 (batch 2) and 32 (batch 1)
  w<s>/grad<size>   d mean(loss) / d image, [batch, 3, size, size]

The fixture stores results only.  Run in the build container with the reference tree's root as the argument:
    python tests/golden/make_golden_clip_loss.py <reference tree>   ->  tests/golden/clip_loss.npz

As in make_golden_clip.py, the reference's LayerNorm.forward (which casts to float32 whatever the model's dtype) is replaced by
torch.nn.LayerNorm.forward for this float64 run, and the reference file is loaded by path.  Nothing from the reference is copied."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clip_cases as cases  # noqa: E402
import clip_loss_cases as lcases  # noqa: E402


def main(ref):
    spec = importlib.util.spec_from_file_location('ref_clip_model', os.path.join(ref, 'models', 'styleganxl', 'feature_networks', 'clip', 'model.py'))
    ref_model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_model)
    ref_model.LayerNorm.forward = torch.nn.LayerNorm.forward
    text = torch.from_numpy(lcases.tokens())
    out = {}
    for w_scale in lcases.W_SCALES:
        m = ref_model.CLIP(**cases.CONFIGS[lcases.CFG])
        m.load_state_dict({k: torch.from_numpy(v) for k, v in cases.state_dict(lcases.CFG, w_scale=w_scale).items()}, strict=True)
        m = m.eval().double().requires_grad_(False)
        for size, n in lcases.GOLDEN_IMAGES.items():
            upsample, avg_pool = torch.nn.Upsample(scale_factor=7), torch.nn.AvgPool2d(kernel_size=size // 32)
            image = torch.from_numpy(lcases.images(size, n)).double().requires_grad_(True)
            loss = 1 - m(avg_pool(upsample(image)), text)[0] / 100
            loss.mean().backward()
            out[f'w{w_scale}/loss{size}'], out[f'w{w_scale}/grad{size}'] = loss.detach().numpy(), image.grad.numpy()
            print(f'w_scale {w_scale} size {size}: loss {loss.detach().numpy().ravel()}, max|grad| {image.grad.abs().max():.3e}, '
                  f'median|grad| {image.grad.abs().median():.3e}')
    path = os.path.join(HERE, 'clip_loss.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: make_golden_clip_loss.py <reference tree root>')
    main(sys.argv[1])
