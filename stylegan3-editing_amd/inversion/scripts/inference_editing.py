"""InterFaceGAN editing of real images after ReStyle inversion (reference inversion/scripts/inference_editing.py:24-138).

As inference_iterative.py in this package, the harness is a set of functions over tensors: there is no pyrallis CLI and no
torchvision dataset.  `get_inversions_on_batch` and `edit_batch` keep the reference's signatures and return values (PIL
images, finished on the device).  `edit_batch_strips` builds the saved result strips [input | inversion | F edits] on the
device: every edit direction is one batched sweep (FaceEditor.edit_tensors) and every tile is written by `to_uint8` straight
into its columns of the strip.  `run_editing` writes what the reference writes:

  <output_path>/editing_results/<direction>/<name>   one strip per image and direction
  <output_path>/stats.txt                            'Runtime {mean:.4f}+-{std:.4f}' over the per-batch edit time
"""
import os
import time

import numpy as np
import torch

from editing.interfacegan.face_editor import FaceEditor
from models.stylegan3.model import GeneratorType
from torch_utils.ops.image_finish import to_uint8
from utils.inference_utils import get_average_image, run_on_batch

DEFAULT_EDIT_DIRECTIONS = ['age', 'smile', 'pose']
DEFAULT_FACTOR_RANGES = ['(-5_5)', '(-5_5)', '(-5_5)']


def parse_factor_ranges(factor_ranges):
    """Tuples pass through; the reference's '(-5_5)' strings are parsed as inversion/options/test_options.py:45-50 does."""
    out = []
    for factor in factor_ranges:
        if isinstance(factor, str):
            start, end = factor.strip("()").split("_")
            out.append((int(start), int(end)))
        else:
            start, end = factor
            out.append((int(start), int(end)))
    return out


def _edit_plan(opts):
    directions = list(getattr(opts, 'edit_directions', None) or DEFAULT_EDIT_DIRECTIONS)
    ranges = parse_factor_ranges(getattr(opts, 'factor_ranges', None) or DEFAULT_FACTOR_RANGES)
    if len(directions) != len(ranges):
        raise ValueError(f'one factor range per edit direction is needed: {directions} and {ranges}')
    return list(zip(directions, ranges))


def get_inversions_on_batch(inputs, net, avg_image, opts, landmarks_transform=None):
    result_batch, result_latents = run_on_batch(inputs=inputs, net=net, opts=opts, avg_image=avg_image, landmarks_transform=landmarks_transform)
    # the final inversion is the one to edit
    y_hat = [result_batch[idx][-1] for idx in range(len(result_batch))]
    latents = [torch.from_numpy(result_latents[idx][-1]).to(inputs.device) for idx in range(len(result_batch))]
    return y_hat, torch.stack(latents)


def edit_batch(inputs, net, avg_image, latent_editor, opts, landmarks_transform=None):
    """{idx: {'inversion': PIL image, direction: [PIL image per factor]}} (reference :103-124).  As in the reference, every edit
    applies a user transform: the landmarks transforms, or a random one per direction when there are none."""
    from PIL import Image
    y_hat, latents = get_inversions_on_batch(inputs=inputs, net=net, avg_image=avg_image, opts=opts, landmarks_transform=landmarks_transform)
    inv = to_uint8(torch.stack(y_hat).float()).cpu().numpy()
    results = {idx: {'inversion': Image.fromarray(inv[idx])} for idx in range(len(inputs))}
    for edit_direction, factor_range in _edit_plan(opts):
        edit_images, _ = latent_editor.edit(latents=latents, direction=edit_direction, factor_range=factor_range,
                                            apply_user_transformations=True, user_transforms=landmarks_transform)
        for idx in range(inputs.shape[0]):
            results[idx][edit_direction] = [step_res[idx] for step_res in edit_images]
    return results


def strip_size(opts, net):
    """Tile size of the result strips: 256 with resize_outputs, else opts.output_size (reference :53)."""
    if getattr(opts, 'resize_outputs', False):
        return 256
    return int(getattr(opts, 'output_size', None) or net.decoder.img_resolution)


def edit_batch_strips(inputs, net, avg_image, latent_editor, opts, landmarks_transform=None, **synthesis_kwargs):
    """{direction: uint8 [N, s, (2+F)*s, 3]} on the device, each row of tiles [input | inversion | F edits] resized to s
    (reference :73-85: tensor2im, PIL resize to (s, s), concatenation along the width).  Draws the same random transforms as
    `edit_batch`."""
    s = strip_size(opts, net)
    y_hat, latents = get_inversions_on_batch(inputs=inputs, net=net, avg_image=avg_image, opts=opts, landmarks_transform=landmarks_transform)
    y_hat = torch.stack(y_hat).float()
    n = int(inputs.shape[0])
    head = torch.empty([n, s, 2 * s, 3], dtype=torch.uint8, device=inputs.device)
    to_uint8(inputs, (s, s), out=head[:, :, :s])
    to_uint8(y_hat, (s, s), out=head[:, :, s:])
    strips = {}
    for edit_direction, factor_range in _edit_plan(opts):
        images, _ = latent_editor.edit_tensors(latents=latents, direction=edit_direction, factor_range=factor_range,
                                               apply_user_transformations=True, user_transforms=landmarks_transform, **synthesis_kwargs)
        f = int(images.shape[0])
        strip = torch.empty([n, s, (2 + f) * s, 3], dtype=torch.uint8, device=inputs.device)
        strip[:, :, :2 * s].copy_(head)
        for k in range(f):
            to_uint8(images[k], (s, s), out=strip[:, :, (2 + k) * s:(3 + k) * s])
        strips[edit_direction] = strip
    return strips


def run_editing(net, opts, images, names, output_path, landmarks_transforms=None, editor=None, batch_size=None, n_images=None):
    """images: [M,3,256,256] tensor (any device); names: M file names; landmarks_transforms: optional [M,3,3].
    Writes the strips and stats.txt (module docstring); returns the runtime string."""
    from PIL import Image
    device = next(net.parameters()).device
    total = int(images.shape[0]) if n_images is None else min(int(n_images), int(images.shape[0]))
    assert len(names) >= total
    bs = int(batch_size or getattr(opts, 'test_batch_size', 2))
    if editor is None:
        editor = FaceEditor(net.decoder, generator_type=GeneratorType.ALIGNED)
    out_path_results = os.path.join(output_path, 'editing_results')
    os.makedirs(out_path_results, exist_ok=True)
    with torch.no_grad():
        avg_image = get_average_image(net)
    global_time = []
    for b0 in range(0, total, bs):
        b1 = min(b0 + bs, total)
        with torch.no_grad():
            x = images[b0:b1].to(device).float()
            lt = None if landmarks_transforms is None else landmarks_transforms[b0:b1].to(device).float()
            tic = time.time()
            strips = edit_batch_strips(x, net, avg_image, editor, opts, landmarks_transform=lt)
            strips = {k: v.cpu().numpy() for k, v in strips.items()}       # the copy to the host ends the batch's device work
            global_time.append(time.time() - tic)
        for edit_name, strip in strips.items():
            edit_save_dir = os.path.join(out_path_results, edit_name)
            os.makedirs(edit_save_dir, exist_ok=True)
            for i in range(b1 - b0):
                Image.fromarray(strip[i]).save(os.path.join(edit_save_dir, os.path.basename(str(names[b0 + i]))))
    result_str = f'Runtime {np.mean(global_time):.4f}+-{np.std(global_time):.4f}'
    print(result_str)
    with open(os.path.join(output_path, 'stats.txt'), 'w') as f:
        f.write(result_str)
    return result_str
