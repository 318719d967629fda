"""InterFaceGAN latent editing (API of reference editing/interfacegan/face_editor.py:11-62).

The reference renders one synthesis call per editing factor (batch N) and finishes every image on the CPU (`tensor2im`).  Here
the F factors x N latents of an edit form ONE sweep: all F*N items are rendered `max_batch` at a time, factor-major, each with
its own user transform, optionally sharded over the ranks of torch.distributed (as the StyleCLIP sweep,
editing/styleclip_global_directions/edit.py `render_sweep`), and the images are finished on the device by `to_uint8`
(csrc/sg3_image_finish.hip).  `edit` keeps the reference's contract: nesting of the returned images / latents, factors
`range(*factor_range)`, random transforms drawn from numpy's global stream in the reference's order, and the value the
generator's `synthesis.input.transform` holds after the call.

Directions: this package ships no configs/paths_config.py.  `directions` maps a name to a `.npy` path or an array (what the
reference's `interfacegan_*_edit_paths` hold); without it configs.paths_config is used when importable."""
from pathlib import Path

import numpy as np
import torch

from models.stylegan3.model import GeneratorType
from sg3_runtime.sharded import all_gather_ragged, shard_range
from utils.common import generate_random_transform

DIRECTION_NAMES = ('age', 'smile', 'pose', 'Male')


def _load_direction(value, device):
    arr = np.load(value) if isinstance(value, (str, Path)) else value
    if isinstance(arr, torch.Tensor):
        return arr.to(device)
    return torch.from_numpy(np.asarray(arr)).to(device)


def render_items(generator, ws, transforms=None, max_batch=16, shard=False, **synthesis_kwargs):
    """Render ws [items, num_ws, w_dim] `max_batch` at a time; transforms: None (the generator's own transform, whatever it holds),
    a [3,3] tensor for every item or [items,3,3] per item.  The generator's transform is restored afterwards.  Under
    torch.distributed with `shard`, each rank renders its `shard_range` and the images are all-gathered in item order.
    Returns [items, C, R, R] on every rank."""
    synthesis = generator.synthesis
    n = int(ws.shape[0])
    start, stop = 0, n
    distributed = shard and torch.distributed.is_available() and torch.distributed.is_initialized()
    if distributed:
        start, stop = shard_range(n, torch.distributed.get_rank(), torch.distributed.get_world_size())
    has_input = hasattr(synthesis, 'input')
    saved = synthesis.input.transform if has_input else None
    if transforms is None and has_input and saved.ndim == 3 and saved.shape[0] != 1:
        if n % int(saved.shape[0]) != 0:
            raise RuntimeError(f'render_items: the generator holds {int(saved.shape[0])} transforms for {n} items')
        transforms = saved.repeat(n // int(saved.shape[0]), 1, 1)
    outs = []
    try:
        with torch.no_grad():
            for b0 in range(start, stop, max_batch):
                b1 = min(b0 + max_batch, stop)
                if transforms is not None:
                    synthesis.input.transform = transforms if transforms.ndim == 2 else transforms[b0:b1].contiguous()
                outs.append(synthesis(ws[b0:b1], noise_mode='const', **synthesis_kwargs))
    finally:
        if has_input:
            synthesis.input.transform = saved
    res = int(generator.img_resolution)
    local = torch.cat(outs) if outs else torch.zeros([0, int(generator.img_channels), res, res], device=ws.device)
    return all_gather_ragged(local, n) if distributed else local


class FaceEditor:

    def __init__(self, stylegan_generator, generator_type=GeneratorType.ALIGNED, directions=None, max_batch=16, shard=False):
        self.generator = stylegan_generator
        self.max_batch, self.shard = int(max_batch), bool(shard)
        if directions is None:
            try:
                from configs import paths_config
            except ImportError:
                raise ValueError('FaceEditor: no `directions` given and configs.paths_config cannot be imported; pass directions='
                                 f'{{name: .npy path or array}} with the keys {list(DIRECTION_NAMES)}') from None
            paths = (paths_config.interfacegan_aligned_edit_paths if generator_type == GeneratorType.ALIGNED
                     else paths_config.interfacegan_unaligned_edit_paths)
            directions = {name: paths[name] for name in DIRECTION_NAMES}
        device = next(stylegan_generator.parameters()).device
        self.interfacegan_directions = {name: _load_direction(v, device) for name, v in directions.items()}

    def _edit_transform(self, apply_user_transformations, user_transforms, n_factors):
        """What the reference assigns to synthesis.input.transform (None: it leaves the generator's alone).  One random draw
        when a transform is needed and none is given; none at all for an empty factor range."""
        if not apply_user_transformations or n_factors == 0:
            return None
        if user_transforms is None:
            user_transforms = generate_random_transform(translate=0.3, rotate=25)
        if isinstance(user_transforms, np.ndarray):
            user_transforms = torch.from_numpy(user_transforms)
        device = next(self.generator.parameters()).device
        return user_transforms.to(device).float()

    def edit_tensors(self, latents, direction, factor=1, factor_range=None, user_transforms=None, apply_user_transformations=False,
                     **synthesis_kwargs):
        """Same arguments as `edit`.  Returns (images [F,N,3,R,R] float32 on the generator's device, latents [F,N,num_ws,w_dim]);
        F = len(range(*factor_range)), or 1 for a single `factor`."""
        d = self.interfacegan_directions[direction]
        if factor_range is not None:
            factors = list(range(*factor_range))
        else:
            factors = [factor]
            user_transforms = None                 # the reference's single-factor call draws its own transform (face_editor.py:44)
        n = int(latents.shape[0])
        t = self._edit_transform(apply_user_transformations, user_transforms, len(factors))
        if not factors:
            res = int(self.generator.img_resolution)
            return (torch.zeros([0, n, int(self.generator.img_channels), res, res], device=latents.device),
                    torch.zeros([0, *latents.shape], dtype=latents.dtype, device=latents.device))
        edit_latents = torch.stack([latents + f * d for f in factors])
        per_item = None
        if t is not None:
            if t.ndim == 3 and t.shape[0] != 1:
                if int(t.shape[0]) != n:
                    raise RuntimeError(f'FaceEditor: {int(t.shape[0])} user transforms for {n} latents')
                per_item = t.unsqueeze(0).expand(len(factors), n, 3, 3).reshape(-1, 3, 3)
            else:
                per_item = t.reshape(3, 3)
        items = edit_latents.reshape(len(factors) * n, *edit_latents.shape[2:])
        images = render_items(self.generator, items, per_item, max_batch=self.max_batch, shard=self.shard, **synthesis_kwargs)
        if t is not None:
            self.generator.synthesis.input.transform = t           # what the reference leaves there
        return images.reshape(len(factors), n, *images.shape[1:]), edit_latents

    def edit(self, latents, direction, factor=1, factor_range=None, user_transforms=None, apply_user_transformations=False,
             **synthesis_kwargs):
        """Reference contract: range mode returns ([per factor: N PIL images], [per factor: latents [N,num_ws,w_dim]]); single
        mode (N PIL images, latents)."""
        from PIL import Image
        from torch_utils.ops.image_finish import to_uint8
        images, edit_latents = self.edit_tensors(latents, direction, factor=factor, factor_range=factor_range, user_transforms=user_transforms,
                                                 apply_user_transformations=apply_user_transformations, **synthesis_kwargs)
        f, n = int(images.shape[0]), int(images.shape[1])
        u8 = to_uint8(images.reshape(f * n, *images.shape[2:])).cpu().numpy() if f * n else None
        pil = [[Image.fromarray(u8[i * n + j]) for j in range(n)] for i in range(f)]
        if factor_range is not None:
            return pil, [edit_latents[i] for i in range(f)]
        return pil[0], edit_latents[0]
