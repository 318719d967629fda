"""StyleCLIP latent mapper inference (reference editing/styleclip_mapper/scripts/inference.py).

`run_on_batch` edits a batch of W+ codes, w_hat = w + 0.1 * mapper(w), and renders them; on the HIP path (eval mode, no
gradients, CUDA float32 [N, 16, 512]) w_hat comes straight from the fused mapper kernel.  `run` walks the latents file in full
batches (the reference's DataLoader uses drop_last=True and checks n_images only between batches) and writes
`inference_results/latent_{i:05d}.pt` per item and `stats.txt`.  Under torch.distributed each rank takes a contiguous
`shard_range` of the batches and writes its files under their global indices; no collective is needed.

The reference also writes every image (or the input/output pair) as a JPEG through torchvision.utils.save_image.  That is
left to the caller: torchvision is not a dependency of this package and its JPEG rounding is not pinned by any test here.  The
rendered batch is what `run_on_batch` returns.
"""
import os
import sys
import time
from argparse import Namespace

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset

sys.path.append('.')
sys.path.append('..')

from editing.styleclip_mapper.datasets.latents_dataset import LatentsDataset  # noqa: E402
from editing.styleclip_mapper.options.test_options import TestOptions  # noqa: E402
from sg3_runtime.sharded import shard_range  # noqa: E402


def _batches_to_run(n_items, batch_size, n_images):
    """Number of leading full batches the reference loop processes (reference :52-56)."""
    full = n_items // batch_size
    if n_images is None:
        n_images = n_items
    if n_images <= 0:
        return 0
    return min(full, -(-n_images // batch_size))


def run(test_opts, net=None):
    """Reference :22-84.  `net` (optional) is a ready StyleCLIPMapper-like module with `.mapper` and `.decoder`; passing it
    skips loading the checkpoint and uses `test_opts` as the options.  Returns the global indices of the items written."""
    out_path_results = os.path.join(test_opts.exp_dir, 'inference_results')
    os.makedirs(out_path_results, exist_ok=True)

    if net is None:
        from editing.styleclip_mapper.styleclip_mapper import StyleCLIPMapper
        ckpt = torch.load(test_opts.checkpoint_path, map_location='cpu', weights_only=False)
        opts = ckpt['opts']
        opts.update(vars(test_opts))
        opts = Namespace(**opts)
        net = StyleCLIPMapper(opts)
        net.eval()
        net.cuda()
    else:
        opts = test_opts
    device = next(net.decoder.parameters()).device

    test_latents = torch.load(opts.latents_test_path, map_location='cpu')
    transforms = np.load(opts.fourier_features_transforms_path, allow_pickle=True) if opts.fourier_features_transforms_path else None
    dataset = LatentsDataset(latents=test_latents.cpu(), opts=opts, transforms=transforms)
    bs = int(opts.test_batch_size)
    n_batches = _batches_to_run(len(dataset), bs, opts.n_images)
    b0, b1 = 0, n_batches
    rank = 0
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        rank = torch.distributed.get_rank()
        b0, b1 = shard_range(n_batches, rank, torch.distributed.get_world_size())
    dataloader = DataLoader(Subset(dataset, range(b0 * bs, b1 * bs)), batch_size=bs, shuffle=False,
                            num_workers=int(opts.test_workers), drop_last=True)

    global_i = b0 * bs
    global_time = []
    written = []
    for input_batch in dataloader:
        with torch.no_grad():
            if opts.fourier_features_transforms_path:
                input_cuda, transform = input_batch
                transform = transform.to(device)
            else:
                input_cuda, transform = input_batch, None
            input_cuda = input_cuda.to(device)
            tic = time.time()
            result_batch = run_on_batch(input_cuda, transform, net, opts.couple_outputs)
            if device.type == 'cuda':
                torch.cuda.synchronize(device)
            global_time.append(time.time() - tic)
        w_hat = result_batch[1].detach().cpu()
        for i in range(bs):
            torch.save(w_hat[i].clone(), os.path.join(out_path_results, f'latent_{global_i:05d}.pt'))
            written.append(global_i)
            global_i += 1

    if rank == 0:
        result_str = 'Runtime {:.4f}+-{:.4f}'.format(np.mean(global_time) if global_time else float('nan'),
                                                     np.std(global_time) if global_time else float('nan'))
        print(result_str)
        with open(os.path.join(opts.exp_dir, 'stats.txt'), 'w') as f:
            f.write(result_str)
    return written


def run_on_batch(inputs, transform, net, couple_outputs=False):
    """(x_hat, w_hat) or (x_hat, w_hat, x) with w_hat = w + 0.1 * net.mapper(w), x_hat = synthesis(w_hat), x = synthesis(w).
    A [B, 3, 3] `transform` is set on the decoder's input layer and left there (reference :87-99)."""
    w = inputs
    with torch.no_grad():
        edit = getattr(net.mapper, 'edit', None)
        w_hat = edit(w, 0.1) if edit is not None else w + 0.1 * net.mapper(w)
        if transform is not None:
            net.decoder.synthesis.input.transform = transform
        x_hat = net.decoder.synthesis(w_hat)
        result_batch = (x_hat, w_hat)
        if couple_outputs:
            x = net.decoder.synthesis(w)
            result_batch = (x_hat, w_hat, x)
    return result_batch


if __name__ == '__main__':
    run(TestOptions().parse())
