"""delta_i_c for StyleCLIP's global directions (reference editing/styleclip_global_directions/preprocess/create_delta_i_c.py:17-113):
every StyleSpace channel is set to mean - strength * std and to mean + strength * std for `num_samples` latents, the rendered
images are prepared for CLIP and encoded, and the per-channel direction in CLIP's space is the normalised mean of the normalised
feature differences.  `main` writes `clip_features.npy` [channels, num_samples, 2, D] and `delta_i_c.npy` [channels, D], the
files `edit.load_direction_calculator` reads.

The reference renders the 2 * num_samples images of a channel with batch-1 synthesis calls and prepares each with five torch
ops.  Here the items of consecutive channels are assembled into StyleSpace batches of `max_batch`, rendered by one synthesis
forward each and prepared by one launch of `torch_utils.ops.clip_preprocess`; under torch.distributed the channels are sharded
over the ranks and the features all-gathered in channel order.

What a swept item looks like -- the reference's loop (:99-107) writes the perturbed value into `latents_s` in place and never
restores it.  While channel c of a layer is swept, every earlier channel of that layer and every channel of all earlier layers
sits at mean + strength * std, for all samples.  Files made by the reference were made this way.
  restore=False (default)  reproduces that: the item of channel c carries all channels before c at + strength.  This is a closed
                           form of the channel index, so a packed batch and a rank's first channel need no sequential state.
  restore=True             perturbs each channel alone on the original latents: the procedure of the StyleCLIP paper.
The caller's `latents_s` is never written to in either mode.

The CLIP model is external to this package, like the text encoder of `global_direction.py`: `image_encoder` is a callable
[n,3,224,224] -> [n,D] (CLIP's `encode_image`).  The package's own CLIP (models/clip, native transformer kernels on the GPU) is
used when `Options.clip_checkpoint_path` names its state-dict file and no `image_encoder` is passed.  `main` takes an `Options`
(no pyrallis CLI) and, as this package has no configs/paths_config.py, the options carry the generator path."""
import pickle
import warnings
from dataclasses import dataclass
from pathlib import Path
from typing import Optional

import numpy as np
import torch

from sg3_runtime.sharded import all_gather_ragged, shard_range
from torch_utils.ops.clip_preprocess import clip_preprocess


@dataclass
class Options:
    # path to the StyleGAN3 generator (.pkl or state dict)
    checkpoint_path: Optional[Path] = None
    # resolution of the images the generator renders
    stylegan_size: int = 1024
    # landscape model: the config-T sizes instead of config-R when the checkpoint is a state dict
    is_landscape: bool = False
    # S latent codes written by s_statistics.py
    latents_s_path: Path = Path("stats/S")
    # StyleSpace statistics written by s_statistics.py
    latents_statistics_path: Path = Path("stats/s_stats")
    # perturbation in standard deviations: 5 for FFHQ, 10 for other domains
    manipulation_strength: int = 5
    # directory the result files go to
    results_path: Path = Path("delta_i_c")
    # latents per channel; the reference's authors used 300
    num_samples: int = 1
    # CLIP state-dict file for the package's own encoder (models.clip.load); used when no image_encoder is passed
    clip_checkpoint_path: Optional[Path] = None


def generate_images(stylegan_model, latents_s, batch_size=1, **synthesis_kwargs):
    """Render a StyleSpace batch `batch_size` items per synthesis forward and prepare the images for CLIP: [items,3,224,224].
    Extra keyword arguments (e.g. force_fp32=True) go to Generator.synthesis."""
    all_images = []
    for i in range(0, latents_s['input'].shape[0], batch_size):
        curr_latents_s = {l: latents_s[l][i:i + batch_size] for l in latents_s}
        with torch.no_grad():
            curr_images = stylegan_model.synthesis(None, all_s=curr_latents_s, noise_mode='const', **synthesis_kwargs)
            all_images.append(clip_preprocess(curr_images))
    return torch.cat(all_images)


def get_clip_features(image_encoder, images):
    """images [num_samples,2,3,h,w] -> features [1,num_samples,2,D] of one channel."""
    images_reshaped = images.view(-1, 3, images.shape[-2], images.shape[-1])
    with torch.no_grad():
        clip_features = image_encoder(images_reshaped)
    return clip_features.view(images.shape[0], 2, -1).unsqueeze(0)


def get_delta_i_c(clip_features):
    """clip_features [channels,num_samples,2,D] (numpy) -> unit rows [channels,D].  A channel that changes nothing for some sample
    has a zero difference there, and its row is NaN, as in the reference; one warning counts such rows."""
    with np.errstate(divide='ignore', invalid='ignore'):
        features_norm = np.linalg.norm(clip_features, axis=-1)
        normalized_features = clip_features / features_norm[:, :, :, None]
        delta_i_c = normalized_features[:, :, 1, :] - normalized_features[:, :, 0, :]
        normalized_delta_i_c = delta_i_c / np.linalg.norm(delta_i_c, axis=-1)[:, :, None]
        normalized_delta_i_c = normalized_delta_i_c.mean(axis=1)
        normalized_delta_i_c = normalized_delta_i_c / np.linalg.norm(normalized_delta_i_c, axis=-1)[:, None]
    bad = int((~np.isfinite(normalized_delta_i_c).all(axis=-1)).sum())
    if bad:
        warnings.warn(f'get_delta_i_c: {bad} of {normalized_delta_i_c.shape[0]} rows are not finite (channels that change nothing in CLIP space)')
    return normalized_delta_i_c


def _endpoints(latents_s, s_mean, s_std, strength):
    """Per layer the two values a swept channel takes, [2, C] float32: the reference's `mean + direction * std` in the statistics'
    own dtype, rounded to float32 on assignment."""
    out = {}
    for layer, v in latents_s.items():
        m, s = np.asarray(s_mean[layer]), np.asarray(s_std[layer])
        both = np.stack([m + (-strength) * s, m + strength * s])
        out[layer] = torch.from_numpy(np.ascontiguousarray(both)).to(device=v.device, dtype=v.dtype)
    return out


def sweep_items(latents_s, ends, i0, i1, restore=False):
    """The StyleSpace batch of flat sweep items [i0, i1), item = (channel * num_samples + sample) * 2 + direction, channels
    numbered through the layers in `latents_s` key order."""
    n = int(latents_s['input'].shape[0])
    device = latents_s['input'].device
    items = torch.arange(i0, i1, device=device)
    channel, sample, direction = items // (2 * n), (items // 2) % n, items % 2
    out, offset = {}, 0
    for layer, v in latents_s.items():
        local = (channel - offset).unsqueeze(1)                           # the swept channel in this layer's numbering
        cidx = torch.arange(v.shape[1], device=device).unsqueeze(0)
        rows = v[sample]
        if not restore:
            rows = torch.where(cidx < local, ends[layer][1].unsqueeze(0), rows)
        out[layer] = torch.where(cidx == local, ends[layer][direction], rows)
        offset += int(v.shape[1])
    return out


def compute_clip_features(G, latents_s, s_mean, s_std, image_encoder, manipulation_strength=5, max_batch=32, restore=False,
                          shard=False, channel_range=None, **synthesis_kwargs):
    """Encoder features of the whole sweep: [channels, num_samples, 2, D] in the dtype the encoder returns, channels in
    `latents_s` key order ('input' first), which is the order `features_channels_to_s` splits by.

    latents_s: {layer: [num_samples, C_layer]} tensors on G's device (not modified); s_mean, s_std: {layer: [C_layer]}.
    image_encoder: callable [n,3,224,224] -> [n,D].  It is called on up to `max_batch` images at a time, which may belong to
    several channels, so it must treat the samples of a batch independently (CLIP's encoder in eval mode does).
    restore: see the module header.  shard=True under an initialised torch.distributed splits the channels over the ranks;
    every rank returns the full result.  channel_range=(first, end) sweeps only those flat channel numbers (a slice of the full
    result, e.g. to continue an interrupted sweep): with restore=False the channels before `first` sit at + strength."""
    n = int(latents_s['input'].shape[0])
    first, end = (0, sum(int(v.shape[1]) for v in latents_s.values())) if channel_range is None else (int(channel_range[0]), int(channel_range[1]))
    channels = end - first
    start, stop = first, end
    distributed = shard and torch.distributed.is_available() and torch.distributed.is_initialized()
    if distributed:
        start, stop = (first + v for v in shard_range(channels, torch.distributed.get_rank(), torch.distributed.get_world_size()))
    ends = _endpoints(latents_s, s_mean, s_std, manipulation_strength)
    feats = []
    for i0 in range(start * 2 * n, stop * 2 * n, max_batch):
        i1 = min(i0 + max_batch, stop * 2 * n)
        images = generate_images(G, sweep_items(latents_s, ends, i0, i1, restore=restore), batch_size=max_batch, **synthesis_kwargs)
        with torch.no_grad():
            feats.append(image_encoder(images))
    if not feats:                                                         # a rank with no channel still needs D and the dtype
        with torch.no_grad():
            feats.append(image_encoder(torch.zeros([1, 3, 224, 224], device=latents_s['input'].device))[:0])
    local = torch.cat(feats)
    local = local.view(stop - start, n, 2, local.shape[-1])
    return all_gather_ragged(local, channels) if distributed else local


def main(opts: Options, image_encoder=None, generator=None, max_batch=32, restore=False, shard=False, **synthesis_kwargs):
    """Writes results_path / clip_features.npy and delta_i_c.npy.  `image_encoder`: see compute_clip_features; when None, the
    package's CLIP is loaded from `opts.clip_checkpoint_path` if that is set, else CLIP's ViT-B/32 through the `clip` package.
    `generator` replaces loading `opts.checkpoint_path`."""
    results_path = Path(opts.results_path)
    results_path.mkdir(exist_ok=True, parents=True)
    device = torch.device('cuda' if torch.cuda.is_available() else 'cpu') if generator is None else next(generator.parameters()).device
    if image_encoder is None and getattr(opts, 'clip_checkpoint_path', None) is not None:
        from models.clip import load as load_clip
        image_encoder = load_clip(opts.clip_checkpoint_path, device).encode_image
    if image_encoder is None:
        try:
            import clip
        except ImportError as err:
            raise RuntimeError('create_delta_i_c.main: the `clip` package is not installed and no `image_encoder` was passed '
                               '(a callable [n,3,224,224] -> [n,D]; the CLIP model is external to this package)') from err
        clip_model, _ = clip.load("ViT-B/32", device=str(device))
        image_encoder = clip_model.encode_image
    if generator is None:
        from models.stylegan3.model import SG3Generator
        generator = SG3Generator(opts.checkpoint_path, res=opts.stylegan_size, config="landscape" if opts.is_landscape else None,
                                 device=str(device)).decoder.to(device)
    with open(str(opts.latents_s_path), "rb") as f:
        latents_s = pickle.load(f)
    latents_s = {l: torch.from_numpy(np.asarray(latents_s[l][:opts.num_samples])).float().to(device) for l in latents_s}
    with open(str(opts.latents_statistics_path), "rb") as f:
        _, mean, std = pickle.load(f)
    all_clip_features = compute_clip_features(generator, latents_s, mean, std, image_encoder, manipulation_strength=opts.manipulation_strength,
                                              max_batch=max_batch, restore=restore, shard=shard, **synthesis_kwargs)
    all_clip_features = all_clip_features.detach().cpu().numpy()
    delta_i_c = get_delta_i_c(all_clip_features)
    if not shard or not torch.distributed.is_initialized() or torch.distributed.get_rank() == 0:
        np.save(str(results_path / "clip_features.npy"), all_clip_features)
        np.save(str(results_path / "delta_i_c.npy"), delta_i_c)
    return all_clip_features, delta_i_c
