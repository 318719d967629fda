"""Golden fixture of the StyleCLIP delta_i_c preprocessing, produced by running the REFERENCE's own
editing/styleclip_global_directions/preprocess/create_delta_i_c.py on the CPU with the reference's own Generator (seeded Ttiny /
Rtiny weights, tests/delta_i_c_cases.py):

  <cfg>/layers, S/<layer>, mean/<layer>, std/<layer>   the inputs: StyleSpace latents of NUM_SAMPLES seeded z and the statistics
  <cfg>/clip_features     what the reference's `main` wrote to clip_features.npy  [channels, NUM_SAMPLES, 2, 16]
  <cfg>/delta_i_c         what it wrote to delta_i_c.npy                            [channels, 16]
  <cfg>/image_absmax      the largest |pixel| the generator rendered during the sweep
  <cfg>/pre_sub, pre_row, pre_col   the reference's `generate_images` of the unperturbed latents: every 7th pixel, the last row
                          and the last column of [NUM_SAMPLES,3,224,224] (the full arrays are too large to commit)

Run in the build container only:
    python tests/golden/make_golden_delta_i_c.py   ->  tests/golden/delta_i_c.npz

What is not the reference here, all of it visible below (the arrangement of make_golden_interfacegan.py): `.cuda()` is the
identity (make_golden_callers, imported first).  The file imports clip / pyrallis / torchvision / tqdm / configs, so
`generate_images`, `get_clip_features`, `get_delta_i_c` and `main` are taken from the file's own text at run time (ast source
segment, executed as is, never written); the sweep is run by the reference's `main` body, not by a restated loop.  `main` gets
stand-ins for what does not exist offline: `clip.load` returns the stand-in encoder of the tests, `SG3Generator` returns the
seeded generator (behind a proxy that records the largest rendered |pixel|), `Normalize` is torchvision's arithmetic written
out ((x - mean) / std per channel), `tqdm` is the identity; the `S` and `s_stats` pickles it reads are written to a temporary
directory in s_statistics.py's formats, the statistics widened to float64 (tests/delta_i_c_cases.py says why).  Nothing from the
reference is stored: the fixture holds seeded inputs and the reference's OUTPUTS only."""
import os
import pickle
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_callers as mgc  # noqa: E402  (puts the reference first on sys.path, neutralises .cuda(), no grad)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import delta_i_c_cases as cases  # noqa: E402

REF_FILE = 'editing/styleclip_global_directions/preprocess/create_delta_i_c.py'


class Normalize:
    """torchvision.transforms.Normalize on a float [n,3,h,w] batch: (x - mean[c]) / std[c]."""

    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, x):
        m = torch.as_tensor(self.mean, dtype=x.dtype).view(-1, 1, 1)
        s = torch.as_tensor(self.std, dtype=x.dtype).view(-1, 1, 1)
        return x.clone().sub_(m).div_(s)


class Recording:
    """The generator as `main` uses it (`.synthesis(None, all_s=..., noise_mode=...)`), keeping the largest |pixel| rendered."""

    def __init__(self, G):
        self.G, self.absmax = G, 0.0

    def synthesis(self, *args, **kwargs):
        img = self.G.synthesis(*args, **kwargs)
        self.absmax = max(self.absmax, float(img.abs().max()))
        return img


def gen(out):
    generate_images = mgc.reference_function(REF_FILE, 'generate_images', torch=torch, F=F, Normalize=Normalize)
    get_clip_features = mgc.reference_function(REF_FILE, 'get_clip_features', torch=torch)
    get_delta_i_c = mgc.reference_function(REF_FILE, 'get_delta_i_c', np=np)
    for cfg in cases.CONFIGS:
        G = mgc.ref_generator(cfg)
        latents, s_mean, s_std = cases.stats_latents(G)
        rec = Recording(G)
        clip = types.SimpleNamespace(load=lambda name, device=None: (cases.StandInEncoder(), None))
        main = mgc.reference_function(REF_FILE, 'main', torch=torch, np=np, pickle=pickle, clip=clip, tqdm=lambda it: it,
                                      SG3Generator=lambda *a, **k: types.SimpleNamespace(decoder=rec), Options=object,
                                      generate_images=generate_images, get_clip_features=get_clip_features, get_delta_i_c=get_delta_i_c)
        with tempfile.TemporaryDirectory() as tmp:
            tmp = Path(tmp)
            with open(tmp / 'S', 'wb') as f:
                pickle.dump(latents, f)
            with open(tmp / 's_stats', 'wb') as f:
                pickle.dump([{'theta': 0.0, 'x': 0.0, 'y': 0.0}, s_mean, s_std], f)
            args = types.SimpleNamespace(checkpoint_path=None, stylegan_size=64, is_landscape=False, latents_s_path=tmp / 'S',
                                         latents_statistics_path=tmp / 's_stats', manipulation_strength=cases.STRENGTH,
                                         results_path=tmp / 'out', num_samples=cases.NUM_SAMPLES)
            main(args)
            out[f'{cfg}/clip_features'] = np.load(tmp / 'out' / 'clip_features.npy')
            out[f'{cfg}/delta_i_c'] = np.load(tmp / 'out' / 'delta_i_c.npy')
        out[f'{cfg}/image_absmax'] = np.float64(rec.absmax)
        out[f'{cfg}/layers'] = np.array(list(latents.keys()))
        for k in latents:
            out[f'{cfg}/S/{k}'], out[f'{cfg}/mean/{k}'], out[f'{cfg}/std/{k}'] = latents[k], s_mean[k], s_std[k]
        pre = generate_images(G, {k: torch.from_numpy(v) for k, v in latents.items()}, batch_size=1).numpy()
        out[f'{cfg}/pre_sub'], out[f'{cfg}/pre_row'], out[f'{cfg}/pre_col'] = cases.subgrid(pre)
        print(cfg, out[f'{cfg}/clip_features'].shape, out[f'{cfg}/clip_features'].dtype, 'absmax', rec.absmax,
              'non-finite delta_i_c rows', int((~np.isfinite(out[f'{cfg}/delta_i_c']).all(axis=-1)).sum()))


def main():
    out = {}
    gen(out)
    path = os.path.join(HERE, 'delta_i_c.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
