"""Golden fixture of the InterFaceGAN editing callers, produced by running the REFERENCE's own code on CPU with the reference's
own Generator (seeded Ttiny / Rtiny weights):

  ig/<cfg>/<case>/images      editing/interfacegan/face_editor.py  FaceEditor.edit  -> its PIL images as uint8 [F,N,R,R,3]
  ig/<cfg>/<case>/transform   synthesis.input.transform after the call
  ig/<cfg>/anim               editing/interfacegan/edit_synthetic.py  prepare_animation / get_result_from_vecs frames [K,R,R,3]

The cases are tests/interfacegan_cases.py.  Run in the build container only:
    python tests/golden/make_golden_interfacegan.py   ->  tests/golden/interfacegan.npz

What is not the reference here, all of it visible below (the same arrangement as make_golden_callers.py, whose import performs
it): `.cuda()` is the identity (no GPU in the build container); `FaceEditor.__init__` loads the pretrained boundary files from
configs.paths_config, which do not exist offline, so the editor is created without it and the synthetic directions are
injected as the tensors `__init__` would have built; edit_synthetic.py imports pyrallis / tqdm / configs, so `prepare_animation`
and `get_result_from_vecs` are taken from the file's own text at run time (ast source segment, executed as is, never written).
Nothing from the reference is stored: the fixture holds the reference's OUTPUTS for seeded inputs only."""
import os
import sys
import typing

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_callers as mgc  # noqa: E402  (puts the reference first on sys.path, neutralises .cuda(), no grad)

import torch  # noqa: E402

import interfacegan_cases as cases  # noqa: E402
from editing.interfacegan.face_editor import FaceEditor  # noqa: E402
from utils.common import tensor2im  # noqa: E402


def u8(images):
    return np.stack([np.array(im) for im in images])


def gen(out):
    for cfg in ('Ttiny', 'Rtiny'):
        G = mgc.ref_generator(cfg)
        editor = FaceEditor.__new__(FaceEditor)
        editor.generator = G
        editor.interfacegan_directions = {k: torch.from_numpy(v) for k, v in cases.directions(G.w_dim).items()}
        lat = torch.from_numpy(cases.latents(G.num_ws, G.w_dim))
        lm = torch.from_numpy(cases.landmarks())
        kept = {}
        for case in cases.CASES:
            if case['seed'] is not None:
                np.random.seed(case['seed'])
            images, latents = editor.edit(lat, **cases.edit_kwargs(case, lm))
            if 'factor_range' in case:
                out[f'ig/{cfg}/{case["key"]}/images'] = np.stack([u8(step) for step in images])
                kept[case['key']] = latents
            else:
                out[f'ig/{cfg}/{case["key"]}/images'] = u8(images)[None]
            out[f'ig/{cfg}/{case["key"]}/transform'] = G.synthesis.input.transform.numpy()
        names = dict(Generator=type(G), List=typing.List, N_TRANSITIONS=25, torch=torch)   # names the functions use
        get_result_from_vecs = mgc.reference_function('editing/interfacegan/edit_synthetic.py', 'get_result_from_vecs', **names)
        prepare_animation = mgc.reference_function('editing/interfacegan/edit_synthetic.py', 'prepare_animation', np=np, tqdm=lambda it: it,
                                                   tensor2im=tensor2im, get_result_from_vecs=get_result_from_vecs, **names)
        anim_latents = torch.stack([step[:1] for step in kept['A']])
        out[f'ig/{cfg}/anim'] = np.stack(prepare_animation(anim_latents, G, n_transitions=cases.N_ANIM))


def main():
    out = {}
    gen(out)
    path = os.path.join(HERE, 'interfacegan.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    main()
