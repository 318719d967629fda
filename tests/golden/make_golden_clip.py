"""Golden fixture of the CLIP encoders, produced by running the REFERENCE's own models/styleganxl/feature_networks/clip/model.py
on the CPU with the seeded weights of tests/clip_cases.py (loaded with strict=True), for the configurations GOLDEN_CONFIGS:

  <cfg>/image64, <cfg>/text64     the reference's float64 encode_image / encode_text, [GOLDEN_BATCH, embed_dim]
  <cfg>/image_err, <cfg>/text_err [2]: max |float32 model - float64 model| and max |convert_weights (float16) model - float64 model|
                                  of the reference itself, on the same inputs
  <cfg>/keys                      the reference module's state-dict keys and shapes, 'name:[shape]', in its order

The fixture stores outputs and names only.  Run in the build container with the reference tree's root as the argument:
    python tests/golden/make_golden_clip.py <reference tree>   ->  tests/golden/clip.npz

What is not the reference here: its LayerNorm.forward casts the input to float32 whatever the model's dtype, which would cap the
float64 run at float32 accuracy; for the float64 run only, that method is replaced by torch.nn.LayerNorm.forward.  The float32 and
float16 runs use the reference unmodified.  The reference file is loaded by path (its package name `models` is also this
package's).  Nothing from the reference is copied."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clip_cases as cases  # noqa: E402


def main(ref):
    spec = importlib.util.spec_from_file_location('ref_clip_model', os.path.join(ref, 'models', 'styleganxl', 'feature_networks', 'clip', 'model.py'))
    ref_model = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_model)
    ref_ln_forward = ref_model.LayerNorm.forward
    out = {}
    for cfg in cases.GOLDEN_CONFIGS:
        sd = {k: torch.from_numpy(v) for k, v in cases.state_dict(cfg).items()}
        image, toks = torch.from_numpy(cases.images(cfg, cases.GOLDEN_BATCH)), torch.from_numpy(cases.tokens(cfg, cases.GOLDEN_BATCH))

        def run(kind):
            m = ref_model.CLIP(**cases.CONFIGS[cfg])
            m.load_state_dict(sd, strict=True)
            m.eval()
            if kind == 'f64':
                m = m.double()
            elif kind == 'f16':
                ref_model.convert_weights(m)
            with torch.no_grad():
                return m, m.encode_image(image).double().numpy(), m.encode_text(toks).double().numpy()

        ref_model.LayerNorm.forward = torch.nn.LayerNorm.forward
        try:
            m, img64, txt64 = run('f64')
        finally:
            ref_model.LayerNorm.forward = ref_ln_forward
        _, img32, txt32 = run('f32')
        _, img16, txt16 = run('f16')
        out[f'{cfg}/image64'], out[f'{cfg}/text64'] = img64, txt64
        out[f'{cfg}/image_err'] = np.array([np.abs(img32 - img64).max(), np.abs(img16 - img64).max()])
        out[f'{cfg}/text_err'] = np.array([np.abs(txt32 - txt64).max(), np.abs(txt16 - txt64).max()])
        out[f'{cfg}/keys'] = np.array([f'{k}:{list(v.shape)}' for k, v in m.state_dict().items()])
        print(cfg, 'max|image|', np.abs(img64).max(), 'image err (f32, f16)', out[f'{cfg}/image_err'], 'max|text|', np.abs(txt64).max(),
              'text err (f32, f16)', out[f'{cfg}/text_err'])
    path = os.path.join(HERE, 'clip.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: make_golden_clip.py <reference tree root>')
    main(sys.argv[1])
