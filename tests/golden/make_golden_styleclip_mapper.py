"""Golden fixture of the StyleCLIP latent mapper, produced by running the REFERENCE's own latent_mappers.py on the CPU:

  <case>/delta    mapper(x)                      [6, 16, 512] float32, x = tests/mapper_cases.py inputs()
  <case>/keys     the reference module's state-dict keys and shapes, 'name:[shape]'
  (w_hat)         w + 0.1 * mapper(w): not stored.  The script checks that the reference's w_hat equals, bit for bit, the
                  float32 x + float32(0.1) * delta (one rounded product, one rounded sum), which is how the tests rebuild it.

The cases, seeded weights (non-zero biases) and inputs are tests/mapper_cases.py; the fixture stores outputs only.  Run in the
build container with the reference tree's root as the argument:
    python tests/golden/make_golden_styleclip_mapper.py <reference tree>   ->  tests/golden/styleclip_mapper.npz

What is not the reference here: the reference's `fused_leaky_relu` moves its input with `.cuda()`; there is no GPU in the build
container, so `torch.Tensor.cuda` is patched to the identity while this script runs.  Nothing from the reference is copied."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mapper_cases as cases  # noqa: E402


def main(ref):
    sys.path.insert(0, ref)
    torch.Tensor.cuda = lambda self, *a, **k: self
    from editing.styleclip_mapper import latent_mappers as ref_lm
    x = torch.from_numpy(cases.inputs())
    out = {'x_check': x.numpy()[:, :1, :4]}
    for case in cases.CASES:
        o = cases.opts(case)
        m = ref_lm.SingleMapper(o) if o.mapper_type == 'SingleMapper' else ref_lm.LevelsMapper(o)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in cases.state_dict(o).items()}, strict=True)
        m.eval()
        with torch.no_grad():
            delta = m(x)
            w_hat = x + 0.1 * m(x)
        d = delta.numpy().astype(np.float32)
        assert np.array_equal(w_hat.numpy(), x.numpy() + np.float32(0.1) * d), case
        out[f'{case}/delta'] = d
        out[f'{case}/keys'] = np.array([f'{k}:{list(v.shape)}' for k, v in m.state_dict().items()])
    path = os.path.join(HERE, 'styleclip_mapper.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: make_golden_styleclip_mapper.py <reference tree root>')
    main(sys.argv[1])
