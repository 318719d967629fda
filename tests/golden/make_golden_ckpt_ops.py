"""Generate tests/golden/ckpt_ops.npz by running the REFERENCE's `conv2d_resample`, `fma` and `grid_sample_gradfix` on
the CPU, in the style of make_golden.py.

Run in the build container only (the reference is mounted read-only at /root/reference):

    python tests/golden/make_golden_ckpt_ops.py

Nothing from the reference is copied: the fixture holds reference OUTPUTS, the inputs are regenerated from seeds
(tests/ckpt_cases.py).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, '/root/reference')

import torch  # noqa: E402

from ckpt_cases import (CONV2D_RESAMPLE_CASES, RESAMPLE_FILTER, conv2d_resample_inputs, fma_inputs,  # noqa: E402
                        grid_sample_inputs)

from torch_utils.ops import conv2d_resample, fma, grid_sample_gradfix, upfirdn2d  # noqa: E402

torch.set_grad_enabled(False)


def main():
    out = {}
    f = upfirdn2d.setup_filter(RESAMPLE_FILTER)
    for name, c in CONV2D_RESAMPLE_CASES.items():
        x, w = (torch.from_numpy(a) for a in conv2d_resample_inputs(c))
        y = conv2d_resample.conv2d_resample(x, w, f=f, up=c['up'], down=c['down'], padding=c['padding'], groups=c['groups'],
                                            flip_weight=c['flip_weight'])
        out['conv2d_resample/' + name] = y.numpy()
    a, b, c = (torch.from_numpy(v) for v in fma_inputs())
    out['fma'] = fma.fma(a, b, c).numpy()
    image, grid = (torch.from_numpy(v) for v in grid_sample_inputs())
    out['grid_sample'] = grid_sample_gradfix.grid_sample(image, grid).numpy()
    np.savez_compressed(os.path.join(HERE, 'ckpt_ops.npz'), **out)
    print('ckpt_ops.npz', len(out), {k: v.shape for k, v in list(out.items())[:3]})


if __name__ == '__main__':
    main()
