"""2-D convolution between an optional FIR upsampling and an optional FIR downsampling
(operator API of reference torch_utils/ops/conv2d_resample.py: `conv2d_resample` :47).

The generator graph of this package never calls it.  It exists because the module source embedded in upstream training
snapshots (the StyleGAN2-style discriminator next to `G_ema`) imports it by name while the snapshot is unpickled.

The op is a pipeline of three stages, and it is evaluated as exactly that:

    1. up > 1:    `upfirdn2d.upsample2d` -- zero-insert by `up`, filter with `f`, gain up^2, output centred on the input
       up == 1:   nothing
    2. convolve with `w` (`flip_weight=True`: what conv2d computes, a correlation; False: taps reversed, a true convolution)
    3. down > 1:  filter with `f` and keep every `down`-th sample
       down == 1: nothing

Zeros are put around the image ONCE, in front of stage 2 at the latest, never between the stages: the caller's `padding`
(counted in samples of the upsampled image) plus, when there is a stage 3, what keeps its filter centred -- the filter reaches
`taps - down` samples beyond one output step, and the odd sample goes in front.  Stages 1 and 3 are this package's `upfirdn2d`
(the HIP kernel and its autograd on GPU tensors), stage 2 is `conv2d_gradfix.conv2d`.
"""
import torch

from . import conv2d_gradfix
from . import upfirdn2d
from ._resample_args import fir_extent, four_sided
from .. import misc


def _margins(padding, f, down):
    """(left, right, top, bottom) zeros around the upsampled image: the caller's plus the centring of the decimation filter."""
    sides = list(four_sided(padding))
    if down > 1:
        for axis, taps in enumerate(fir_extent(f)):
            reach = taps - down
            sides[2 * axis] += (reach + 1) // 2
            sides[2 * axis + 1] += reach // 2
    return sides


def _is_conv_padding(m):
    return m[0] == m[1] >= 0 and m[2] == m[3] >= 0


@misc.profiled_function
def conv2d_resample(x, w, f=None, up=1, down=1, padding=0, groups=1, flip_weight=True, flip_filter=False):
    """x [N, C, H, W], w [O, C / groups, kh, kw], f from `upfirdn2d.setup_filter` (None: no filtering)  ->  [N, O, H', W']."""
    for name, value in (('up', up), ('down', down), ('groups', groups)):
        if not isinstance(value, int) or value < 1:
            raise ValueError(f'conv2d_resample: {name} must be a positive int, got {value!r}')
    if x.ndim != 4 or w.ndim != 4 or x.dtype != w.dtype:
        raise ValueError(f'conv2d_resample: expected 4-D x and w of one dtype, got {tuple(x.shape)} {x.dtype} and {tuple(w.shape)} {w.dtype}')
    if f is not None and f.dtype != torch.float32:
        raise ValueError('conv2d_resample: the resampling filter must be float32 (see upfirdn2d.setup_filter)')
    kernel = w if flip_weight else w.flip([2, 3])
    m = _margins(padding, f, down)

    if up > 1:
        x = upfirdn2d.upsample2d(x, f, up=up, padding=m, flip_filter=flip_filter)
        m = [0, 0, 0, 0]
    if _is_conv_padding(m):
        x = conv2d_gradfix.conv2d(x, kernel, padding=[m[2], m[0]], groups=groups)
    else:       # uneven or negative margins: pad / crop as a pass of its own
        x = conv2d_gradfix.conv2d(upfirdn2d.upfirdn2d(x, None, padding=m), kernel, groups=groups)
    if down > 1:
        x = upfirdn2d.upfirdn2d(x, f, down=down, flip_filter=flip_filter)
    return x
