"""Rendered images -> the normalised tensors CLIP's image encoder takes, on the device (libsg3hip: csrc/sg3_clip_preprocess.hip).

The reference prepares every rendered image of the delta_i_c sweep with five torch ops
(editing/styleclip_global_directions/preprocess/create_delta_i_c.py:53-56): bicubic `F.interpolate` to 224 x 224 with
align_corners=True, `(y + 1) / 2`, `clamp(0, 1)` and torchvision's `Normalize` with CLIP's constants.  `composite` below is that
arithmetic written out (torchvision is not a dependency) and is the definition; `clip_preprocess` runs it as one HIP launch for
CUDA float32 input that records no gradient."""
import ctypes

import torch
import torch.nn.functional as F

from .. import _sg3abi as abi

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def composite(x, size=(224, 224), mean=CLIP_MEAN, std=CLIP_STD):
    """The definition: x [B,3,H,W] floating point -> [B,3,h,w] of the same dtype, differentiable."""
    y = F.interpolate(x, size=tuple(int(v) for v in size), mode='bicubic', align_corners=True)
    y = ((y + 1) / 2).clamp(0, 1)
    m = torch.as_tensor(mean, dtype=y.dtype, device=y.device).view(1, 3, 1, 1)
    s = torch.as_tensor(std, dtype=y.dtype, device=y.device).view(1, 3, 1, 1)
    return (y - m) / s


def clip_preprocess(x, size=(224, 224), mean=CLIP_MEAN, std=CLIP_STD, out=None):
    """x [B,3,H,W] floating point (any strides), size (h, w), out: optional float32 [B,3,h,w] to fill (any strides; kernel path
    only).  Returns [B,3,h,w].  CUDA float32 input with no gradient recorded runs the HIP kernel, one launch on the current
    stream; CPU tensors, other dtypes and inputs that record a gradient take `composite`, which is the definition."""
    if not isinstance(x, torch.Tensor) or not x.is_floating_point():
        raise RuntimeError(f'clip_preprocess: x must be a floating-point tensor, got {getattr(x, "dtype", type(x))}')
    if x.ndim != 4 or int(x.shape[1]) != 3:
        raise RuntimeError(f'clip_preprocess: x must be [B,3,H,W], got {list(x.shape)}')
    if len(size) != 2 or int(size[0]) <= 0 or int(size[1]) <= 0:
        raise RuntimeError(f'clip_preprocess: size must be (h, w) with positive entries, got {size}')
    if len(mean) != 3 or len(std) != 3 or any(float(v) == 0 for v in std):
        raise RuntimeError(f'clip_preprocess: mean and std must have 3 entries and std no zero, got {mean}, {std}')
    b, _, hh, ww = (int(v) for v in x.shape)
    h, w = int(size[0]), int(size[1])
    if not (x.is_cuda and x.dtype == torch.float32) or (torch.is_grad_enabled() and x.requires_grad) or b == 0:
        if out is not None:
            raise RuntimeError('clip_preprocess: out is only supported for CUDA float32 input with no gradient recorded')
        return composite(x, (h, w), mean, std)
    if out is None:
        out = torch.empty([b, 3, h, w], dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (b, 3, h, w) or out.device != x.device:
        raise RuntimeError(f'clip_preprocess: out must be float32 {[b, 3, h, w]} on {x.device}, got {out.dtype} {list(out.shape)} on {out.device}')
    p = abi.ClipPreprocessParams()
    p.x, p.y = abi.ptr(x), abi.ptr(out)
    p.xStride, p.yStride = abi.strides4(x), abi.strides4(out)
    p.B, p.C, p.H, p.W, p.h, p.w = b, 3, hh, ww, h, w
    p.mean, p.std = (abi.c_f32 * 3)(*[float(v) for v in mean]), (abi.c_f32 * 3)(*[float(v) for v in std])
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_clip_preprocess(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_clip_preprocess')
    return out
