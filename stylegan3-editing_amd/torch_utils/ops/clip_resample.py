"""Nearest upsampling followed by average pooling, fused (libsg3hip: csrc/sg3_clip_resample.hip).

The reference's CLIP loss prepares its image with `AvgPool2d(stylegan_size // 32)(Upsample(scale_factor=7)(image))`
(criteria/clip_loss.py): 224 x 224 for every size that is a multiple of 32, through an intermediate 7 times the image in each
direction.  `composite` below is those two torch modules and is the definition; `nearest_up_avg_pool` runs the pair as one HIP
launch with no intermediate for CUDA float32 tensors, and its adjoint as one launch in gather form (no atomics: deterministic).
CPU tensors, other dtypes and double backward take the composite."""
import ctypes

import torch
import torch.nn.functional as F

from .. import _sg3abi as abi


def out_size(n, up, k):
    """AvgPool2d floors: floor(up * n / k)."""
    return (int(up) * int(n)) // int(k)


def composite(x, up, k):
    """The definition: x [B,C,H,W] floating point -> [B,C,floor(up H / k),floor(up W / k)], differentiable."""
    return F.avg_pool2d(F.interpolate(x, scale_factor=int(up), mode='nearest'), int(k))


def _launch(x, y, up, k, adjoint):
    b, c, h, w = (int(v) for v in x.shape)
    p = abi.ClipResampleParams()
    p.x, p.y = abi.ptr(x), abi.ptr(y)
    p.xStride, p.yStride = abi.strides4(x), abi.strides4(y)
    p.B, p.C, p.H, p.W, p.oh, p.ow, p.up, p.k, p.adjoint = b, c, h, w, int(y.shape[2]), int(y.shape[3]), int(up), int(k), int(adjoint)
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_clip_resample(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_clip_resample')


class _NearestUpAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, up, k):
        ctx.up, ctx.k, ctx.shape = up, k, tuple(x.shape)
        y = torch.empty(list(x.shape[:2]) + [out_size(x.shape[2], up, k), out_size(x.shape[3], up, k)], dtype=torch.float32, device=x.device)
        _launch(x, y, up, k, False)
        return y

    @staticmethod
    def backward(ctx, dy):
        if torch.is_grad_enabled() and dy.requires_grad:          # double backward: the op is linear, so the composite's adjoint at any point
            x = torch.zeros(ctx.shape, dtype=dy.dtype, device=dy.device, requires_grad=True)
            return torch.autograd.grad(composite(x, ctx.up, ctx.k), x, dy, create_graph=True)[0], None, None
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dy.device)
        _launch(dx, dy.detach(), ctx.up, ctx.k, True)
        return dx, None, None


def nearest_up_avg_pool(x, up, k):
    """x [B,C,H,W] floating point (any strides) -> avg_pool2d(nearest upsampling by the integer `up`, kernel and stride `k`).
    CUDA float32 runs the HIP kernel, forward and backward one launch each on the current stream; everything else `composite`."""
    if not isinstance(x, torch.Tensor) or not x.is_floating_point() or x.ndim != 4:
        raise RuntimeError(f'nearest_up_avg_pool: x must be a floating-point [B,C,H,W] tensor, got {getattr(x, "dtype", type(x))} {list(getattr(x, "shape", []))}')
    if int(up) != up or int(k) != k or up < 1 or k < 1:
        raise RuntimeError(f'nearest_up_avg_pool: up and k must be positive integers, got {up}, {k}')
    up, k = int(up), int(k)
    if out_size(x.shape[2], up, k) < 1 or out_size(x.shape[3], up, k) < 1:
        raise RuntimeError(f'nearest_up_avg_pool: {list(x.shape)} upsampled by {up} is smaller than the pooling window {k}')
    if not (x.is_cuda and x.dtype == torch.float32) or x.numel() == 0:
        return composite(x, up, k)
    return _NearestUpAvgPool.apply(x, up, k)
