"""Pool-to-256, crop and pool-to-112 of the identity loss, fused (libsg3hip: csrc/sg3_face_pool.hip).

The reference prepares the ArcFace input with `AdaptiveAvgPool2d((256, 256))` (only when `x.shape[2] != 256`), the crop
`[:, :, 35:223, 32:220]` and `AdaptiveAvgPool2d((112, 112))` (criteria/id_loss.py extract_feats).  `composite` below is those torch
calls and is the definition.  Together they are one separable banded linear map per plane, `out = Ay @ X @ Ax.T` (`matrices`);
`face_pool` runs it as one HIP launch that reads the source once and writes no 256 x 256 intermediate, and its adjoint as one
launch in gather form (no atomics: deterministic, exact zeros outside the crop's footprint).  CPU tensors, other dtypes and
double backward take the composite."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from .. import _sg3abi as abi

OUT = 112
_ROWS, _COLS = (35, 223), (32, 220)


def composite(x):
    """The definition: x [B,C,H,W] floating point -> [B,C,112,112], differentiable."""
    if x.shape[2] != 256:
        x = F.adaptive_avg_pool2d(x, (256, 256))
    return F.adaptive_avg_pool2d(x[:, :, _ROWS[0]:_ROWS[1], _COLS[0]:_COLS[1]], (OUT, OUT))


def adaptive_pool_matrix(n_in, n_out):
    """[n_out, n_in] float64 weights of adaptive average pooling: window [floor(i n_in / n_out), ceil((i + 1) n_in / n_out))."""
    m = np.zeros([n_out, n_in], dtype=np.float64)
    for i in range(n_out):
        a, b = (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)
        m[i, a:b] = 1.0 / (b - a)
    return m


def matrices(h, w):
    """(Ay [112, h], Ax [112, w]) float64 with composite(x) == Ay @ x @ Ax.T per plane."""
    pool = h != 256
    out = []
    for n, (lo, hi) in ((h, _ROWS), (w, _COLS)):
        first = adaptive_pool_matrix(n, 256) if pool else np.eye(n)
        crop = first[lo:hi]
        out.append(adaptive_pool_matrix(crop.shape[0], OUT) @ crop)
    return out[0], out[1]


def _launch(x, y, adjoint):
    b, c, h, w = (int(v) for v in x.shape)
    p = abi.FacePoolParams()
    p.x, p.y = abi.ptr(x), abi.ptr(y)
    p.xStride, p.yStride = abi.strides4(x), abi.strides4(y)
    p.B, p.C, p.H, p.W, p.pool, p.adjoint = b, c, h, w, int(h != 256), int(adjoint)
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_face_pool(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_face_pool')


class _FacePool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.shape = tuple(x.shape)
        y = torch.empty(list(x.shape[:2]) + [OUT, OUT], dtype=torch.float32, device=x.device)
        _launch(x, y, False)
        return y

    @staticmethod
    def backward(ctx, dy):
        if torch.is_grad_enabled() and dy.requires_grad:          # double backward: the op is linear, so the composite's adjoint at any point
            x = torch.zeros(ctx.shape, dtype=dy.dtype, device=dy.device, requires_grad=True)
            return torch.autograd.grad(composite(x), x, dy, create_graph=True)[0]
        dx = torch.empty(ctx.shape, dtype=torch.float32, device=dy.device)
        _launch(dx, dy.detach(), True)
        return dx


def face_pool(x):
    """x [B,C,H,W] floating point (any strides) -> [B,C,112,112].  CUDA float32 runs the HIP kernel, forward and backward one
    launch each on the current stream; everything else `composite`."""
    if not isinstance(x, torch.Tensor) or not x.is_floating_point() or x.ndim != 4:
        raise RuntimeError(f'face_pool: x must be a floating-point [B,C,H,W] tensor, got {getattr(x, "dtype", type(x))} {list(getattr(x, "shape", []))}')
    if not (x.is_cuda and x.dtype == torch.float32) or x.numel() == 0:
        return composite(x)
    return _FacePool.apply(x)
