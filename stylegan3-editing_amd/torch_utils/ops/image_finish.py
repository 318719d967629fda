"""Rendered images -> the uint8 tiles the editing scripts save, on the device (libsg3hip: csrc/sg3_image_finish.hip).

The reference finishes every edited image on the CPU: `tensor2im` (utils/common.py:39-45) and, for the result strips, PIL's
`Image.resize` (inversion/scripts/inference_editing.py:82-85).  `to_uint8` computes exactly that, bit for bit, for a whole batch
in one launch: `to_uint8(x, size)[b] == np.array(tensor2im(x[b]).resize(size))`.  The kernel's fixed-point bicubic taps are
PIL's, built on the host in double precision by `sg3_resample_coeffs` and kept on the device per (in, out, device)."""
import ctypes

import numpy as np
import torch

from .. import _sg3abi as abi

_tables = {}


def _table(n_in, n_out, device):
    key = (int(n_in), int(n_out), str(device))
    if key not in _tables:
        lib = abi.load()
        k = lib.sg3_resample_coeffs(n_in, n_out, None, None)
        if k <= 0:
            raise RuntimeError(f'to_uint8: no resampling table for {n_in} -> {n_out}: {abi.last_error()}')
        bounds = np.zeros([n_out, 2], np.int32)
        coeffs = np.zeros([n_out, k], np.int32)
        if lib.sg3_resample_coeffs(n_in, n_out, bounds.ctypes.data, coeffs.ctypes.data) != k:
            raise RuntimeError(f'to_uint8: sg3_resample_coeffs failed: {abi.last_error()}')
        _tables[key] = (torch.from_numpy(bounds).to(device), torch.from_numpy(coeffs).to(device), k)
    return _tables[key]


def _check_out(out, shape, device):
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or out.device != torch.device(device):
        raise RuntimeError(f'to_uint8: out must be uint8 {list(shape)} on {device}, got {out.dtype} {list(out.shape)} on {out.device}')
    return out


def to_uint8(x, size=None, out=None):
    """x [B,3,H,W] floating point (any strides), size (w, h) as in PIL or None (no resize), out: optional uint8 [B,h,w,3] to
    fill (any strides, e.g. the column band `strip[:, :, k*w:(k+1)*w]` of a result strip).  Returns out.
    CUDA float32 input runs the HIP kernel; any other input takes tensor2im + PIL, which is the definition."""
    if not isinstance(x, torch.Tensor) or not x.is_floating_point():
        raise RuntimeError(f'to_uint8: x must be a floating-point tensor, got {getattr(x, "dtype", type(x))}')
    if x.ndim != 4 or int(x.shape[1]) != 3:
        raise RuntimeError(f'to_uint8: x must be [B,3,H,W], got {list(x.shape)}')
    b, _, hh, ww = (int(v) for v in x.shape)
    if size is None:
        w, h = ww, hh
    else:
        if len(size) != 2 or int(size[0]) <= 0 or int(size[1]) <= 0:
            raise RuntimeError(f'to_uint8: size must be (w, h) with positive entries, got {size}')
        w, h = int(size[0]), int(size[1])
    out = _check_out(out, [b, h, w, 3], x.device)
    if b == 0:
        return out
    if not (x.is_cuda and x.dtype == torch.float32):
        from utils.common import tensor2im
        for i in range(b):
            im = tensor2im(x[i])
            if (w, h) != im.size:
                im = im.resize((w, h))
            out[i].copy_(torch.from_numpy(np.array(im)))
        return out
    lib = abi.load()
    p = abi.ImageFinishParams()
    p.x, p.y = abi.ptr(x), abi.ptr(out)
    p.xStride, p.yStride = abi.strides4(x), abi.strides4(out)
    p.B, p.H, p.W, p.h, p.w = b, hh, ww, h, w
    if w != ww:
        bh, ch, p.kH = _table(ww, w, x.device)
        p.boundsH, p.coeffsH = abi.ptr(bh), abi.ptr(ch)
    if h != hh:
        bv, cv, p.kV = _table(hh, h, x.device)
        p.boundsV, p.coeffsV = abi.ptr(bv), abi.ptr(cv)
    with torch.cuda.device(x.device):
        abi.check(lib.sg3_image_finish(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_image_finish')
    return out
