"""Weight gradient of the plain convolutions of torch_utils/ops/plain_conv.py, summed over the batch, on the fp32 matrix cores
(libsg3hip: csrc/sg3_conv2d_wgrad_sum.hip).  With plain_conv_grad.py (the data gradient) this is the convolution half of training
the encoder trunk.

The train-mode BatchNorm in front of a residual unit's first convolution enters as `in_scale` / `in_shift`: the kernel applies
x -> in_scale * x + in_shift to real pixels while it stages them (padding stays zero), so the normalised tensor is never written.
Products are exact fp32 (v_mfma_f32_32x32x2_f32) and the pixel sum has a fixed order: results are bit-identical on repeat."""
import ctypes

import torch

from .. import _sg3abi as abi


def out_size(h, w, k, stride):
    """Output size of the forward convolution (padding k // 2) for an h x w input."""
    pad = k // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def splits(n, i, o, h, w, k, stride):
    """(nSplit, chunksPerSplit, xSegs) of the launch: chunk c = (sample * OH + oy) * xSegs + xs is the output pixels
    [P xs, min(OW, P xs + P)) of one output row, P = 32 // stride; split j sums the chunks [j * chunksPerSplit, (j + 1) * chunksPerSplit).  Host only."""
    out = [ctypes.c_int() for _ in range(3)]
    rc = abi.load().sg3_conv2d_wgrad_sum_splits(n, i, o, h, w, k, stride, *[ctypes.byref(v) for v in out])
    if rc != abi.SG3_OK:
        raise RuntimeError(f'sg3_conv2d_wgrad_sum_splits failed (rc={rc}): {abi.last_error()}')
    return tuple(v.value for v in out)


def wgrad(x, dy, k, stride, in_scale=None, in_shift=None, out=None):
    """x [N,I,H,W], dy [N,O,OH,OW] -> dW [O,I,k,k] = sum over samples and pixels of dy * (in_scale * x + in_shift), zero padded."""
    assert x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and dy.is_cuda and dy.dtype == torch.float32 and dy.ndim == 4
    assert k in (1, 3) and stride in (1, 2) and dy.device == x.device
    x, dy = x.contiguous(), dy.contiguous()
    n, i, h, w = (int(v) for v in x.shape)
    o = int(dy.shape[1])
    if int(dy.shape[0]) != n or tuple(dy.shape[2:]) != out_size(h, w, k, stride):
        raise RuntimeError(f'conv2d_wgrad_sum: dy is {tuple(dy.shape)}, the forward of a {tuple(x.shape)} input with k {k}, stride {stride} '
                           f'gives {(n, o) + out_size(h, w, k, stride)}')
    assert (in_scale is None) == (in_shift is None)
    if in_scale is not None:
        assert in_scale.numel() == i and in_shift.numel() == i
        in_scale = in_scale.detach().to(device=x.device, dtype=torch.float32).contiguous()
        in_shift = in_shift.detach().to(device=x.device, dtype=torch.float32).contiguous()
    dw = torch.empty([o, i, k, k], dtype=torch.float32, device=x.device) if out is None else out
    assert dw.is_contiguous() and tuple(dw.shape) == (o, i, k, k) and dw.dtype == torch.float32
    n_split = splits(n, i, o, h, w, k, stride)[0]
    partial = torch.empty([n_split, o, i, k, k], dtype=torch.float32, device=x.device) if n_split > 1 else None
    p = abi.Conv2dWgradSumParams()
    p.x, p.dy, p.inScale, p.inShift, p.dw, p.partial = abi.ptr(x), abi.ptr(dy), abi.ptr(in_scale), abi.ptr(in_shift), abi.ptr(dw), abi.ptr(partial)
    p.N, p.I, p.O, p.H, p.W, p.k, p.stride = n, i, o, h, w, k, stride
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_conv2d_wgrad_sum(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_conv2d_wgrad_sum')
    return dw
