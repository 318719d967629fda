"""The kernels of the LPIPS criterion besides the 3x3 convolutions (libsg3hip: csrc/sg3_lpips.hip; criteria/lpips uses them):
the first layer's space-to-depth preparation and its adjoint, the 5x5 convolution (forward and, on transposed flipped weights, data
gradient), MaxPool2d(3, 2) forward and backward, and the per-layer head with its closed-form gradient.  Everything is float32 on
the device, exact fp32 arithmetic, no atomics on floats.  There is no fallback: CPU tensors and other dtypes belong to the
composite in criteria/lpips/lpips.py."""
import ctypes

import torch

from .. import _sg3abi as abi


def _f32_cuda(*tensors):
    for t in tensors:
        assert t.is_cuda and t.dtype == torch.float32, 'lpips_ops: CUDA float32 tensors only'


def conv1_out_size(h, w):
    """Output size of the 11x11 stride-4 pad-2 convolution."""
    return (h - 7) // 4 + 1, (w - 7) // 4 + 1


def regroup_conv1_weight(w):
    """[O,3,11,11] -> [O,48,3,3]: zero-extended to 12x12 and regrouped so that the layer is a valid 3x3 convolution over the
    canvas of `prepare` (channel c*16 + ry*4 + rx)."""
    o = w.shape[0]
    w12 = torch.zeros([o, 3, 12, 12], dtype=w.dtype, device=w.device)
    w12[:, :, :11, :11] = w
    return w12.view(o, 3, 3, 4, 3, 4).permute(0, 1, 3, 5, 2, 4).reshape(o, 48, 3, 3).contiguous()


def _prepare_params(x, canvas, mean, std, scale=None):
    n, _, h, w = (int(v) for v in x.shape)
    p = abi.LpipsPrepareParams()
    p.x, p.xStride, p.canvas, p.scale = abi.ptr(x), abi.strides4(x), abi.ptr(canvas), abi.ptr(scale)
    p.N, p.H, p.W = n, h, w
    p.mean, p.std = (abi.c_f32 * 3)(*mean), (abi.c_f32 * 3)(*std)
    return p


def prepare(x, mean, std, out=None):
    """x [N,3,H,W] (any strides) -> the z-scored, zero-framed, pixel-unshuffled canvas [N,48,OH+2,OW+2].  `mean`, `std`: 3 floats."""
    _f32_cuda(x)
    assert x.ndim == 4 and x.shape[1] == 3
    oh, ow = conv1_out_size(int(x.shape[2]), int(x.shape[3]))
    canvas = torch.empty([x.shape[0], 48, oh + 2, ow + 2], dtype=torch.float32, device=x.device) if out is None else out
    assert canvas.is_contiguous() and tuple(canvas.shape) == (x.shape[0], 48, oh + 2, ow + 2) and canvas.dtype == torch.float32
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_lpips_prepare(ctypes.byref(_prepare_params(x, canvas, mean, std)), abi.stream_ptr(x.device)), 'sg3_lpips_prepare')
    return canvas


def prepare_bwd(dcanvas, hw, mean, std, scale=None, out=None):
    """The adjoint of `prepare`: dcanvas [N,48,OH+2,OW+2] -> dx [N,3,H,W] with (H, W) = hw, times the device scalar `scale`."""
    _f32_cuda(dcanvas)
    h, w = int(hw[0]), int(hw[1])
    oh, ow = conv1_out_size(h, w)
    assert dcanvas.is_contiguous() and tuple(dcanvas.shape[1:]) == (48, oh + 2, ow + 2)
    dx = torch.empty([dcanvas.shape[0], 3, h, w], dtype=torch.float32, device=dcanvas.device) if out is None else out
    assert tuple(dx.shape) == (dcanvas.shape[0], 3, h, w) and dx.dtype == torch.float32 and dx.device == dcanvas.device
    if scale is not None:
        _f32_cuda(scale)
        assert scale.numel() == 1
    with torch.cuda.device(dx.device):
        abi.check(abi.load().sg3_lpips_prepare_bwd(ctypes.byref(_prepare_params(dx, dcanvas, mean, std, scale)), abi.stream_ptr(dx.device)),
                  'sg3_lpips_prepare_bwd')
    return dx


class PackedConv5:
    """A 5x5 stride-1 pad-2 convolution in the operand layout of sg3_conv2d_k5.  `transpose=True` packs the weight of the data
    gradient (channels swapped, taps flipped): `run(dy)` is then conv_transpose2d(dy, weight, padding=2)."""

    def __init__(self, weight, bias=None, relu=False, transpose=False):
        _f32_cuda(weight)
        assert weight.ndim == 4 and tuple(weight.shape[2:]) == (5, 5)
        w = weight.detach()
        if transpose:
            assert bias is None and not relu
            w = w.permute(1, 0, 2, 3).flip(2, 3)
        w = w.contiguous()
        self.O, self.I, self.relu = int(w.shape[0]), int(w.shape[1]), int(bool(relu))
        self.bias = None if bias is None else bias.detach().to(device=w.device, dtype=torch.float32).contiguous()
        lib = abi.load()
        self.packed = torch.empty([int(lib.sg3_conv2d_k5_packed_floats(self.O, self.I))], dtype=torch.float32, device=w.device)
        with torch.cuda.device(w.device):
            abi.check(lib.sg3_conv2d_k5_pack(abi.ptr(w), abi.ptr(self.packed), self.O, self.I, abi.stream_ptr(w.device)), 'sg3_conv2d_k5_pack')

    def run(self, x, out=None):
        _f32_cuda(x)
        assert x.ndim == 4 and x.shape[1] == self.I
        x = x.contiguous()
        n, _, h, w = (int(v) for v in x.shape)
        out = torch.empty([n, self.O, h, w], dtype=torch.float32, device=x.device) if out is None else out
        assert out.is_contiguous() and tuple(out.shape) == (n, self.O, h, w) and out.dtype == torch.float32
        p = abi.Conv2dK5Params()
        p.x, p.wPacked, p.bias, p.out = abi.ptr(x), abi.ptr(self.packed), abi.ptr(self.bias), abi.ptr(out)
        p.N, p.I, p.O, p.H, p.W, p.relu = n, self.I, self.O, h, w, self.relu
        with torch.cuda.device(x.device):
            abi.check(abi.load().sg3_conv2d_k5(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_conv2d_k5')
        return out

    __call__ = run


def maxpool3s2(x, out=None):
    """F.max_pool2d(x, 3, 2), bit for bit."""
    _f32_cuda(x)
    assert x.ndim == 4
    x = x.contiguous()
    n, c, h, w = (int(v) for v in x.shape)
    if h < 3 or w < 3:
        raise RuntimeError(f'maxpool3s2: a {h} x {w} input has no 3 x 3 window')
    y = torch.empty([n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1], dtype=torch.float32, device=x.device) if out is None else out
    assert y.is_contiguous() and tuple(y.shape) == (n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1) and y.dtype == torch.float32
    p = abi.Maxpool3s2Params()
    p.x, p.y, p.N, p.C, p.H, p.W = abi.ptr(x), abi.ptr(y), n, c, h, w
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_maxpool3s2(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_maxpool3s2')
    return y


def maxpool3s2_bwd(x, dy, addend=None, relu_mask=False, out=None):
    """dx = sum of dy over the windows whose first maximum is the pixel (+ addend), times (x > 0) when `relu_mask`.  `out` may be
    any strided [N,C,H,W] view (the interior of a zeroed frame)."""
    _f32_cuda(x, dy)
    assert x.is_contiguous() and dy.is_contiguous() and x.ndim == 4
    n, c, h, w = (int(v) for v in x.shape)
    assert tuple(dy.shape) == (n, c, (h - 3) // 2 + 1, (w - 3) // 2 + 1)
    dx = torch.empty_like(x) if out is None else out
    assert tuple(dx.shape) == tuple(x.shape) and dx.dtype == torch.float32 and dx.device == x.device
    if addend is not None:
        _f32_cuda(addend)
        assert addend.is_contiguous() and tuple(addend.shape) == tuple(x.shape)
    p = abi.Maxpool3s2BwdParams()
    p.x, p.dy, p.addend, p.dx, p.dxStride = abi.ptr(x), abi.ptr(dy), abi.ptr(addend), abi.ptr(dx), abi.strides4(dx)
    p.N, p.C, p.H, p.W, p.reluMask = n, c, h, w, int(bool(relu_mask))
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_maxpool3s2_bwd(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_maxpool3s2_bwd')
    return dx


_counters = {}


def _counter(device, n):
    """The tickets of the head's last-workgroup sum: zero between launches (the kernel leaves them so), one buffer per device and
    stream."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _counters.get(key)
    if buf is None or buf.numel() < n:
        buf = _counters[key] = torch.zeros([max(n, 16)], dtype=torch.int32, device=device)
    return buf


def head(fx, fy, lin, want_grad=False, relu_mask=False, value=None, grad_out=None):
    """One LPIPS layer: (value [N], dfx or None).  value[n] = mean_hw sum_c lin_c (n(fx) - n(fy))^2; dfx = d value[n] / d fx[n] in closed
    form (0 for pixels whose channel norm is 0; with `relu_mask` also 0 where fx <= 0).  `value` may be a preallocated [N] view, `grad_out` a preallocated tensor
    like fx (it implies `want_grad`)."""
    _f32_cuda(fx, fy, lin)
    assert fx.ndim == 4 and fx.shape == fy.shape and fx.is_contiguous() and fy.is_contiguous() and lin.numel() == fx.shape[1]
    n, c, h, w = (int(v) for v in fx.shape)
    lin = lin.detach().reshape(-1).contiguous()
    lib = abi.load()
    value = torch.empty([n], dtype=torch.float32, device=fx.device) if value is None else value
    assert value.is_contiguous() and value.numel() == n and value.dtype == torch.float32
    dfx = grad_out if grad_out is not None else (torch.empty_like(fx) if want_grad else None)
    assert dfx is None or (dfx.is_contiguous() and dfx.shape == fx.shape and dfx.dtype == torch.float32 and dfx.device == fx.device)
    with torch.cuda.device(fx.device):
        partial = torch.empty([n * int(lib.sg3_lpips_head_blocks(h, w))], dtype=torch.float32, device=fx.device)
        p = abi.LpipsHeadParams()
        p.fx, p.fy, p.lin, p.value, p.dfx, p.partial = abi.ptr(fx), abi.ptr(fy), abi.ptr(lin), abi.ptr(value), abi.ptr(dfx), abi.ptr(partial)
        p.counter = abi.ptr(_counter(fx.device, n))
        p.N, p.C, p.h, p.w, p.reluMask = n, c, h, w, int(bool(relu_mask))
        abi.check(lib.sg3_lpips_head(ctypes.byref(p), abi.stream_ptr(fx.device)), 'sg3_lpips_head')
    return value, dfx
