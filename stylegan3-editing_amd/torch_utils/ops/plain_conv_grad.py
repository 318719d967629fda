"""Data gradient of the plain convolutions of torch_utils/ops/plain_conv.py on the fp32 matrix cores (libsg3hip:
csrc/sg3_conv2d_dgrad.hip), with the element-wise neighbours of the backward pass fused in: the BatchNorm behind the forward
convolution folded into the weights, the BatchNorm in front of it as an output scale, the derivative of the PReLU in front as an
epilogue mask, and the gradient arriving over the shortcut as an epilogue addend.

Only the gradient with respect to the input exists: the identity loss differentiates through a frozen network (criteria/id_loss.py).
Products are exact fp32 (v_mfma_f32_32x32x2_f32): gradients at these layers are small enough (1e-4 .. 1e-9) that the absolute floor
of a split-precision operand would swamp them."""
import ctypes

import torch

from .. import _sg3abi as abi


class PackedDgrad:
    """Transposed weights of one convolution (kernel 1 or 3, stride 1 or 2, padding k // 2) in the operand layout of
    sg3_conv2d_dgrad.  `k_scale` [O] multiplies the forward's output channels (a folded BatchNorm behind it), `out_scale` [I]
    its input channels (an eval-mode BatchNorm in front of it)."""

    def __init__(self, weight, k_scale=None, out_scale=None, stride=1):
        assert weight.is_cuda and weight.dtype == torch.float32 and weight.ndim == 4 and weight.shape[2] == weight.shape[3]
        self.O, self.I, self.k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        assert self.k in (1, 3) and stride in (1, 2)
        self.stride = int(stride)
        dev = weight.device
        w = weight.detach()
        if k_scale is not None:
            w = w * k_scale.detach().to(device=dev, dtype=torch.float32).view(-1, 1, 1, 1)
        wt = w.permute(1, 0, 2, 3).contiguous()
        scale = None if out_scale is None else out_scale.detach().to(device=dev, dtype=torch.float32).contiguous()
        lib = abi.load()
        self.packed = torch.empty([int(lib.sg3_modconv_packed_floats(self.I, self.O, self.k, abi.SG3_CONV_FP32))], dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            abi.check(lib.sg3_conv2d_pack(abi.ptr(wt), abi.ptr(scale), abi.ptr(self.packed), None, self.I, self.O, self.k, abi.SG3_CONV_FP32,
                                          abi.stream_ptr(dev)), 'sg3_conv2d_pack')

    def out_size(self, h, w):
        """Output size of the forward convolution for an h x w input."""
        pad = self.k // 2
        return (h + 2 * pad - self.k) // self.stride + 1, (w + 2 * pad - self.k) // self.stride + 1

    def run(self, dy, in_hw, act=None, slope=None, addend=None, out=None):
        """dy [N,O,OH,OW] -> dx [N,I,H,W] with (H, W) = in_hw:  dx = conv_transpose(dy) (+ addend, any strides), then times the
        derivative of the PReLU with per-channel `slope` whose saved output (all slopes >= 0) or pre-activation is `act`."""
        assert dy.is_cuda and dy.dtype == torch.float32 and dy.ndim == 4 and dy.shape[1] == self.O
        dy = dy.contiguous()
        n, h, w = int(dy.shape[0]), int(in_hw[0]), int(in_hw[1])
        if tuple(dy.shape[2:]) != self.out_size(h, w):
            raise RuntimeError(f'conv2d_dgrad: dy is {tuple(dy.shape[2:])}, the forward of a {h} x {w} input gives {self.out_size(h, w)}')
        dx = torch.empty([n, self.I, h, w], dtype=torch.float32, device=dy.device) if out is None else out
        assert dx.is_contiguous() and tuple(dx.shape) == (n, self.I, h, w) and dx.dtype == torch.float32
        p = abi.Conv2dDgradParams()
        p.dy, p.wPacked, p.dx = abi.ptr(dy), abi.ptr(self.packed), abi.ptr(dx)
        if act is not None:
            assert act.is_contiguous() and tuple(act.shape) == tuple(dx.shape) and act.dtype == torch.float32 and slope is not None and slope.numel() == self.I
            slope = slope.detach().to(torch.float32).contiguous()
            p.act, p.slope = abi.ptr(act), abi.ptr(slope)
        if addend is not None:
            assert tuple(addend.shape) == tuple(dx.shape) and addend.dtype == torch.float32 and addend.device == dx.device
            p.addend, p.addStride = abi.ptr(addend), abi.strides4(addend)
        p.N, p.I, p.O, p.H, p.W, p.OH, p.OW = n, self.I, self.O, h, w, int(dy.shape[2]), int(dy.shape[3])
        p.k, p.stride = self.k, self.stride
        with torch.cuda.device(dy.device):
            abi.check(abi.load().sg3_conv2d_dgrad(ctypes.byref(p), abi.stream_ptr(dy.device)), 'sg3_conv2d_dgrad')
        return dx
