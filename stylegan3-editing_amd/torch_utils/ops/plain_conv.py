"""Plain (non-modulated) convolution on the fp32 matrix cores, with the element-wise neighbours of the ReStyle
encoder's convolutions fused in: an eval-mode BatchNorm in front (per-channel affine applied to real pixels only, so
zero padding stays zero), a BatchNorm behind (folded into the packed weights and the bias), PReLU / leaky ReLU.

Replaces, for inference, the module calls Conv2d / BatchNorm2d / PReLU / LeakyReLU of the IR-SE50 backbone and the
GradualStyleBlock heads (reference models/setgan/encoder/encoders/helpers.py:98-120, restyle_psp_encoders.py:26-50,
map2style.py:15-24).  No autograd here: training the encoder trunk records these forwards and differentiates them by hand with
plain_conv_grad.py (data gradient), plain_conv_wgrad.py (weight gradient) and batchnorm_train.py; there the BatchNorm in front is the
batch's, handed to `run` per call, and nothing is folded into the packed weights.
"""
import ctypes

import torch

from .. import _sg3abi as abi

ACT_NONE, ACT_PRELU, ACT_LRELU = 0, 1, 2

# Arithmetic of the convolutions (3x3 stride 1: the bulk of the backbone; 3x3 stride 2: the first unit of each stage and level 1
# of the style heads; 1x1: the projection shortcuts):
#   'f16x3' : fp16 hi/lo operand split, three fp16 MFMAs per K step, fp32 accumulation (5.3x the fp32 MFMA rate).  Per operand:
#             activations relative 2^-21 plus up to ~2^-23 absolute (below |x| = 2^-3 the halves leave fp16's normal range);
#             weights lifted per output channel by a power of two when packed (undone exactly in the epilogue), relative 2^-22
#             within 2^-17 of their channel's maximum (tests/split_model.py).  Operands must stay inside the fp16 range; every
#             launch checks that on the device and raises a flag (`overflowed`), on which the caller repeats its forward with 'fp32'.
#   'fp32'  : v_mfma_f32_32x32x2_f32, exact products.
precision = 'f16x3'
_flags = {}


def _flag(device):
    key = (device.type, device.index)
    if key not in _flags:
        _flags[key] = torch.zeros([1], dtype=torch.int32, device=device)
    return _flags[key]


def reset_overflow(device):
    _flag(torch.device(device)).zero_()


def overflowed(device):
    """True when a split-precision launch since the last `reset_overflow` met an operand outside the fp16 range
    (synchronises with the device)."""
    return bool(int(_flag(torch.device(device)).item()))


class PackedConv:
    """Weights of one convolution in the implicit-GEMM operand layout, plus its fused epilogue / prologue vectors."""

    def __init__(self, weight, out_scale=None, bias=None, in_scale=None, in_shift=None, act=ACT_NONE, slope=None, stride=1, padding=0,
                 precision=None, chains=False):
        # `chains`: the exact-fp32 form of this object accumulates every output in four chains instead of one (SG3_CONV_FP32_CHAINS: the
        # recorded training forward, whose error would otherwise grow with the 24 units it passes through; same pack)
        self.chains = bool(chains)
        # `precision`: 'fp32' / 'f16x3' for this object whatever the module-wide `precision` says (the LPIPS criterion runs exact fp32);
        # None follows the module-wide setting at every call
        assert precision in (None, 'fp32', 'f16x3')
        self.precision = precision
        assert weight.is_cuda and weight.dtype == torch.float32 and weight.ndim == 4 and weight.shape[2] == weight.shape[3]
        self.O, self.I, self.k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[2])
        assert self.k in (1, 3) and stride in (1, 2)
        self.stride, self.padding, self.act = int(stride), int(padding), int(act)
        dev = weight.device
        self._w = weight.detach().contiguous()
        f32 = lambda t: None if t is None else t.detach().to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        self.out_scale, self.bias, self.in_scale, self.in_shift, self.slope = f32(out_scale), f32(bias), f32(in_scale), f32(in_shift), f32(slope)
        self._packed = {}
        self._scales = {}

    def packed(self, prec):
        """Packed operand image for one arithmetic form (built on first use)."""
        if prec not in self._packed:
            lib = abi.load()
            dev = self._w.device
            buf = torch.empty([int(lib.sg3_modconv_packed_floats(self.O, self.I, self.k, prec))], dtype=torch.float32, device=dev)
            scale = torch.empty([self.O], dtype=torch.float32, device=dev) if prec == abi.SG3_CONV_F16X3 else None
            with torch.cuda.device(dev):
                abi.check(lib.sg3_conv2d_pack(abi.ptr(self._w), abi.ptr(self.out_scale), abi.ptr(buf), abi.ptr(scale), self.O, self.I, self.k, prec,
                                              abi.stream_ptr(dev)), 'sg3_conv2d_pack')
            self._packed[prec], self._scales[prec] = buf, scale
        return self._packed[prec]

    def weight_scale(self, prec):
        """[O] inverse powers of two the f16x3 pack lifted the output channels by (None for 'fp32')."""
        self.packed(prec)
        return self._scales[prec]

    def __call__(self, x):
        return self.run(x)

    def _params(self, x, out, in_scale=None, in_shift=None):
        split = (self.precision or precision) == 'f16x3'
        prec = abi.SG3_CONV_F16X3 if split else abi.SG3_CONV_FP32
        n, _, h, w = (int(v) for v in x.shape)
        p = abi.Conv2dParams()
        p.x, p.wPacked, p.out = abi.ptr(x), abi.ptr(self.packed(prec)), abi.ptr(out)
        p.precision, p.rangeFlag, p.wScale = prec, (abi.ptr(_flag(x.device)) if split else None), abi.ptr(self._scales[prec])
        if self.chains and not split:
            p.precision = abi.SG3_CONV_FP32_CHAINS
        p.inScale, p.inShift = abi.ptr(self.in_scale if in_scale is None else in_scale), abi.ptr(self.in_shift if in_shift is None else in_shift)
        p.bias, p.slope = abi.ptr(self.bias), abi.ptr(self.slope)
        p.N, p.I, p.O, p.H, p.W = n, self.I, self.O, h, w
        p.k, p.stride, p.pad, p.act = self.k, self.stride, self.padding, self.act
        return p

    def form(self, x):
        """The kernel form `run(x)` launches under the current `precision` (or the object's own; sg3_conv2d_form: 0 .. 11 for 'fp32',
        abi.SG3_CONV2D_FORM_F16X3 + 0 .. 5 for 'f16x3'); nothing is launched."""
        assert x.is_cuda and x.ndim == 4 and x.shape[1] == self.I
        with torch.cuda.device(x.device):
            return int(abi.load().sg3_conv2d_form(ctypes.byref(self._params(x, x))))

    def run(self, x, in_scale=None, in_shift=None):
        """`in_scale` / `in_shift` [I] float32 contiguous on x's device: this call's input affine in place of the object's own (a train-mode
        BatchNorm in front, whose statistics belong to the batch)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.shape[1] == self.I
        assert (in_scale is None) == (in_shift is None) and (in_scale is None or (in_scale.numel() == in_shift.numel() == self.I and in_scale.is_contiguous()
                                                                                  and in_shift.is_contiguous() and in_scale.dtype == in_shift.dtype == torch.float32))
        x = x.contiguous()
        n, _, h, w = (int(v) for v in x.shape)
        oh = (h + 2 * self.padding - self.k) // self.stride + 1
        ow = (w + 2 * self.padding - self.k) // self.stride + 1
        out = torch.empty([n, self.O, oh, ow], dtype=torch.float32, device=x.device)
        p = self._params(x, out, in_scale, in_shift)
        with torch.cuda.device(x.device):
            abi.check(abi.load().sg3_conv2d(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_conv2d')
        return out


def bn_affine(bn):
    """Eval-mode BatchNorm2d as y = a * x + b."""
    a = bn.weight.detach() * torch.rsqrt(bn.running_var.detach() + bn.eps)
    b = bn.bias.detach() - bn.running_mean.detach() * a
    return a, b
