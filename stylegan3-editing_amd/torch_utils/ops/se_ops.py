"""Squeeze-and-excitation tail of the IR-SE residual units on libsg3hip (csrc/sg3_se.hip: sg3_se_residual).

Replaces, for GPU inference, `shortcut + res * sigmoid(fc2(relu(fc1(mean_hw(res)))))` of the reference's `SEModule` +
`bottleneck_IR_SE.forward` (models/setgan/encoder/encoders/helpers.py:57-73, :117-120): seven torch launches -> two."""
import ctypes

import torch

from .. import _sg3abi as abi


def _fc(fc1_weight, fc2_weight, c):
    w1 = fc1_weight.detach().reshape(fc1_weight.shape[0], -1).to(torch.float32).contiguous()
    w2 = fc2_weight.detach().reshape(fc2_weight.shape[0], -1).to(torch.float32).contiguous()
    r = int(w1.shape[0])
    if tuple(w1.shape) != (r, c) or tuple(w2.shape) != (c, r):
        raise RuntimeError(f'se_residual: fc1 {tuple(w1.shape)}, fc2 {tuple(w2.shape)} for {c} channels')
    return w1, w2, r


def _forward(res, shortcut, fc1_weight, fc2_weight, out):
    """out = shortcut + res * gate(res) (out may be res); returns the plane means [N,C] the first launch leaves."""
    if not (res.is_cuda and res.dtype == torch.float32 and res.is_contiguous() and shortcut.dtype == torch.float32 and shortcut.device == res.device):
        raise RuntimeError('se_residual: float32 CUDA tensors, res contiguous')
    n, c, h, w = (int(v) for v in res.shape)
    if tuple(shortcut.shape) != (n, c, h, w):
        raise RuntimeError(f'se_residual: shortcut {tuple(shortcut.shape)} vs res {tuple(res.shape)}')
    w1, w2, r = _fc(fc1_weight, fc2_weight, c)
    mean = torch.empty([n, c], dtype=torch.float32, device=res.device)
    p = abi.SeParams()
    p.res, p.shortcut, p.fc1, p.fc2, p.mean, p.out = abi.ptr(res), abi.ptr(shortcut), abi.ptr(w1), abi.ptr(w2), abi.ptr(mean), abi.ptr(out)
    p.scStride = abi.strides4(shortcut)
    p.N, p.C, p.H, p.W, p.R = n, c, h, w, r
    with torch.cuda.device(res.device):
        abi.check(abi.load().sg3_se_residual(ctypes.byref(p), abi.stream_ptr(res.device)), 'sg3_se_residual')
    return mean


def se_residual(res, shortcut, fc1_weight, fc2_weight):
    """res [N,C,H,W] float32 contiguous (overwritten with the result and returned), shortcut [N,C,H,W] (any strides),
    fc1_weight [R,C,1,1] | [R,C], fc2_weight [C,R,1,1] | [C,R]."""
    _forward(res, shortcut, fc1_weight, fc2_weight, res)
    return res


def se_residual_record(res, shortcut, fc1_weight, fc2_weight):
    """`se_residual` for a forward that will be differentiated: `res` is kept (the backward needs it) and the result goes to a new
    tensor.  -> (out, mean [N,C]); the same two launches."""
    out = torch.empty_like(res)
    return out, _forward(res, shortcut, fc1_weight, fc2_weight, out)


def se_residual_bwd(dout, res, mean, fc1_weight, fc2_weight, scatter_hw=None):
    """Backward of `se_residual_record` with respect to res and the shortcut -> (dres, dscatter); see `_backward`."""
    return _backward(dout, res, mean, fc1_weight, fc2_weight, scatter_hw)[:2]


def se_residual_bwd_train(dout, res, mean, fc1_weight, fc2_weight, scatter_hw=None):
    """`se_residual_bwd` that also hands out dg [N,C] = sum_hw dout * res, the gate's upstream gradient the first launch leaves in
    its scratch: with the saved mean it gives the gradients of fc1 and fc2 as two small matrix products (`se_weight_grads`)."""
    return _backward(dout, res, mean, fc1_weight, fc2_weight, scatter_hw)


def se_weight_grads(dg, mean, fc1_weight, fc2_weight):
    """(dfc1, dfc2) of gate = sigmoid(fc2 relu(fc1 mean)) from dg = dL/dgate [N,C] and the saved plane means [N,C].  Plain torch on
    [N,C] / [N,R] tensors: the gate is recomputed from the mean (two matrix products, relu, sigmoid) rather than saved, then the two
    matrix products of the gradients; about nine small launches that the units' ABI-call counts do not include."""
    w1, w2 = fc1_weight.detach().flatten(1), fc2_weight.detach().flatten(1)
    u_pre = mean @ w1.t()
    u = torch.relu(u_pre)
    g = torch.sigmoid(u @ w2.t())
    dz = dg * g * (1 - g)
    du = (dz @ w2) * (u_pre > 0)
    return (du.t() @ mean).view_as(fc1_weight), (dz.t() @ u).view_as(fc2_weight)


def _backward(dout, res, mean, fc1_weight, fc2_weight, scatter_hw):
    """Backward of `se_residual_record` (csrc/sg3_se_bwd.hip, two launches) -> (dres, dscatter, dg).  The shortcut's gradient is `dout`
    itself; with `scatter_hw` = (inH, inW), the size of the input an identity shortcut subsampled by 2, dscatter [N,C,inH,inW] is
    dout at the even positions and zero elsewhere (else None)."""
    if not (dout.is_cuda and dout.dtype == torch.float32 and res.dtype == torch.float32 and res.is_contiguous() and tuple(res.shape) == tuple(dout.shape)):
        raise RuntimeError('se_residual_bwd: float32 CUDA tensors of one shape, res contiguous')
    dout = dout.contiguous()
    n, c, h, w = (int(v) for v in res.shape)
    w1, w2, r = _fc(fc1_weight, fc2_weight, c)
    if tuple(mean.shape) != (n, c) or not mean.is_contiguous() or mean.dtype != torch.float32:
        raise RuntimeError(f'se_residual_bwd: mean {tuple(mean.shape)} for {(n, c)}')
    dg = torch.empty([n, c], dtype=torch.float32, device=res.device)
    dres = torch.empty_like(res)
    p = abi.SeBwdParams()
    p.dout, p.res, p.mean, p.fc1, p.fc2, p.dg, p.dres = abi.ptr(dout), abi.ptr(res), abi.ptr(mean), abi.ptr(w1), abi.ptr(w2), abi.ptr(dg), abi.ptr(dres)
    dsc = None
    if scatter_hw is not None:
        ih, iw = int(scatter_hw[0]), int(scatter_hw[1])
        dsc = torch.empty([n, c, ih, iw], dtype=torch.float32, device=res.device)
        p.dscatter, p.inH, p.inW = abi.ptr(dsc), ih, iw
    p.N, p.C, p.H, p.W, p.R = n, c, h, w, r
    with torch.cuda.device(res.device):
        abi.check(abi.load().sg3_se_residual_bwd(ctypes.byref(p), abi.stream_ptr(res.device)), 'sg3_se_residual_bwd')
    return dres, dsc, dg
