"""Learned Perceptual Image Patch Similarity, AlexNet variant, version 0.1 (reference criteria/lpips/lpips.py): the perceptual term
of PTI's loss.

    LPIPS(x, y) = sum over the five tapped layers l and the samples of  mean_hw( lin_l( (n(fx_l) - n(fy_l))^2 ) ) / N

with f_l the post-ReLU AlexNet features of the z-scored image and n() the per-pixel unit normalisation over channels.

Weights are never downloaded and torchvision is not needed: `alexnet_weights` is a torchvision AlexNet state dict (or its path;
`features.N.*`, `classifier.*` ignored), `lin_weights` the published linear layers (`lin0.model.1.weight` ... or renamed).  The
module is frozen, in eval mode and stays on the CPU until the caller moves it.

Two paths, chosen as IDLoss chooses (`uses_hip`): a CUDA float32 [N,3,H,W] `x` with no parameter recording a gradient runs on
libsg3hip, forward and backward (csrc/sg3_lpips.hip, sg3_conv2d, sg3_conv2d_dgrad; exact fp32 products, no float atomics, results
bit-identical on repeat); anything else is the composite under autograd, which is the reference's formula unchanged.  `y` is a
constant of the loss on the HIP path: its features are computed without saving anything and kept across calls (one entry, keyed
on the tensor's address, version, shape and device and on the parameters' addresses and versions -- PTI passes the same target
for 350 steps); `clear_cache()` drops them.

A pixel whose channels are all zero (r = |fx| = 0): the reference's autograd differentiates sqrt at 0 and returns NaN there, which
spreads over the whole image gradient.  The HIP path writes 0 for that pixel's head gradient instead: every channel of such a pixel
sits at ReLU's zero, so any finite value would be masked to 0 by the ReLU derivative one step later anyway.  The composite keeps
the reference's behaviour.

Images need H, W >= 31 (one pixel must be left after the second pool); smaller ones raise RuntimeError on both paths."""
import torch
import torch.nn as nn

from criteria.lpips.networks import get_network, LinLayers
from criteria.lpips.utils import alexnet_features_state, get_state_dict

MIN_SIZE = 31


class LPIPS(nn.Module):
    def __init__(self, net_type: str = 'alex', version: str = '0.1', alexnet_weights=None, lin_weights=None, pretrained: bool = True):
        assert version in ['0.1'], 'v0.1 is only supported now'
        super().__init__()
        self.net = get_network(net_type)
        self.lin = LinLayers(self.net.n_channels_list)
        if pretrained:
            if alexnet_weights is None or lin_weights is None:
                raise ValueError('LPIPS: give the pretrained weights as alexnet_weights (torchvision AlexNet state dict or path) and '
                                 'lin_weights (LPIPS v0.1 alex linear layers, state dict or path); nothing is downloaded')
            self.net.layers.load_state_dict(alexnet_features_state(alexnet_weights))
            self.lin.load_state_dict(get_state_dict(lin_weights))
        self.requires_grad_(False)
        self.eval()
        self._hip = None            # (key, packed operands)
        self._y_cache = None        # (key, raw features of y)

    # ---- which path ---------------------------------------------------------------------------------------------------------

    def uses_hip(self, x):
        """Does `forward(x, y)` take the HIP path?"""
        return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.shape[1] == 3
                and not any(p.requires_grad for p in self.parameters()))

    def clear_cache(self):
        self._y_cache = None

    def _apply(self, fn, *args, **kwargs):
        self._hip, self._y_cache = None, None                  # .to() / .float(): packed operands and cached features are stale
        return super()._apply(fn, *args, **kwargs)

    # ---- the composite: the reference's formula ------------------------------------------------------------------------------

    def layer_terms(self, x, y):
        """[5, N] per-layer, per-sample terms of the composite."""
        feat_x, feat_y = self.net(x), self.net(y)
        diff = [(fx - fy) ** 2 for fx, fy in zip(feat_x, feat_y)]
        return torch.stack([l(d).mean((2, 3), True).reshape(-1) for d, l in zip(diff, self.lin)])

    def composite(self, x, y):
        feat_x, feat_y = self.net(x), self.net(y)
        diff = [(fx - fy) ** 2 for fx, fy in zip(feat_x, feat_y)]
        res = [l(d).mean((2, 3), True) for d, l in zip(diff, self.lin)]
        return torch.sum(torch.cat(res, 0)) / x.shape[0]

    # ---- the HIP path --------------------------------------------------------------------------------------------------------

    def _param_key(self):
        tensors = list(self.net.layers.parameters()) + list(self.lin.parameters()) + [self.net.mean, self.net.std]
        return tuple((t.data_ptr(), t._version) for t in tensors)

    def _operands(self, device):
        """Packed weights of the five convolutions and their data gradients, built on first use and again when a parameter changed."""
        from torch_utils.ops import lpips_ops
        from torch_utils.ops.plain_conv import ACT_PRELU, PackedConv
        from torch_utils.ops.plain_conv_grad import PackedDgrad
        key = (self._param_key(), device)
        if self._hip is not None and self._hip[0] == key:
            return self._hip[1]
        convs = [self.net.layers[i] for i in (0, 3, 6, 8, 10)]
        if any(c.weight.device != device for c in convs):
            raise RuntimeError(f'LPIPS: the input is on {device}, the network on {convs[0].weight.device}; move the criterion first')
        ops = type('LpipsOperands', (), {})()
        ops.mean = [float(v) for v in self.net.mean.flatten().tolist()]
        ops.std = [float(v) for v in self.net.std.flatten().tolist()]
        zeros = {c: torch.zeros([c], dtype=torch.float32, device=device) for c in (48, 64, 192, 384, 256)}
        ops.zeros = zeros

        def relu_conv(weight, bias, padding):
            return PackedConv(weight, bias=bias, act=ACT_PRELU, slope=zeros[int(weight.shape[0])], stride=1, padding=padding, precision='fp32')

        w1 = lpips_ops.regroup_conv1_weight(convs[0].weight.detach().float())
        ops.conv = [relu_conv(w1, convs[0].bias, 0),
                    lpips_ops.PackedConv5(convs[1].weight.detach().float(), bias=convs[1].bias, relu=True)]
        ops.conv += [relu_conv(c.weight.detach().float(), c.bias, 1) for c in convs[2:]]
        ops.dgrad = [PackedDgrad(w1), lpips_ops.PackedConv5(convs[1].weight.detach().float(), transpose=True)]
        ops.dgrad += [PackedDgrad(c.weight.detach().float()) for c in convs[2:]]
        ops.lin = [l[1].weight.detach().float().reshape(-1).contiguous() for l in self.lin]
        self._hip = (key, ops)
        return ops

    def _features_hip(self, x, ops):
        """The five tapped (post-ReLU, pre-pool) feature maps of x: 1 prepare + 5 convolutions + 2 pools."""
        from torch_utils.ops import lpips_ops
        f1 = ops.conv[0](lpips_ops.prepare(x, ops.mean, ops.std))
        f2 = ops.conv[1](lpips_ops.maxpool3s2(f1))
        f3 = ops.conv[2](lpips_ops.maxpool3s2(f2))
        f4 = ops.conv[3](f3)
        f5 = ops.conv[4](f4)
        return [f1, f2, f3, f4, f5]

    def _y_features(self, y, ops):
        key = (y.data_ptr(), y._version, tuple(y.shape), y.device, self._hip[0])
        if self._y_cache is None or self._y_cache[0] != key:
            self._y_cache = None
            self._y_cache = (key, self._features_hip(y, ops))
        return self._y_cache[1]

    def layer_terms_hip(self, x, y):
        """[5, N] per-layer, per-sample terms on the HIP path (no gradient)."""
        ops = self._operands(x.device)
        with torch.no_grad():
            return _LpipsHip.run(self, ops, x.detach(), y.detach(), False)[0]

    # ---- forward -------------------------------------------------------------------------------------------------------------

    def forward(self, x: torch.Tensor, y: torch.Tensor):
        if x.ndim != 4 or tuple(x.shape) != tuple(y.shape):
            raise RuntimeError(f'LPIPS: x and y must be [N,3,H,W] tensors of one shape, got {list(x.shape)} and {list(y.shape)}')
        if x.shape[2] < MIN_SIZE or x.shape[3] < MIN_SIZE:
            raise RuntimeError(f'LPIPS: images must be at least {MIN_SIZE} x {MIN_SIZE} (one pixel left after the second pool), got '
                               f'{x.shape[2]} x {x.shape[3]}')
        if not (self.uses_hip(x) and self.uses_hip(y) and y.device == x.device):
            return self.composite(x, y)
        return _LpipsHip.apply(x, y.detach(), self)


class _LpipsHip(torch.autograd.Function):
    """The whole HIP path as one node: the backward returns the gradient for x only."""

    @staticmethod
    def run(module, ops, x, y, want_grad):
        """([5, N] terms, features of x, head gradients or None)"""
        from torch_utils.ops import lpips_ops
        fy = module._y_features(y, ops)
        fx = module._features_hip(x, ops)
        n = int(x.shape[0])
        terms = torch.empty([5, n], dtype=torch.float32, device=x.device)
        # the head of the last layer masks its own gradient with the ReLU derivative; the others meet theirs as addends of the
        # data-gradient epilogues, which mask the sum
        heads = [lpips_ops.head(a, b, lin, want_grad=want_grad, relu_mask=(i == 4), value=terms[i])[1]
                 for i, (a, b, lin) in enumerate(zip(fx, fy, ops.lin))]
        return terms, fx, heads

    @staticmethod
    def forward(ctx, x, y, module):
        ops = module._operands(x.device)
        want_grad = ctx.needs_input_grad[0]
        terms, fx, heads = _LpipsHip.run(module, ops, x, y, want_grad)
        ctx.ops, ctx.hw, ctx.n = ops, (int(x.shape[2]), int(x.shape[3])), int(x.shape[0])
        if want_grad:
            ctx.save_for_backward(*fx, *heads)
        return terms.sum() / x.shape[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        from torch_utils.ops import lpips_ops
        ops = ctx.ops
        f1, f2, f3, f4, f5, h1, h2, h3, h4, h5 = ctx.saved_tensors
        d4 = ops.dgrad[4].run(h5, f4.shape[2:], act=f4, slope=ops.zeros[256], addend=h4)         # at conv 4's output
        d3 = ops.dgrad[3].run(d4, f3.shape[2:], act=f3, slope=ops.zeros[384], addend=h3)         # at conv 3's output
        dp2 = ops.dgrad[2].run(d3, f3.shape[2:])                                                  # at the second pool's output
        d2 = lpips_ops.maxpool3s2_bwd(f2, dp2, addend=h2, relu_mask=True)                         # at conv 2's output
        dp1 = ops.dgrad[1].run(d2)                                                                # at the first pool's output
        oh, ow = int(f1.shape[2]), int(f1.shape[3])
        ring = torch.zeros([ctx.n, 64, oh + 2, ow + 2], dtype=torch.float32, device=f1.device)
        lpips_ops.maxpool3s2_bwd(f1, dp1, addend=h1, relu_mask=True, out=ring[:, :, 1:-1, 1:-1])  # at conv 1's output, framed
        dcanvas = ops.dgrad[0].run(ring, (oh + 2, ow + 2))               # pad-1 transpose of the framed dy = the valid convolution's
        scale = (grad_out.detach().to(torch.float32) / ctx.n).reshape(1)
        dx = lpips_ops.prepare_bwd(dcanvas, ctx.hw, ops.mean, ops.std, scale=scale)
        return dx, None, None
