"""ArcFace-style IR / IR-SE backbone (reference models/setgan/encoder/encoders/model_irse.py, from TreB1eN's InsightFace_Pytorch),
module-for-module compatible with the reference so its checkpoints load: `input_layer.*`, `body.N.*`, `output_layer.{0,3,4}.*`.

`forward()` is the plain PyTorch definition, used on CPU and for every other configuration.  `features_hip()` runs the
112 x 112 network in eval mode on libsg3hip and differentiates it with respect to the image by hand (the identity loss,
criteria/id_loss.py): the recording forward is the fused residual units of helpers.py (`forward_hip_record`), the backward walks
them in reverse on the data-gradient kernels (`backward_hip`).  The head -- BatchNorm2d, Flatten, Linear(25088, 512), BatchNorm1d,
l2 norm, folded into one GEMM plus bias -- stays on torch ops, forward and backward: it streams 51 MB of weights for a handful of
rows, one launch each way.  Weights are constants there: no parameter gradient exists on this path."""
import torch
from torch.autograd.function import once_differentiable
from torch.nn import BatchNorm1d, BatchNorm2d, Conv2d, Dropout, Linear, Module, PReLU, Sequential

from models.setgan.encoder.encoders.helpers import Flatten, bottleneck_IR, bottleneck_IR_SE, get_blocks, l2_norm


class Backbone(Module):
    def __init__(self, input_size, num_layers, mode='ir', drop_ratio=0.4, affine=True):
        super().__init__()
        assert input_size in [112, 224], 'input_size should be 112 or 224'
        assert num_layers in [50, 100, 152], 'num_layers should be 50, 100 or 152'
        assert mode in ['ir', 'ir_se'], 'mode should be ir or ir_se'
        self.input_size, self.num_layers, self.mode = input_size, num_layers, mode
        unit_module = bottleneck_IR if mode == 'ir' else bottleneck_IR_SE
        self.input_layer = Sequential(Conv2d(3, 64, (3, 3), 1, 1, bias=False), BatchNorm2d(64), PReLU(64))
        side = 7 if input_size == 112 else 14
        self.output_layer = Sequential(BatchNorm2d(512), Dropout(drop_ratio), Flatten(), Linear(512 * side * side, 512),
                                       BatchNorm1d(512, affine=affine))
        self.body = Sequential(*[unit_module(b.in_channel, b.depth, b.stride) for block in get_blocks(num_layers) for b in block])
        self._packed = None

    def forward(self, x):
        x = self.input_layer(x)
        x = self.body(x)
        x = self.output_layer(x)
        return l2_norm(x)

    # ---- eval-mode path on libsg3hip, differentiable with respect to the image ----
    def invalidate_packed(self):
        self._packed = None
        for m in getattr(self, 'body', ()):
            m._packed = None

    def train(self, mode=True):
        self.invalidate_packed()
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        self.invalidate_packed()
        return super().load_state_dict(*args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self.invalidate_packed()          # .to(device) / .float() move the parameters the packed copies came from
        return super()._apply(fn, *args, **kwargs)

    def hip_ready(self):
        """The module's side of what `features_hip` covers: eval mode, the 112 x 112 network, and no parameter that records a
        gradient (the hand-written backward reaches the image only)."""
        return not self.training and self.input_size == 112 and not any(q.requires_grad for q in self.parameters())

    def hip_supported(self, x):
        """`hip_ready` and a CUDA float32 [N,3,112,112] batch."""
        return (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and tuple(x.shape[1:]) == (3, 112, 112)
                and self.hip_ready())

    def _pack(self):
        from torch_utils.ops.plain_conv import ACT_NONE, ACT_PRELU, PackedConv, bn_affine
        from torch_utils.ops.plain_conv_grad import PackedDgrad
        conv, bn, prelu = self.input_layer[0], self.input_layer[1], self.input_layer[2]
        a, b = bn_affine(bn)
        pk = dict(slope=prelu.weight.detach().to(torch.float32).contiguous(), mixed=bool((prelu.weight.detach() < 0).any()))
        pk['stem'] = PackedConv(conv.weight, out_scale=a, bias=b, act=ACT_PRELU, slope=prelu.weight, stride=1, padding=1)
        if pk['mixed']:                                  # a negative slope: keep the pre-activation (see helpers._grad_pack)
            pk['stem_linear'] = PackedConv(conv.weight, out_scale=a, bias=b, act=ACT_NONE, stride=1, padding=1)
        pk['stem_grad'] = PackedDgrad(conv.weight, k_scale=a, stride=1)
        # head: BatchNorm2d -> Flatten -> Linear -> BatchNorm1d is one affine map (Dropout is the identity in eval mode)
        bn2, lin, bn1 = self.output_layer[0], self.output_layer[3], self.output_layer[4]
        a2, b2 = bn_affine(bn2)
        pix = lin.in_features // a2.numel()
        a2, b2 = a2.repeat_interleave(pix), b2.repeat_interleave(pix)
        s1 = torch.rsqrt(bn1.running_var.detach() + bn1.eps)
        if bn1.weight is not None:
            s1 = s1 * bn1.weight.detach()
        t1 = -bn1.running_mean.detach() * s1
        if bn1.bias is not None:
            t1 = t1 + bn1.bias.detach()
        w = lin.weight.detach()
        pk['head_w'] = (w * a2.unsqueeze(0) * s1.unsqueeze(1)).t().contiguous()                        # [25088, 512]
        pk['head_b'] = (s1 * (w @ b2 + lin.bias.detach()) + t1).contiguous()
        self._packed = pk

    def _trunk_record(self, x, record):
        pk = self._packed
        saved = []
        if record and pk['mixed']:
            act = pk['stem_linear'](x)
            h = torch.nn.functional.prelu(act, pk['slope'])
        else:
            act = h = pk['stem'](x)
        for unit in self.body:
            if record:
                h, s = unit.forward_hip_record(h)
                saved.append(s)
            else:
                h = unit.forward_hip(h)
        return h, (act if record else None), saved

    def _trunk_backward(self, pk, stem_act, saved, d):
        """d [N,512,7,7], the gradient at the body's output -> the gradient at the image, through what `_trunk_record` kept and the
        packed weights `pk` that forward ran on (the record holds them: a `.to()`, `eval()` or `load_state_dict` between forward and
        backward drops the module's packs, not the record's)."""
        for i in range(len(self.body) - 1, -1, -1):
            d = self.body[i].backward_hip(saved[i], d, post=(stem_act, pk['slope']) if i == 0 else None)
        return pk['stem_grad'].run(d, (int(stem_act.shape[2]), int(stem_act.shape[3])))

    def _forward_record(self, x, record):
        """Split-precision convolutions first; if any of them met an operand outside the fp16 range (flagged on the device) the
        forward is repeated on the exact fp32 kernels, as the encoders do (restyle_psp_encoders._forward_hip)."""
        from torch_utils.ops import plain_conv
        if self._packed is None:
            self._pack()
        plain_conv.reset_overflow(x.device)
        out = self._trunk_record(x, record)
        if plain_conv.precision != 'fp32' and plain_conv.overflowed(x.device):
            saved, plain_conv.precision = plain_conv.precision, 'fp32'
            try:
                out = self._trunk_record(x, record)
            finally:
                plain_conv.precision = saved
        return out

    def features_hip(self, x):
        """l2-normalised features [N,512] of x [N,3,112,112] (see `hip_supported`); the gradient reaches x alone."""
        if not self.hip_supported(x):
            raise RuntimeError('Backbone.features_hip: needs a CUDA float32 [N,3,112,112] batch, eval mode, input_size 112 and frozen parameters')
        return _BackboneFeatures.apply(x, self)

    def launches(self):
        """(forward, backward) counts of kernel-launching library calls of one `features_hip` (sg3_se_residual and its backward are
        one call, two kernels, each) without an overflow repeat."""
        proj = sum(1 for u in self.body if not isinstance(u.shortcut_layer, torch.nn.MaxPool2d))
        se = 1 if self.mode == 'ir_se' else 0
        n = len(self.body)
        return 1 + n * (2 + se) + proj, 1 + n * (2 + se) + proj


class _BackboneFeatures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, net):
        record = ctx.needs_input_grad[0]
        body, stem_act, saved = net._forward_record(x.contiguous(), record)
        pk = net._packed
        if not record:
            return l2_norm(torch.addmm(pk['head_b'], body.flatten(1), pk['head_w']))
        with torch.enable_grad():
            leaf = body.detach().requires_grad_(True)
            feats = l2_norm(torch.addmm(pk['head_b'], leaf.flatten(1), pk['head_w']))
        ctx.net, ctx.pk, ctx.stem_act, ctx.units, ctx.head = net, pk, stem_act, saved, (leaf, feats)
        return feats.detach()

    @staticmethod
    @once_differentiable
    def backward(ctx, dfeats):
        leaf, feats = ctx.head
        d = torch.autograd.grad(feats, leaf, dfeats.detach(), retain_graph=True)[0]       # the record lives as long as the outer graph does
        return ctx.net._trunk_backward(ctx.pk, ctx.stem_act, ctx.units, d), None


def IR_50(input_size):
    """Constructs a ir-50 model."""
    return Backbone(input_size, num_layers=50, mode='ir', drop_ratio=0.4, affine=False)


def IR_101(input_size):
    """Constructs a ir-101 model."""
    return Backbone(input_size, num_layers=100, mode='ir', drop_ratio=0.4, affine=False)


def IR_152(input_size):
    """Constructs a ir-152 model."""
    return Backbone(input_size, num_layers=152, mode='ir', drop_ratio=0.4, affine=False)


def IR_SE_50(input_size):
    """Constructs a ir_se-50 model."""
    return Backbone(input_size, num_layers=50, mode='ir_se', drop_ratio=0.4, affine=False)


def IR_SE_101(input_size):
    """Constructs a ir_se-101 model."""
    return Backbone(input_size, num_layers=100, mode='ir_se', drop_ratio=0.4, affine=False)


def IR_SE_152(input_size):
    """Constructs a ir_se-152 model."""
    return Backbone(input_size, num_layers=152, mode='ir_se', drop_ratio=0.4, affine=False)
