"""IR / IR-SE residual units of the ReStyle encoder backbone (ArcFace-style ResNet), module-for-module compatible
with the reference so its checkpoints load (reference models/setgan/encoder/encoders/helpers.py: get_blocks :30-55,
SEModule :57-73, bottleneck_IR :76-95, bottleneck_IR_SE :98-120).

`forward()` is the plain PyTorch definition (used on CPU and, by default, for training); on a GPU in eval mode the owning encoder
calls `forward_hip()`, which runs the two 3x3 convolutions on the matrix cores with their element-wise neighbours
fused (torch_utils/ops/plain_conv.py): BN1 as an input affine of conv1, PReLU as its epilogue, BN2 folded into conv2.
With the encoder's `native_training` switch on, train mode runs `forward_train_record()` / `backward_train()`: batch statistics,
and gradients for the input and every parameter from libsg3hip.
"""
import os
from collections import namedtuple

import torch
from torch.nn import AdaptiveAvgPool2d, BatchNorm2d, Conv2d, MaxPool2d, Module, PReLU, ReLU, Sequential, Sigmoid


class Flatten(Module):
    def forward(self, input):  # pylint: disable=redefined-builtin
        return input.view(input.size(0), -1)


def l2_norm(input, axis=1):  # pylint: disable=redefined-builtin
    return torch.div(input, torch.norm(input, 2, axis, True))


class Bottleneck(namedtuple('Block', ['in_channel', 'depth', 'stride'])):
    """One residual unit: input channels, output channels, stride of its second convolution."""


def get_block(in_channel, depth, num_units, stride=2):
    return [Bottleneck(in_channel, depth, stride)] + [Bottleneck(depth, depth, 1) for _ in range(num_units - 1)]


_STAGES = {50: (3, 4, 14, 3), 100: (3, 13, 30, 3), 152: (3, 8, 36, 3)}


def get_blocks(num_layers):
    if num_layers not in _STAGES:
        raise ValueError(f"Invalid number of layers: {num_layers}. Must be one of [50, 100, 152]")
    units = _STAGES[num_layers]
    widths = [(64, 64), (64, 128), (128, 256), (256, 512)]
    return [get_block(in_channel=i, depth=d, num_units=u) for (i, d), u in zip(widths, units)]


# GPU inference runs the squeeze-and-excitation tail on two HIP kernels unless SG3_SE_TORCH=1 (A/B timing)
_SE_KERNELS = os.environ.get('SG3_SE_TORCH', '0') != '1'


class SEModule(Module):
    """Squeeze-and-excitation: x * sigmoid(fc2(relu(fc1(mean_hw(x)))))."""

    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = AdaptiveAvgPool2d(1)
        self.fc1 = Conv2d(channels, channels // reduction, kernel_size=1, padding=0, bias=False)
        self.relu = ReLU(inplace=True)
        self.fc2 = Conv2d(channels // reduction, channels, kernel_size=1, padding=0, bias=False)
        self.sigmoid = Sigmoid()

    def gate(self, x):
        # the two 1x1 convolutions act on a [N,C,1,1] tensor: plain matrix products
        m = x.mean(dim=(2, 3))
        m = torch.relu(m @ self.fc1.weight.flatten(1).t())
        return torch.sigmoid(m @ self.fc2.weight.flatten(1).t()).unsqueeze(-1).unsqueeze(-1)

    def forward(self, x):
        return x * self.gate(x)


class _ResidualUnit(Module):
    use_se = False

    def __init__(self, in_channel, depth, stride):
        super().__init__()
        self.stride = stride
        if in_channel == depth:
            self.shortcut_layer = MaxPool2d(1, stride)
        else:
            self.shortcut_layer = Sequential(Conv2d(in_channel, depth, (1, 1), stride, bias=False), BatchNorm2d(depth))
        layers = [BatchNorm2d(in_channel),
                  Conv2d(in_channel, depth, (3, 3), (1, 1), 1, bias=False), PReLU(depth),
                  Conv2d(depth, depth, (3, 3), stride, 1, bias=False), BatchNorm2d(depth)]
        if self.use_se:
            layers.append(SEModule(depth, 16))
        self.res_layer = Sequential(*layers)
        self._packed = None
        self._train_packed = None

    def forward(self, x):
        return self.res_layer(x) + self.shortcut_layer(x)

    # ---- fused eval-mode path on libsg3hip ----
    def _pack(self):
        from torch_utils.ops.plain_conv import ACT_NONE, ACT_PRELU, PackedConv, bn_affine
        bn1, conv1, prelu, conv2, bn2 = (self.res_layer[i] for i in range(5))
        a1, b1 = bn_affine(bn1)
        a2, b2 = bn_affine(bn2)
        pk = dict(conv1=PackedConv(conv1.weight, in_scale=a1, in_shift=b1, act=ACT_PRELU, slope=prelu.weight, stride=1, padding=1),
                  conv2=PackedConv(conv2.weight, out_scale=a2, bias=b2, act=ACT_NONE, stride=self.stride, padding=1))
        if isinstance(self.shortcut_layer, Sequential):
            sc, sbn = self.shortcut_layer[0], self.shortcut_layer[1]
            a, b = bn_affine(sbn)
            pk['shortcut'] = PackedConv(sc.weight, out_scale=a, bias=b, act=ACT_NONE, stride=self.stride, padding=0)
        self._packed = pk

    def forward_hip(self, x):
        if self._packed is None:
            self._pack()
        pk = self._packed
        res = pk['conv2'](pk['conv1'](x))
        if 'shortcut' in pk:
            shortcut = pk['shortcut'](x)
        else:
            shortcut = x if self.stride == 1 else x[:, :, ::self.stride, ::self.stride]
        if self.use_se:
            se = self.res_layer[5]
            if res.is_cuda and res.dtype == torch.float32 and not torch.is_grad_enabled() and _SE_KERNELS:
                from torch_utils.ops import se_ops
                return se_ops.se_residual(res.contiguous(), shortcut, se.fc1.weight, se.fc2.weight)      # two launches
            return torch.addcmul(shortcut, res, se.gate(res))
        return res + shortcut

    # ---- the same path differentiated with respect to the input (frozen weights: the identity loss) ----
    def _grad_pack(self):
        """Transposed weights for the data gradient (torch_utils/ops/plain_conv_grad.py), kept inside `_packed` so that whatever
        invalidates the forward pack drops these too.  BN2 and the shortcut's BatchNorm scale dy's channels, BN1 the result's."""
        if self._packed is None:
            self._pack()
        pk = self._packed
        if 'grad' not in pk:
            from torch_utils.ops.plain_conv import ACT_NONE, PackedConv, bn_affine
            from torch_utils.ops.plain_conv_grad import PackedDgrad
            bn1, conv1, prelu, conv2, bn2 = (self.res_layer[i] for i in range(5))
            a1, b1 = bn_affine(bn1)
            a2, _ = bn_affine(bn2)
            gk = dict(conv1=PackedDgrad(conv1.weight, out_scale=a1, stride=1), conv2=PackedDgrad(conv2.weight, k_scale=a2, stride=self.stride))
            if isinstance(self.shortcut_layer, Sequential):
                a, _ = bn_affine(self.shortcut_layer[1])
                gk['shortcut'] = PackedDgrad(self.shortcut_layer[0].weight, k_scale=a, stride=self.stride)
            # A PReLU output tells the branch its input took only while no slope is negative (decided here, once per pack); a layer
            # with a negative slope keeps its pre-activation instead: conv1 without the epilogue, then one PReLU
            gk['mixed'] = bool((prelu.weight.detach() < 0).any())
            if gk['mixed']:
                gk['conv1_linear'] = PackedConv(conv1.weight, in_scale=a1, in_shift=b1, act=ACT_NONE, stride=1, padding=1)
            gk['slope'] = prelu.weight.detach().to(torch.float32).contiguous()
            pk['grad'] = gk
        return pk['grad']

    def forward_hip_record(self, x):
        """`forward_hip` keeping what `backward_hip` needs (the packed gradient weights included, so that a repack between forward
        and backward cannot change them) -> (out, saved).  At most four launches, five with a projection."""
        gk = self._grad_pack()
        pk = self._packed
        if gk['mixed']:
            act = gk['conv1_linear'](x)
            h1 = torch.nn.functional.prelu(act, gk['slope'])
        else:
            act = h1 = pk['conv1'](x)
        res = pk['conv2'](h1)
        if 'shortcut' in pk:
            shortcut = pk['shortcut'](x)
        else:
            shortcut = x if self.stride == 1 else x[:, :, ::self.stride, ::self.stride]
        mean = None
        if self.use_se:
            from torch_utils.ops import se_ops
            se = self.res_layer[5]
            out, mean = se_ops.se_residual_record(res, shortcut, se.fc1.weight, se.fc2.weight)
        else:
            out = res + shortcut
        return out, (act, res, mean, (int(x.shape[2]), int(x.shape[3])), gk)

    def backward_hip(self, saved, dout, post=None):
        """Gradient of `forward_hip_record` with respect to x:
            dx = a1 * dgrad1(prelu' * dgrad2(dres; a2 w2, stride)) + shortcut path,   dres from the SE backward (or dout itself).
        `post` = (act, slope) multiplies dx by the derivative of a PReLU in front of the unit (the stem's).  At most six launches,
        seven with a projection."""
        act, res, mean, (h, w), gk = saved                   # gk: the transposed weights the forward's pack belongs to
        identity_s2 = 'shortcut' not in gk and self.stride != 1
        dsc = None
        if self.use_se:
            from torch_utils.ops import se_ops
            se = self.res_layer[5]
            dres, dsc = se_ops.se_residual_bwd(dout, res, mean, se.fc1.weight, se.fc2.weight, scatter_hw=(h, w) if identity_s2 else None)
        else:
            dres = dout
            if identity_s2:
                dsc = dout.new_zeros([dout.shape[0], dout.shape[1], h, w])
                dsc[:, :, ::self.stride, ::self.stride] = dout
        dh1 = gk['conv2'].run(dres, (h, w), act=act, slope=gk['slope'])
        if 'shortcut' in gk:
            addend = gk['shortcut'].run(dout, (h, w))
        else:
            addend = dsc if identity_s2 else dout
        if post is None:
            return gk['conv1'].run(dh1, (h, w), addend=addend)
        return gk['conv1'].run(dh1, (h, w), addend=addend, act=post[0], slope=post[1])

    # ---- train mode: batch statistics, and gradients for the input and every parameter ----
    def _train_packs(self):
        """Forward and transposed weights of the unit's convolutions with nothing folded in (in training the BatchNorms are the batch's),
        keyed on (data_ptr, _version) of the weights: rebuilt after an optimizer step, kept between the iterations of one step."""
        convs = [self.res_layer[1], self.res_layer[3]] + ([self.shortcut_layer[0]] if isinstance(self.shortcut_layer, Sequential) else [])
        key = tuple((c.weight.data_ptr(), c.weight._version) for c in convs)
        tp = getattr(self, '_train_packed', None)
        if tp is None or tp['key'] != key:
            from torch_utils.ops.plain_conv import ACT_NONE, PackedConv
            from torch_utils.ops.plain_conv_grad import PackedDgrad
            dev, depth = convs[0].weight.device, int(convs[0].weight.shape[0])
            tp = dict(key=key, one=torch.ones([depth], device=dev), zero=torch.zeros([depth], device=dev),
                      conv1=PackedConv(convs[0].weight, act=ACT_NONE, stride=1, padding=1, chains=True), dgrad1=PackedDgrad(convs[0].weight, stride=1),
                      conv2=PackedConv(convs[1].weight, act=ACT_NONE, stride=self.stride, padding=1, chains=True), dgrad2=PackedDgrad(convs[1].weight, stride=self.stride))
            if len(convs) == 3:
                tp['shortcut'] = PackedConv(convs[2].weight, act=ACT_NONE, stride=self.stride, padding=0, chains=True)
                tp['dshortcut'] = PackedDgrad(convs[2].weight, stride=self.stride)
            self._train_packed = tp
        return tp

    def forward_train_record(self, x, stats_out=None):
        """`forward` in train mode on libsg3hip, keeping what `backward_train` needs -> (out, saved):
            BN1 statistics; conv1 with the batch's affine fused, raw; PReLU; conv2, raw; BN2 statistics and apply;
            the shortcut (projection: 1x1 convolution, BatchNorm statistics and apply); the squeeze-and-excitation tail (IR: one add).
        Seven ABI calls for IR-SE (six for IR), three more with a projection, once the packs exist.  The convolutions follow
        `plain_conv.precision` ('fp32' takes the four-chain form); the split-precision overflow flag is the CALLER's to reset, read and
        answer with a repeat under 'fp32' (`BackboneEncoder._trunk_train_forward` does so for the whole trunk: one flag read per
        forward, not one per unit).  The running statistics are NOT touched: every (BatchNorm2d, Stats) pair is appended to `stats_out`, and the caller applies them once its forward is accepted
        (torch_utils/ops/batchnorm_train.update_running)."""
        from torch_utils.ops import batchnorm_train as bt
        tp = self._train_packs()
        bn1, _, prelu, _, bn2 = (self.res_layer[i] for i in range(5))
        x = x.contiguous()
        st1 = bt.stats(x, bn1.weight, bn1.bias, bn1.eps)
        pre = tp['conv1'].run(x, in_scale=st1.a, in_shift=st1.b)
        h1 = bt.apply(pre, tp['one'], tp['zero'], slope=prelu.weight)
        c2 = tp['conv2'].run(h1)
        st2 = bt.stats(c2, bn2.weight, bn2.bias, bn2.eps)
        res = bt.apply(c2, st2.a, bn2.bias, centre=st2.mean, centre_lo=st2.mean_lo)
        pairs = [(bn1, st1), (bn2, st2)]
        sc_raw = st_s = None
        if 'shortcut' in tp:
            sbn = self.shortcut_layer[1]
            sc_raw = tp['shortcut'].run(x)
            st_s = bt.stats(sc_raw, sbn.weight, sbn.bias, sbn.eps)
            shortcut = bt.apply(sc_raw, st_s.a, sbn.bias, centre=st_s.mean, centre_lo=st_s.mean_lo)
            pairs.append((sbn, st_s))
        else:
            shortcut = x if self.stride == 1 else x[:, :, ::self.stride, ::self.stride]
        mean = None
        if self.use_se:
            from torch_utils.ops import se_ops
            se = self.res_layer[5]
            out, mean = se_ops.se_residual_record(res, shortcut, se.fc1.weight, se.fc2.weight)
        else:
            out = res + shortcut
        if stats_out is not None:
            stats_out.extend(pairs)
        return out, (x, st1, pre, h1, c2, st2, res, mean, sc_raw, st_s, prelu.weight.detach().to(torch.float32).contiguous(), tp)

    def backward_train(self, saved, dout, post=None):
        """Gradient of `forward_train_record` -> (dx, grads), grads keyed like `named_parameters()`:
            the squeeze-and-excitation backward (its dg and the saved mean give dfc1 / dfc2 as small matrix products); BN2 backward
            (sums, then the pass); wgrad2; dgrad2; the slope gradient, whose launch also applies the PReLU derivative (from the saved
            PRE-activation: a slope may be zero); wgrad1 with the BN1 affine fused; dgrad1; BN1 backward with the shortcut path's
            gradient as the addend; with a projection its BatchNorm backward, wgrad and dgrad.
        `post` = (act, slope): dx is multiplied by the derivative of a PReLU in front of the unit (the stem's) and returned as
        (dx, dx before that mask).  Ten ABI calls for IR-SE (nine for IR), four more with a projection; not counted: the torch
        operations of `se_ops.se_weight_grads` (the gate recomputed from the saved mean, then the two matrix products) and, for IR with a
        stride-2 identity shortcut, torch's zero-fill and strided copy.  dbeta / dgamma of one BatchNorm are two rows of one [2,C]
        tensor: independent values, one storage (autograd copies them into `.grad`; clone before editing one in place)."""
        from torch_utils.ops import batchnorm_train as bt
        from torch_utils.ops.plain_conv_wgrad import wgrad
        x, st1, pre, h1, c2, st2, res, mean, sc_raw, st_s, slope, tp = saved
        h, w = int(x.shape[2]), int(x.shape[3])
        identity_s2 = 'shortcut' not in tp and self.stride != 1
        dout = dout.contiguous()
        g = {}
        dsc = None
        if self.use_se:
            from torch_utils.ops import se_ops
            se = self.res_layer[5]
            dres, dsc, dg = se_ops.se_residual_bwd_train(dout, res, mean, se.fc1.weight, se.fc2.weight, scatter_hw=(h, w) if identity_s2 else None)
            g['res_layer.5.fc1.weight'], g['res_layer.5.fc2.weight'] = se_ops.se_weight_grads(dg, mean, se.fc1.weight, se.fc2.weight)
        else:
            dres = dout
            if identity_s2:
                dsc = dout.new_zeros([dout.shape[0], dout.shape[1], h, w])
                dsc[:, :, ::self.stride, ::self.stride] = dout
        g['res_layer.4.bias'], g['res_layer.4.weight'] = bt.backward_reduce(dres, c2, st2)
        dc2 = bt.backward_apply(dres, c2, st2, g['res_layer.4.bias'], g['res_layer.4.weight'])
        g['res_layer.3.weight'] = wgrad(h1, dc2, 3, self.stride)
        dh1 = tp['dgrad2'].run(dc2, (h, w))
        g['res_layer.2.weight'], dpre = bt.slope_grad(dh1, pre, slope)
        g['res_layer.1.weight'] = wgrad(x, dpre, 3, 1, in_scale=st1.a, in_shift=st1.b)
        dxt = tp['dgrad1'].run(dpre, (h, w))
        if 'shortcut' in tp:
            g['shortcut_layer.1.bias'], g['shortcut_layer.1.weight'] = bt.backward_reduce(dout, sc_raw, st_s)
            dsr = bt.backward_apply(dout, sc_raw, st_s, g['shortcut_layer.1.bias'], g['shortcut_layer.1.weight'])
            g['shortcut_layer.0.weight'] = wgrad(x, dsr, 1, self.stride)
            addend = tp['dshortcut'].run(dsr, (h, w))
        else:
            addend = dsc if identity_s2 else dout
        g['res_layer.0.bias'], g['res_layer.0.weight'] = bt.backward_reduce(dxt, x, st1)
        if post is None:
            return bt.backward_apply(dxt, x, st1, g['res_layer.0.bias'], g['res_layer.0.weight'], addend=addend), g
        return bt.backward_apply(dxt, x, st1, g['res_layer.0.bias'], g['res_layer.0.weight'], addend=addend, act=post[0], slope=post[1], want_raw=True), g


class bottleneck_IR(_ResidualUnit):  # noqa: N801  (reference class name)
    use_se = False


class bottleneck_IR_SE(_ResidualUnit):  # noqa: N801  (reference class name)
    use_se = True


class BasicBlock(Module):
    """ResNet18/34 residual block with torchvision's module names (`conv1 bn1 relu conv2 bn2 downsample`), so the `body.*` keys
    of a ReStyle ResNetBackboneEncoder checkpoint (reference restyle_psp_encoders.py:65-77 flattens resnet34's layer1..4)
    load: y = relu(bn2(conv2(relu(bn1(conv1(x))))) + (downsample(x) | x)); conv1 carries the stride."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1):
        super().__init__()
        self.conv1 = Conv2d(inplanes, planes, (3, 3), stride, 1, bias=False)
        self.bn1 = BatchNorm2d(planes)
        self.relu = ReLU(inplace=True)
        self.conv2 = Conv2d(planes, planes, (3, 3), 1, 1, bias=False)
        self.bn2 = BatchNorm2d(planes)
        self.downsample = None
        if stride != 1 or inplanes != planes:
            self.downsample = Sequential(Conv2d(inplanes, planes, (1, 1), stride, bias=False), BatchNorm2d(planes))
        self.stride = stride
        self._packed = None

    def forward(self, x):
        out = self.bn2(self.conv2(self.relu(self.bn1(self.conv1(x)))))
        return self.relu(out + (x if self.downsample is None else self.downsample(x)))

    def _pack(self):
        from torch_utils.ops.plain_conv import ACT_LRELU, ACT_NONE, PackedConv, bn_affine
        a1, b1 = bn_affine(self.bn1)
        a2, b2 = bn_affine(self.bn2)
        zero = torch.zeros([1], device=self.conv1.weight.device)            # ReLU = leaky ReLU with slope 0 in the epilogue
        pk = dict(conv1=PackedConv(self.conv1.weight, out_scale=a1, bias=b1, act=ACT_LRELU, slope=zero, stride=self.stride, padding=1),
                  conv2=PackedConv(self.conv2.weight, out_scale=a2, bias=b2, act=ACT_NONE, stride=1, padding=1))
        if self.downsample is not None:
            a, b = bn_affine(self.downsample[1])
            pk['shortcut'] = PackedConv(self.downsample[0].weight, out_scale=a, bias=b, act=ACT_NONE, stride=self.stride, padding=0)
        self._packed = pk

    def forward_hip(self, x):
        if self._packed is None:
            self._pack()
        pk = self._packed
        res = pk['conv2'](pk['conv1'](x))
        return torch.relu_(res.add_(pk['shortcut'](x) if 'shortcut' in pk else x))


def resnet34_blocks():
    """The 16 BasicBlocks of torchvision.models.resnet34's layer1..layer4 in order (3, 4, 6, 3 blocks of 64, 128, 256, 512
    channels; the first block of layers 2..4 has stride 2 and a 1x1 projection shortcut)."""
    blocks, inplanes = [], 64
    for planes, count, stride in ((64, 3, 1), (128, 4, 2), (256, 6, 2), (512, 3, 2)):
        for i in range(count):
            blocks.append(BasicBlock(inplanes, planes, stride if i == 0 else 1))
            inplanes = planes
    return blocks
