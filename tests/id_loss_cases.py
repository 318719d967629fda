"""Shared pieces of the identity-loss tests: synthetic IR-SE50 weights, smooth test images, the float64 restatement of the reference
loss, and the closed-form backward of one residual unit in plain torch.

No pretrained ArcFace weights exist offline; everything uses `synth_weights.synth_encoder_state_dict` on the Backbone's
key -> shape manifest, with `output_layer.3.weight` scaled by 1 / sqrt(fan_in) so that the features keep a usable spread.
Nothing here imports the package at module level: tests/golden/make_golden_id_loss.py uses these with the reference's Backbone."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from synth_weights import synth_encoder_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'id_loss.npz')
MANIFEST = os.path.join(HERE, 'golden', 'id_loss_manifest.json')

# the unit shapes of the closed-form check: (in_channel, depth, stride, H, W)
UNIT_SHAPES = [(64, 64, 1, 9, 13), (64, 64, 2, 13, 9), (64, 128, 2, 20, 24), (64, 128, 2, 7, 7)]


def manifest():
    with open(MANIFEST) as f:
        return {k: tuple(v) for k, v in json.load(f).items()}


def is_prelu_key(key):
    parts = key.split('.')
    return parts[-1] == 'weight' and parts[-2] == '2' and (parts[0] == 'input_layer' or parts[-3] == 'res_layer')


def state_dict(man, seed=0, negate=False):
    """{key: torch tensor}; negate: every third PReLU slope of every layer negative."""
    sd = synth_encoder_state_dict({k: list(v) for k, v in man.items()}, seed=seed)
    w = sd['output_layer.3.weight']
    sd['output_layer.3.weight'] = (w / np.sqrt(w.shape[1])).astype(np.float32)
    if negate:
        for k in sd:
            if is_prelu_key(k):
                sd[k] = sd[k].copy()
                sd[k][::3] *= -1
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def images(b, size, seed):
    """[b,3,size,size] float32 in (-1, 1): tanh of bilinearly upsampled noise."""
    r = np.random.RandomState(4000 + seed)
    z = torch.from_numpy(r.randn(b, 3, 8, 8).astype(np.float32))
    return torch.tanh(1.5 * F.interpolate(z, size=(size, size), mode='bilinear', align_corners=False)).contiguous()


def perturbed(x, seed, scale=0.05):
    r = np.random.RandomState(5000 + seed)
    z = torch.from_numpy(r.randn(x.shape[0], 3, 8, 8).astype(np.float32))
    return (x + scale * F.interpolate(z, size=tuple(x.shape[2:]), mode='bilinear', align_corners=False)).clamp(-1, 1).contiguous()


def extract_feats(net, x):
    """The reference's IDLoss.extract_feats around `net` (criteria/id_loss.py), in x's dtype."""
    if x.shape[2] != 256:
        x = F.adaptive_avg_pool2d(x, (256, 256))
    x = x[:, :, 35:223, 32:220]
    x = F.adaptive_avg_pool2d(x, (112, 112))
    return net(x)


def id_loss_reference(net, y_hat, y, x):
    """The reference's IDLoss.forward, restated (its file imports a module that does not exist) -> (loss, sim_improvement, logs,
    (x_feats, y_feats, y_hat_feats))."""
    n_samples = x.shape[0]
    x_feats = extract_feats(net, x)
    y_feats = extract_feats(net, y)
    y_hat_feats = extract_feats(net, y_hat)
    y_feats = y_feats.detach()
    loss = 0
    sim_improvement = 0
    id_logs = []
    count = 0
    for i in range(n_samples):
        diff_target = y_hat_feats[i].dot(y_feats[i])
        diff_input = y_hat_feats[i].dot(x_feats[i])
        diff_views = y_feats[i].dot(x_feats[i])
        id_logs.append({'diff_target': float(diff_target), 'diff_input': float(diff_input), 'diff_views': float(diff_views)})
        loss += 1 - diff_target
        sim_improvement += float(diff_target) - float(diff_views)
        count += 1
    return loss / count, sim_improvement / count, id_logs, (x_feats, y_feats, y_hat_feats)


def loss_and_grad(net, y_hat, y, x):
    """id_loss_reference plus d loss / d y_hat, everything detached."""
    y_hat = y_hat.detach().clone().requires_grad_(True)
    loss, sim, logs, feats = id_loss_reference(net, y_hat, y, x)
    grad, = torch.autograd.grad(loss, y_hat)
    return loss.detach(), sim, logs, tuple(f.detach() for f in feats), grad


def logs_array(logs):
    return np.array([[d['diff_target'], d['diff_input'], d['diff_views']] for d in logs], dtype=np.float64)


def build_backbone(device='cpu', dtype=torch.float32, negate=False, num_layers=50, mode='ir_se'):
    """The package's Backbone(112, ...) in eval mode with the synthetic weights, parameters frozen."""
    from models.setgan.encoder.encoders.model_irse import Backbone
    net = Backbone(112, num_layers, mode=mode, drop_ratio=0.6)
    man = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict(state_dict(man, negate=negate))
    return net.to(device=device, dtype=dtype).eval().requires_grad_(False)


def build_unit(in_channel, depth, stride, seed=0, negate=True, dtype=torch.float64, device='cpu', se=True):
    """One bottleneck_IR_SE (or bottleneck_IR) in eval mode with synthetic weights; negate: a third of its PReLU slopes negative."""
    from models.setgan.encoder.encoders.helpers import bottleneck_IR, bottleneck_IR_SE
    unit = (bottleneck_IR_SE if se else bottleneck_IR)(in_channel, depth, stride)
    man = {'body.0.' + k: list(v.shape) for k, v in unit.state_dict().items()}
    sd = synth_encoder_state_dict(man, seed=seed + 31 * stride + depth)
    sd = {k[len('body.0.'):]: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
    if negate:
        sd['res_layer.2.weight'][::3] *= -1
    unit.load_state_dict(sd)
    return unit.to(device=device, dtype=dtype).eval().requires_grad_(False)


def bn_affine(bn):
    a = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
    return a, bn.bias - bn.running_mean * a


def unit_backward_closed_form(unit, x, dout):
    """dx of one eval-mode bottleneck_IR_SE from dout, by the formulas the HIP backward implements (in x's dtype):
        dg = sum_hw dout res;  dz = dg g (1 - g);  dh = fc2^T dz;  du = dh [u > 0];  dm = fc1^T du;  dres = dout g + dm / (H W)
        dx = a1 * dgrad1(prelu'(pre) * dgrad2(dres; a2 w2, stride)) + shortcut path
    The PReLU branch is read from the PRE-activation: with a negative slope the output's sign does not tell it."""
    bn1, conv1, prelu, conv2, bn2 = (unit.res_layer[i] for i in range(5))
    a1, b1 = bn_affine(bn1)
    a2, b2 = bn_affine(bn2)
    s = unit.stride
    h, w = x.shape[2:]
    pre = F.conv2d(x * a1.view(1, -1, 1, 1) + b1.view(1, -1, 1, 1), conv1.weight, padding=1)
    slope = prelu.weight.view(1, -1, 1, 1)
    h1 = torch.where(pre > 0, pre, pre * slope)
    w2 = conv2.weight * a2.view(-1, 1, 1, 1)
    res = F.conv2d(h1, w2, b2, stride=s, padding=1)
    if len(unit.res_layer) > 5:
        se = unit.res_layer[5]
        fc1, fc2 = se.fc1.weight.flatten(1), se.fc2.weight.flatten(1)
        m = res.mean(dim=(2, 3))
        u = m @ fc1.t()
        g = torch.sigmoid(torch.relu(u) @ fc2.t())
        dg = (dout * res).sum(dim=(2, 3))
        dz = dg * g * (1 - g)
        dh = dz @ fc2
        du = dh * (u > 0).to(dh.dtype)
        dm = du @ fc1
        dres = dout * g.view(*g.shape, 1, 1) + (dm / (res.shape[2] * res.shape[3])).view(*dm.shape, 1, 1)
    else:
        dres = dout

    def dgrad(dy, weight, stride, pad):
        oh = (h + 2 * pad - weight.shape[2]) // stride + 1
        ow = (w + 2 * pad - weight.shape[3]) // stride + 1
        op = (h - ((oh - 1) * stride - 2 * pad + weight.shape[2]), w - ((ow - 1) * stride - 2 * pad + weight.shape[3]))
        return F.conv_transpose2d(dy, weight, stride=stride, padding=pad, output_padding=op)

    dh1 = dgrad(dres, w2, s, 1) * torch.where(pre > 0, torch.ones_like(pre), slope.expand_as(pre))
    dx = dgrad(dh1, conv1.weight, 1, 1) * a1.view(1, -1, 1, 1)
    if isinstance(unit.shortcut_layer, torch.nn.Sequential):
        sa, _ = bn_affine(unit.shortcut_layer[1])
        dx = dx + dgrad(dout, unit.shortcut_layer[0].weight * sa.view(-1, 1, 1, 1), s, 0)
    elif s == 1:
        dx = dx + dout
    else:
        sc = torch.zeros_like(dx)
        sc[:, :, ::s, ::s] = dout
        dx = dx + sc
    return dx
