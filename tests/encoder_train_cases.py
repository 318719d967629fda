"""Shared reference code of the encoder-training tests (test_encoder_train_cpu.py, test_gpu_encoder_train.py): the weight-gradient
shapes and their float64 reference, the K-split cover of the host planner, seeded residual units, and the unit's training backward
restated in plain tensor algebra (any dtype; the CPU test runs it in float64 against autograd)."""
import numpy as np
import torch
import torch.nn.functional as F

# (k, stride, I, O, H, W): every (k, stride) form, channel counts that are no multiple of the 64 x 64 tile (and one above it), rows
# wider than one 32- (stride 1) or 16-pixel (stride 2) chunk with a ragged last chunk, maps smaller than one chunk; then, per
# (k, stride), more than 256 (o, i) tiles: the planner gives those ONE split (no partials, no reduce launch), which a batch of two
# samples reaches in no other way (tests/test_conv2d_dispatch_cpu.py checks which kernels and how many splits this list reaches)
WGRAD_SHAPES = [(3, 1, 64, 64, 9, 13), (3, 1, 6, 64, 12, 12), (3, 1, 40, 20, 5, 70), (3, 2, 64, 64, 13, 9), (3, 2, 128, 128, 7, 7),
                (3, 2, 40, 20, 7, 131), (1, 2, 64, 128, 13, 9), (1, 2, 70, 20, 6, 67), (1, 1, 40, 20, 5, 70), (3, 2, 3, 20, 7, 35),
                (3, 1, 1, 16448, 1, 12), (3, 2, 1, 16448, 1, 24), (1, 1, 1, 16448, 1, 12), (1, 2, 1, 16448, 1, 24)]


def out_hw(h, w, k, stride):
    pad = k // 2
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def randn(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape))           # float64, CPU


def wgrad64(x, dy, k, stride):
    """Weight gradient of conv2d(x, w, stride, padding k // 2) summed over the batch, in the dtype of its arguments."""
    return torch.nn.grad.conv2d_weight(x, (dy.shape[1], x.shape[1], k, k), dy, stride=stride, padding=k // 2)


def padded_affine(x, a, b):
    """a x + b on the pixels; what the convolution's zero padding sees stays zero because padding is applied after this."""
    return x * a.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def split_cover(n, h, w, k, stride, n_split, chunks_per_split, x_segs):
    """How often the planner's splits visit each (sample, output row, output column): an int array [n, OH, OW]."""
    oh, ow = out_hw(h, w, k, stride)
    px = 32 // stride
    n_chunks = n * oh * x_segs
    count = np.zeros([n, oh, ow], dtype=np.int64)
    for j in range(n_split):
        for c in range(j * chunks_per_split, min((j + 1) * chunks_per_split, n_chunks)):
            xs, t = c % x_segs, c // x_segs
            count[t // oh, t % oh, px * xs:min(ow, px * xs + px)] += 1
    return count


# ---- residual units ------------------------------------------------------------------------------------------------------------------

def make_unit(kind, in_channel, depth, stride, seed, negative_slopes=False, se_gain=4.0):
    """A seeded `bottleneck_IR` / `bottleneck_IR_SE` in float64 on the CPU with non-trivial BatchNorm affines and PReLU slopes.  The
    squeeze-and-excitation weights are scaled up so that the hidden ReLU is alive; `negative_slopes`: every third slope is
    negative or zero."""
    from models.setgan.encoder.encoders.helpers import bottleneck_IR, bottleneck_IR_SE
    torch.manual_seed(seed)
    unit = (bottleneck_IR_SE if kind == 'ir_se' else bottleneck_IR)(in_channel, depth, stride).double()
    r = np.random.RandomState(seed + 1)
    with torch.no_grad():
        for m in unit.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.from_numpy(1 + 0.3 * r.randn(m.num_features)))
                m.bias.copy_(torch.from_numpy(0.2 * r.randn(m.num_features)))
            elif isinstance(m, torch.nn.PReLU):
                s = 0.25 + 0.1 * r.randn(m.num_parameters)
                if negative_slopes:
                    s[0::6] = 0.0
                    s[3::6] = -np.abs(s[3::6]) - 0.05
                m.weight.copy_(torch.from_numpy(s))
        if unit.use_se:
            se = unit.res_layer[5]
            se.fc1.weight.mul_(se_gain)
            se.fc2.weight.mul_(se_gain)
    return unit.train()


def bn_backward(dy, x, weight, eps):
    """Training-mode BatchNorm2d backward in closed form -> (dx, dgamma, dbeta)."""
    m = x.shape[0] * x.shape[2] * x.shape[3]
    mean = x.mean(dim=(0, 2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    invstd = (var + eps) ** -0.5
    xhat = (x - mean) * invstd
    dbeta = dy.sum(dim=(0, 2, 3))
    dgamma = (dy * xhat).sum(dim=(0, 2, 3))
    dx = weight.view(1, -1, 1, 1) * invstd * (dy - dbeta.view(1, -1, 1, 1) / m - xhat * dgamma.view(1, -1, 1, 1) / m)
    return dx, dgamma, dbeta


def bn_forward(x, bn):
    mean = x.mean(dim=(0, 2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
    return (x - mean) * (var + bn.eps) ** -0.5 * bn.weight.view(1, -1, 1, 1) + bn.bias.view(1, -1, 1, 1)


def unit_train_algebra(unit, x, dout):
    """Forward and backward of a residual unit in train mode, spelled out the way `_ResidualUnit.backward_train` computes them (no
    autograd) -> (out, dx, {parameter name: gradient}).  The running statistics are not touched."""
    bn1, conv1, prelu, conv2, bn2 = (unit.res_layer[i] for i in range(5))
    s = unit.stride
    # forward
    xt = bn_forward(x, bn1)
    pre = F.conv2d(xt, conv1.weight, padding=1)
    h1 = torch.where(pre > 0, pre, pre * prelu.weight.view(1, -1, 1, 1))
    c2 = F.conv2d(h1, conv2.weight, stride=s, padding=1)
    res = bn_forward(c2, bn2)
    proj = isinstance(unit.shortcut_layer, torch.nn.Sequential)
    if proj:
        sconv, sbn = unit.shortcut_layer[0], unit.shortcut_layer[1]
        sc_raw = F.conv2d(x, sconv.weight, stride=s)
        shortcut = bn_forward(sc_raw, sbn)
    else:
        shortcut = x[:, :, ::s, ::s]
    grads = {}
    if unit.use_se:
        se = unit.res_layer[5]
        w1, w2 = se.fc1.weight.flatten(1), se.fc2.weight.flatten(1)
        m = res.mean(dim=(2, 3))
        u_pre = m @ w1.t()
        u = torch.relu(u_pre)
        g = torch.sigmoid(u @ w2.t())
        out = shortcut + res * g.unsqueeze(-1).unsqueeze(-1)
        # backward of the gate
        dg = (dout * res).sum(dim=(2, 3))
        dz = dg * g * (1 - g)
        grads['res_layer.5.fc2.weight'] = (dz.t() @ u).view_as(se.fc2.weight)
        du = (dz @ w2) * (u_pre > 0)
        grads['res_layer.5.fc1.weight'] = (du.t() @ m).view_as(se.fc1.weight)
        dres = dout * g.unsqueeze(-1).unsqueeze(-1) + ((du @ w1) / (res.shape[2] * res.shape[3])).unsqueeze(-1).unsqueeze(-1)
    else:
        out = shortcut + res
        dres = dout
    dc2, grads['res_layer.4.weight'], grads['res_layer.4.bias'] = bn_backward(dres, c2, bn2.weight, bn2.eps)
    grads['res_layer.3.weight'] = wgrad64(h1, dc2, 3, s)
    dh1 = torch.nn.grad.conv2d_input(h1.shape, conv2.weight, dc2, stride=s, padding=1)
    grads['res_layer.2.weight'] = (dh1 * pre.clamp(max=0)).sum(dim=(0, 2, 3))
    dpre = torch.where(pre > 0, dh1, dh1 * prelu.weight.view(1, -1, 1, 1))
    grads['res_layer.1.weight'] = wgrad64(xt, dpre, 3, 1)
    dxt = torch.nn.grad.conv2d_input(xt.shape, conv1.weight, dpre, padding=1)
    dx, grads['res_layer.0.weight'], grads['res_layer.0.bias'] = bn_backward(dxt, x, bn1.weight, bn1.eps)
    if proj:
        dsc, grads['shortcut_layer.1.weight'], grads['shortcut_layer.1.bias'] = bn_backward(dout, sc_raw, sbn.weight, sbn.eps)
        grads['shortcut_layer.0.weight'] = wgrad64(x, dsc, 1, s)
        dx = dx + torch.nn.grad.conv2d_input(x.shape, sconv.weight, dsc, stride=s)
    else:
        scat = torch.zeros_like(x)
        scat[:, :, ::s, ::s] = dout
        dx = dx + scat
    return out, dx, grads


def unit_autograd(unit, x, dout):
    """The same three results from autograd through `unit.forward` (train mode; the running statistics are restored afterwards)."""
    state = {k: v.clone() for k, v in unit.state_dict().items()}
    xr = x.detach().clone().requires_grad_(True)
    params = dict(unit.named_parameters())
    out = unit(xr)
    gs = torch.autograd.grad(out, [xr] + list(params.values()), dout)
    unit.load_state_dict(state)
    return out.detach(), gs[0], dict(zip(params.keys(), gs[1:]))


# ---- the whole trunk -----------------------------------------------------------------------------------------------------------------

def make_encoder(seed, n_styles=2, se_gain=4.0):
    """`BackboneEncoder(50, 'ir_se')` in float64 on the CPU, train mode: default (seeded) convolution weights, seeded non-trivial
    BatchNorm affines and PReLU slopes in the trunk, squeeze-and-excitation weights scaled by `se_gain`."""
    from models.setgan.encoder.encoders.helpers import SEModule
    from models.setgan.encoder.encoders.restyle_psp_encoders import BackboneEncoder
    torch.manual_seed(seed)
    enc = BackboneEncoder(50, 'ir_se', n_styles=n_styles).double()
    r = np.random.RandomState(seed + 1)
    with torch.no_grad():
        for part in (enc.input_layer, enc.body):
            for m in part.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.weight.copy_(torch.from_numpy(1 + 0.2 * r.randn(m.num_features)))
                    m.bias.copy_(torch.from_numpy(0.1 * r.randn(m.num_features)))
                elif isinstance(m, torch.nn.PReLU):
                    m.weight.copy_(torch.from_numpy(0.25 + 0.05 * r.randn(m.num_parameters)))
                elif isinstance(m, SEModule):
                    m.fc1.weight.mul_(se_gain)
                    m.fc2.weight.mul_(se_gain)
    return enc.train()


def se_hidden_alive(enc, x):
    """One bool per residual unit: does any hidden unit of its squeeze-and-excitation gate pass the ReLU for this batch?  Runs
    `_forward_torch` on a copy of the state (the running statistics are restored)."""
    from models.setgan.encoder.encoders.helpers import SEModule
    state = {k: v.clone() for k, v in enc.state_dict().items()}
    alive, hooks = [], []
    for m in enc.body.modules():
        if isinstance(m, SEModule):
            hooks.append(m.register_forward_hook(
                lambda mod, inp, out: alive.append(bool(((inp[0].mean(dim=(2, 3)) @ mod.fc1.weight.flatten(1).t()) > 0).any()))))
    with torch.no_grad():
        enc._trunk_torch(x)
    for h in hooks:
        h.remove()
    enc.load_state_dict(state)
    return alive


def trunk_named_parameters(enc):
    return [(f'{prefix}.{n}', p) for prefix in ('input_layer', 'body') for n, p in getattr(enc, prefix).named_parameters()]
