"""Shared pieces of the LPIPS tests: synthetic AlexNet / linear-layer weights drawn from a seed against the key -> shape manifest
(He-scaled, small biases; never stored), smooth test images, the reference's forward restated around a feature network and its
linear layers, float64 helpers.

No pretrained weights exist offline.  Nothing here imports the package at module level: tests/golden/make_golden_lpips.py uses
these with the reference's AlexNet / LinLayers."""
import json
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'lpips.npz')
MANIFEST = os.path.join(HERE, 'golden', 'lpips_manifest.json')

MEAN = [-.030, -.088, -.188]
STD = [.458, .448, .450]
CONV_INDICES = (0, 3, 6, 8, 10)
CHANNELS = (64, 192, 384, 256, 256)
# golden cases: name -> (N, H, W)
CASES = {'s64': (2, 64, 64), 's70x93': (1, 70, 93)}


def manifest():
    with open(MANIFEST) as f:
        return OrderedDict((k, tuple(v)) for k, v in json.load(f).items())


def state_dict(man=None, seed=0):
    """{key: float32 tensor} for LPIPS.state_dict(): He-scaled convolution weights, biases of 0.05 sigma, non-negative linear
    layers of mean ~1/C (the published ones are non-negative too), the reference's mean / std."""
    man = manifest() if man is None else man
    r = np.random.RandomState(9000 + seed)
    sd = OrderedDict()
    for key, shape in man.items():
        if key == 'net.mean':
            v = np.asarray(MEAN, dtype=np.float32).reshape(shape)
        elif key == 'net.std':
            v = np.asarray(STD, dtype=np.float32).reshape(shape)
        elif key.startswith('lin.'):
            v = np.abs(r.randn(*shape)) / shape[1]
        elif key.endswith('.weight'):
            v = r.randn(*shape) * np.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        else:
            v = 0.05 * r.randn(*shape)
        sd[key] = torch.from_numpy(np.asarray(v, dtype=np.float32))
    return sd


def upstream_dicts(sd):
    """(torchvision-style AlexNet state dict with `features.N.*` and some `classifier.*`, published-style `lin{k}.model.1.weight`)."""
    alex = OrderedDict((k.replace('net.layers.', 'features.'), v) for k, v in sd.items() if k.startswith('net.layers.'))
    alex['classifier.1.weight'] = torch.zeros(4, 4)
    alex['classifier.1.bias'] = torch.zeros(4)
    lin = OrderedDict((f'lin{k.split(".")[1]}.model.1.weight', v) for k, v in sd.items() if k.startswith('lin.'))
    return alex, lin


def images(n, h, w, seed):
    """[n,3,h,w] float32 in (-1, 1): tanh of bilinearly upsampled noise plus a little fine grain."""
    r = np.random.RandomState(4000 + seed)
    z = torch.from_numpy(r.randn(n, 3, 8, 8).astype(np.float32))
    fine = torch.from_numpy(r.randn(n, 3, h, w).astype(np.float32))
    return torch.tanh(1.5 * F.interpolate(z, size=(h, w), mode='bilinear', align_corners=False) + 0.1 * fine).contiguous()


def perturbed(x, seed, scale=0.4):
    r = np.random.RandomState(5000 + seed)
    z = torch.from_numpy(r.randn(x.shape[0], 3, 8, 8).astype(np.float32)).to(x.device)
    fine = torch.from_numpy(r.randn(*x.shape).astype(np.float32)).to(x.device)
    return (x + scale * F.interpolate(z, size=tuple(x.shape[2:]), mode='bilinear', align_corners=False) + 0.3 * scale * fine).clamp(-1, 1).contiguous()


def case_inputs(name):
    n, h, w = CASES[name]
    x = images(n, h, w, seed=h + w)
    return perturbed(x, seed=h), x          # (x: the image the gradient is for, y: the target)


def layer_terms(net, lin, x, y):
    """The reference's LPIPS.forward around `net` (returns the five normalised feature maps) and `lin`, term by term: [5, N]."""
    feat_x, feat_y = net(x), net(y)
    diff = [(fx - fy) ** 2 for fx, fy in zip(feat_x, feat_y)]
    res = [l(d).mean((2, 3), True) for d, l in zip(diff, lin)]
    return torch.stack([r.reshape(-1) for r in res])


def loss_from_terms(terms):
    return terms.sum() / terms.shape[1]


def loss_and_grad(net, lin, x, y):
    """(loss, [5, N] terms, d loss / d x), detached."""
    x = x.detach().clone().requires_grad_(True)
    terms = layer_terms(net, lin, x, y.detach())
    loss = loss_from_terms(terms)
    grad, = torch.autograd.grad(loss, x)
    return loss.detach(), terms.detach(), grad


def min_pixel_norm(net, x):
    """Smallest channel norm over all pixels of all five NORMALISED maps: ~1 unless a pixel's raw features are all zero (then 0)."""
    with torch.no_grad():
        return min(float(f.pow(2).sum(1).sqrt().min()) for f in net(x))


def build(dtype=torch.float32, device='cpu', seed=0):
    """The package's LPIPS with the synthetic weights, through the strict state-dict route."""
    from criteria.lpips import LPIPS
    m = LPIPS(pretrained=False)
    m.load_state_dict(state_dict(seed=seed), strict=True)
    return m.to(device=device, dtype=dtype)


def whole_bound(e_ref32, ref64, factor=2.0):
    """The project's whole-quantity rule: factor x the float32 yardstick's own error + 1e-7 max|fp64|."""
    return factor * float(e_ref32) + 1e-7 * float(np.abs(np.asarray(ref64)).max())
