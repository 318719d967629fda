"""Writes tests/golden/lpips.npz and lpips_manifest.json from the REFERENCE implementation, on the CPU.

    python tests/golden/make_golden_lpips.py /path/to/reference

The reference tree goes first on sys.path and nothing of this package is imported.  The reference's criteria/lpips/networks.py
imports torchvision, which is absent: a stub `torchvision.models` is registered whose `alexnet(...)` returns an object with the
standard `features` nn.Sequential (untrained).  The reference's AlexNet, LinLayers and normalize_activation are used as they are;
LPIPS.forward is restated around them (tests/lpips_cases.py layer_terms), because the reference's constructor downloads the linear
layers and moves everything to "cuda".  Weights are synthetic (lpips_cases.state_dict) and are not stored, only their key -> shape
manifest.  Per case: the inputs as the float32 values the tests feed; in float64 the loss, the [5, N] per-layer terms and
d loss / d x; and the largest deviation of the reference's own float32 run from the float64 one for each (`*_err32`), the yardstick of
the float32 tests.  No feature pixel of any layer may have zero norm for these seeds: that is asserted here and in the tests."""
import json
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _stub_torchvision():
    def alexnet(*args, **kwargs):
        features = nn.Sequential(
            nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
            nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))
        return types.SimpleNamespace(features=features)
    tv, models = types.ModuleType('torchvision'), types.ModuleType('torchvision.models')
    models.alexnet = alexnet
    tv.models = models
    sys.modules['torchvision'], sys.modules['torchvision.models'] = tv, models


def main(reference_root):
    sys.path.insert(0, reference_root)
    _stub_torchvision()
    from criteria.lpips.networks import AlexNet, LinLayers                  # the reference's
    from criteria.lpips.utils import normalize_activation                   # noqa: F401  (what its BaseNet.forward applies)
    import lpips_cases as cases

    def build(dtype):
        net = AlexNet()
        lin = LinLayers(net.n_channels_list)
        return net, lin

    net, lin = build(torch.float32)
    man = OrderedDict()
    for prefix, mod in (('net.', net), ('lin.', lin)):
        for k, v in mod.state_dict().items():
            man[prefix + k] = list(v.shape)
    with open(cases.MANIFEST, 'w') as f:
        json.dump(man, f, indent=0)
    sd = cases.state_dict(OrderedDict((k, tuple(v)) for k, v in man.items()))
    net.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith('net.')})
    lin.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith('lin.')})
    net.eval()
    net64, lin64 = build(torch.float64)
    net64.load_state_dict(net.state_dict())
    lin64.load_state_dict(lin.state_dict())
    net64, lin64 = net64.double().eval(), lin64.double()

    out = {}
    for name in cases.CASES:
        x, y = cases.case_inputs(name)
        floor = cases.min_pixel_norm(net64, x.double())
        assert floor > 0.5 and cases.min_pixel_norm(net64, y.double()) > 0.5, (name, floor)
        loss, terms, grad = cases.loss_and_grad(net64, lin64, x.double(), y.double())
        loss32, terms32, grad32 = cases.loss_and_grad(net, lin, x, y)
        out[f'{name}_x'], out[f'{name}_y'] = x.numpy(), y.numpy()
        out[f'{name}_loss'], out[f'{name}_terms'], out[f'{name}_grad'] = np.float64(loss), terms.numpy(), grad.numpy()
        out[f'{name}_loss_err32'] = np.float64(abs(float(loss32) - float(loss)))
        out[f'{name}_terms_err32'] = np.float64((terms32.double() - terms).abs().max())
        out[f'{name}_grad_err32'] = np.float64((grad32.double() - grad).abs().max())
        print(name, 'loss', float(loss), 'terms', terms.sum(1).tolist(), 'grad rms', float(grad.pow(2).mean().sqrt()), 'max', float(grad.abs().max()),
              'min pixel norm', floor, 'err32: loss', out[f'{name}_loss_err32'], 'terms', out[f'{name}_terms_err32'], 'grad', out[f'{name}_grad_err32'])
    np.savez(cases.GOLDEN, **out)
    print('wrote', cases.GOLDEN, os.path.getsize(cases.GOLDEN), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
