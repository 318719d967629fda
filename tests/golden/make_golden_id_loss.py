"""Writes tests/golden/id_loss.npz and id_loss_manifest.json from the REFERENCE implementation.

    python tests/golden/make_golden_id_loss.py /path/to/reference

The reference's Backbone (models/setgan/encoder/encoders/model_irse.py) is imported with the reference tree first on sys.path and
nothing of this package; its IDLoss.forward is restated around it (tests/id_loss_cases.py: the reference's criteria/id_loss.py
imports a module that does not exist).  Weights are synthetic and are not stored, only their key -> shape manifest.  Per case, in
float64: features of x, y and y_hat, the loss, sim_improvement, the log values and d loss / d y_hat; the inputs as the float32
values the tests feed; and the largest deviation of the reference's own float32 run from the float64 one for each of those
(`*_err32`), which is the yardstick of the float32 tests.  Both sizes take the pool-to-256 branch."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main(reference_root):
    sys.path.insert(0, reference_root)
    from models.setgan.encoder.encoders.model_irse import Backbone          # the reference's
    import id_loss_cases as cases

    torch.manual_seed(0)
    net = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode='ir_se')
    man = {k: list(v.shape) for k, v in net.state_dict().items()}
    with open(cases.MANIFEST, 'w') as f:
        json.dump(man, f, indent=0, sort_keys=True)
    net.load_state_dict(cases.state_dict({k: tuple(v) for k, v in man.items()}))
    net.eval().requires_grad_(False)
    net64 = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode='ir_se')
    net64.load_state_dict(net.state_dict())
    net64 = net64.double().eval().requires_grad_(False)

    out = {}
    for name, b, size, same in (('s64', 2, 64, False), ('s96', 1, 96, True)):
        x = cases.images(b, size, seed=size)
        y = x if same else cases.perturbed(x, seed=size + 1, scale=0.02)
        y_hat = cases.perturbed(x, seed=size + 2)
        loss, sim, logs, feats, grad = cases.loss_and_grad(net64, y_hat.double(), y.double(), x.double())
        loss32, sim32, logs32, feats32, grad32 = cases.loss_and_grad(net, y_hat, y, x)
        out[f'{name}_x'], out[f'{name}_y_hat'] = x.numpy(), y_hat.numpy()
        if not same:
            out[f'{name}_y'] = y.numpy()
        out[f'{name}_feats'] = torch.stack(feats).numpy()
        out[f'{name}_loss'], out[f'{name}_sim'] = np.float64(loss), np.float64(sim)
        out[f'{name}_logs'] = cases.logs_array(logs)
        out[f'{name}_grad'] = grad.numpy()
        out[f'{name}_feats_err32'] = np.float64((torch.stack(feats32).double() - torch.stack(feats)).abs().max())
        out[f'{name}_loss_err32'] = np.float64(abs(float(loss32) - float(loss)))
        out[f'{name}_sim_err32'] = np.float64(abs(sim32 - sim))
        out[f'{name}_logs_err32'] = np.float64(np.abs(cases.logs_array(logs32) - cases.logs_array(logs)).max())
        out[f'{name}_grad_err32'] = np.float64((grad32.double() - grad).abs().max())
        print(name, 'loss', float(loss), 'sim', sim, 'logs', logs, 'grad rms', float(grad.pow(2).mean().sqrt()), 'max', float(grad.abs().max()),
              'err32: feats', out[f'{name}_feats_err32'], 'loss', out[f'{name}_loss_err32'], 'grad', out[f'{name}_grad_err32'])
    np.savez(cases.GOLDEN, **out)
    print('wrote', cases.GOLDEN, os.path.getsize(cases.GOLDEN), 'bytes')


if __name__ == '__main__':
    main(sys.argv[1])
