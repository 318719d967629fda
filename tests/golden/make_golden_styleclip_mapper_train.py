"""Golden fixtures of StyleCLIP mapper training, produced by running the REFERENCE's own code on the CPU:

  styleclip_mapper_train.npz
    <case>/dx             d/dx of  sum(dDelta * m(x)) + sum(dOut * (x + 0.1 * m(x)))   [6, 16, 512] float32, under CPU autograd of
                          the reference's latent_mappers.py; x = mapper_cases.inputs(), (dDelta, dOut) = mapper_train_cases.upstream(6, 'both')
    <case>/<key>          the gradient of every state-dict entry: biases in full, weights on the lattice [::37, ::41]
    ranger/<name>         the reference's Ranger(lr=0.5) over 13 steps on an [8, 8] and an [8] parameter with the seeded gradients
                          of mapper_train_cases.ranger_grads: parameters after every step, [13, ...] float32
  styleclip_train_options.json
    the defaults of the reference's TrainOptions parser (settings only)

The cases are tests/mapper_cases.py and tests/mapper_train_cases.py; the fixtures store results only.  Run with the reference
tree's root as the argument:
    python tests/golden/make_golden_styleclip_mapper_train.py <reference tree>

As in make_golden_styleclip_mapper.py, `torch.Tensor.cuda` is patched to the identity while this script runs (the reference's
`fused_leaky_relu` moves its input with `.cuda()`).  Nothing from the reference is copied."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mapper_cases as cases  # noqa: E402
import mapper_train_cases as tc  # noqa: E402


def main(ref):
    sys.path.insert(0, ref)
    torch.Tensor.cuda = lambda self, *a, **k: self
    from editing.styleclip_mapper import latent_mappers as ref_lm
    from editing.styleclip_mapper.options.train_options import TrainOptions
    from utils.ranger import Ranger
    out = {}
    d_delta, d_out = (torch.from_numpy(a) for a in tc.upstream(6, 'both'))
    for case in tc.GOLDEN_CASES:
        o = cases.opts(case)
        m = ref_lm.SingleMapper(o) if o.mapper_type == 'SingleMapper' else ref_lm.LevelsMapper(o)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in cases.state_dict(o).items()}, strict=True)
        m.train()
        x = torch.from_numpy(cases.inputs()).requires_grad_(True)
        delta = m(x)
        ((d_delta * delta).sum() + (d_out * (x + 0.1 * delta)).sum()).backward()
        out[f'{case}/dx'] = x.grad.numpy().astype(np.float32)
        for k, p in m.named_parameters():
            g = p.grad.numpy().astype(np.float32)
            out[f'{case}/{k}'] = g[tc.W_LATTICE] if g.ndim == 2 else g
    params = {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in tc.ranger_init().items()}
    opt = Ranger(list(params.values()), lr=tc.RANGER_LR)
    traj = {k: [] for k in params}
    for step in range(1, tc.RANGER_STEPS + 1):
        for k, g in tc.ranger_grads(step).items():
            params[k].grad = torch.from_numpy(g.copy())
        opt.step()
        for k, p in params.items():
            traj[k].append(p.detach().numpy().copy())
    for k, v in traj.items():
        out[f'ranger/{k}'] = np.stack(v).astype(np.float32)
    path = os.path.join(HERE, 'styleclip_mapper_train.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path} ({os.path.getsize(path)} bytes)')
    parser = TrainOptions().parser
    defaults = {a.dest: a.default for a in parser._actions if a.dest != 'help'}
    path = os.path.join(HERE, 'styleclip_train_options.json')
    with open(path, 'w') as f:
        json.dump(defaults, f, indent=1, sort_keys=True)
    print(f'wrote {path}')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: make_golden_styleclip_mapper_train.py <reference tree root>')
    main(sys.argv[1])
