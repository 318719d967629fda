"""CPU: StyleCLIP mapper training without a GPU -- the fp64 gradient restatement of tests/mapper_train_cases.py against the
package composite under float64 autograd, the restated Ranger against the reference's recorded trajectory
(tests/golden/styleclip_mapper_train.npz), TrainOptions against the reference's recorded defaults, and the Coach on stubs."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import mapper_cases as cases
import mapper_train_cases as tc
from helpers import HERE

GOLDEN = os.path.join(HERE, 'golden')


@pytest.mark.parametrize('which', ['delta', 'out', 'both'])
@pytest.mark.parametrize('case', ['levels_all', 'levels_no_coarse', 'single'])
def test_fp64_gradient_restatement_matches_float64_autograd(case, which):
    o = cases.opts(case)
    sd = cases.state_dict(o)
    m = cases.build_mapper(o, sd).double()
    x_np = cases.inputs()
    dd, do = tc.upstream(6, which)
    x = torch.from_numpy(x_np).double().requires_grad_(True)
    delta = m(x)
    loss = 0
    if dd is not None:
        loss = loss + (torch.from_numpy(dd).double() * delta).sum()
    if do is not None:
        loss = loss + (torch.from_numpy(do).double() * (x + tc.ALPHA * delta)).sum()
    loss.backward()
    rx, rg = tc.mapper_grads_fp64(sd, o, x_np, dd, do)
    assert float(np.abs(x.grad.numpy() - rx).max()) <= 1e-10 * float(np.abs(rx).max())
    named = dict(m.named_parameters())
    assert set(named) == set(rg)
    for k, g in rg.items():
        assert float(np.abs(named[k].grad.numpy() - g).max()) <= 1e-10 * float(np.abs(g).max()), k


def test_composite_restatement_of_the_op_module_equals_the_modules():
    """torch_utils.ops.latent_mapper.composite (what a double backward differentiates) is the modules' own arithmetic."""
    from torch_utils.ops import latent_mapper
    o = cases.opts('levels_no_coarse')
    m = cases.build_mapper(o, cases.state_dict(o))
    x = torch.from_numpy(cases.latents(2))
    on = [(r, g) for r, g in m._groups() if g is not None]
    lins = [lin for _, g in on for lin in latent_mapper._linears(g)]
    out, delta = latent_mapper.composite(x, [l.weight for l in lins], [l.bias for l in lins], [r for r, _ in on],
                                         [l.scale for l in lins], [l.lr_mul for l in lins], 0.1)
    with torch.enable_grad():
        ref = m(x).detach()
    assert torch.equal(delta.detach(), ref) and torch.equal(out.detach(), x + 0.1 * ref)


def test_ranger_follows_the_reference_trajectory():
    from utils.ranger import Ranger
    gold = np.load(os.path.join(GOLDEN, 'styleclip_mapper_train.npz'))
    params = {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in tc.ranger_init().items()}
    opt = Ranger(list(params.values()), lr=tc.RANGER_LR)
    for step in range(1, tc.RANGER_STEPS + 1):
        for k, g in tc.ranger_grads(step).items():
            params[k].grad = torch.from_numpy(g.copy())
        opt.step()
        for k, p in params.items():
            ref = gold[f'ranger/{k}'][step - 1]
            assert float(np.abs(p.detach().numpy() - ref).max()) <= 1e-5 * float(np.abs(ref).max()), (step, k)
    st = opt.state[params['w']]
    assert set(st) == {'step', 'exp_avg', 'exp_avg_sq', 'slow_buffer'} and st['step'] == tc.RANGER_STEPS
    assert len(opt.radam_buffer) == 10 and opt.gc_gradient_threshold == 1 and Ranger([params['w']], gc_conv_only=True).gc_gradient_threshold == 3
    # the centralised gradient is left in .grad, and only for tensors of more than one dimension
    assert abs(float(params['w'].grad.mean(dim=1).abs().max())) < 1e-6
    assert np.array_equal(params['b'].grad.numpy(), tc.ranger_grads(tc.RANGER_STEPS)['b'])


def test_ranger_checks_and_skips_parameters_without_gradient():
    from utils.ranger import Ranger
    p = torch.nn.Parameter(torch.ones(3, 3))
    q = torch.nn.Parameter(torch.ones(3))
    for kw in (dict(alpha=1.5), dict(alpha=-0.1), dict(k=0), dict(lr=0), dict(lr=-1.0), dict(eps=0)):
        with pytest.raises(ValueError):
            Ranger([p], **kw)
    opt = Ranger([p, q], lr=0.1)
    p.grad = torch.arange(9.0).reshape(3, 3)
    version = p._version
    opt.step()
    assert p._version > version          # caches keyed by the version counter (the mapper's prepared weights) must see the step
    assert torch.equal(q.detach(), torch.ones(3)) and len(opt.state[q]) == 0
    assert not torch.equal(p.detach(), torch.ones(3, 3))
    assert opt.defaults['betas'] == (.95, 0.999) and opt.defaults['eps'] == 1e-5 and opt.defaults['k'] == 6 and opt.defaults['alpha'] == 0.5


def test_train_options_defaults_are_the_references():
    from editing.styleclip_mapper.options.train_options import TrainOptions
    with open(os.path.join(GOLDEN, 'styleclip_train_options.json')) as f:
        ref = json.load(f)
    parser = TrainOptions().parser
    ours = {a.dest: a.default for a in parser._actions if a.dest != 'help'}
    for k, v in ref.items():
        assert k in ours and ours[k] == v, k
    assert set(ours) - set(ref) == {'clip_checkpoint_path', 'text_tokens'}
    required = {a.dest for a in parser._actions if a.required}
    assert required == {'latents_train_path', 'latents_test_path', 'description'}
    o = TrainOptions().parse(['--latents_train_path', 'a', '--latents_test_path', 'b', '--description', 'c', '--id_lambda', '0'])
    assert o.id_lambda == 0 and o.optim_name == 'ranger' and o.learning_rate == 0.5


def test_aggregate_loss_dict_means():
    from utils.train_utils import aggregate_loss_dict
    assert aggregate_loss_dict([{'a': 1.0, 'b': 2.0}, {'a': 3.0}, {'a': 5.0, 'b': 4.0}]) == {'a': 3.0, 'b': 3.0}
    assert aggregate_loss_dict([]) == {}


def test_mapper_train_entry_points_reject_bad_arguments():
    """Host-side argument checks of the new entry points (nothing is launched)."""
    from torch_utils import _sg3abi
    lib = _sg3abi.load()
    assert lib.sg3_latent_mapper_train_forward(None, None) == _sg3abi.SG3_BAD_ARG
    assert lib.sg3_latent_mapper_backward(None, None) == _sg3abi.SG3_BAD_ARG
    assert lib.sg3_ranger_step(None, None) == _sg3abi.SG3_BAD_ARG
    p = _sg3abi.LatentMapperBackwardParams()
    base = 1 << 20
    n, L = 2, 16
    act = n * L * 512 * 4
    p.x, p.weight, p.acts, p.delta, p.dDelta = base, base + 16 * act, base + 2 * act, base + 6 * act, base + 7 * act
    p.dx, p.scratch = base + 8 * act, base + 9 * act
    p.N, p.L, p.D, p.groups = n, L, 512, 1
    p.levelBegin[0], p.levelEnd[0] = 0, 16

    def rc(**kw):
        q = _sg3abi.LatentMapperBackwardParams.from_buffer_copy(p)
        for k, v in kw.items():
            setattr(q, k, v)
        return lib.sg3_latent_mapper_backward(ctypes.byref(q), None), _sg3abi.last_error()
    for kw, msg in ((dict(D=256), 'only 512'), (dict(L=33), 'L <= 32'), (dict(dDelta=None), 'neither dDelta nor dOut'),
                    (dict(dx=None), 'nothing to compute'), (dict(dW=base + 40 * act), 'together'), (dict(scratch=base + 8 * act + 16), 'overlap'),
                    (dict(dx=base), 'overlap'), (dict(scratch=None), 'null'), (dict(weight=base + 16 * act + 4), 'aligned')):
        code, err = rc(**kw)
        assert code == _sg3abi.SG3_BAD_ARG and msg in err, (kw, err)
    r = _sg3abi.RangerParams()
    r.count = 0
    assert lib.sg3_ranger_step(ctypes.byref(r), None) == _sg3abi.SG3_BAD_ARG and '1..32' in _sg3abi.last_error()
    r.count, r.beta1, r.beta2, r.eps = 1, 0.95, 0.999, 1e-5
    assert lib.sg3_ranger_step(ctypes.byref(r), None) == _sg3abi.SG3_BAD_ARG and 'null pointer' in _sg3abi.last_error()
    t = r.t[0]
    t.p, t.grad, t.expAvg, t.expAvgSq, t.slow, t.rows, t.cols = base, base + 64, base + 4096, base + 8192, base + 12288, 4, 8
    assert lib.sg3_ranger_step(ctypes.byref(r), None) == _sg3abi.SG3_BAD_ARG and 'overlaps' in _sg3abi.last_error()


def test_new_structs_match_the_header():
    import re
    from torch_utils import _sg3abi
    with open(os.path.join(os.path.dirname(HERE), 'include', 'sg3_ops.h')) as f:
        src = f.read()
    for cname, cls in (('sg3_latent_mapper_train_params', _sg3abi.LatentMapperTrainParams),
                       ('sg3_latent_mapper_backward_params', _sg3abi.LatentMapperBackwardParams),
                       ('sg3_ranger_tensor', _sg3abi.RangerTensor), ('sg3_ranger_params', _sg3abi.RangerParams)):
        body = re.search(r'typedef struct ' + cname + r' \{(.*?)\} ' + cname + ';', src, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        names = []
        for decl in body.split(';'):
            if decl.strip():
                parts = decl.strip().split(',')
                names += [re.sub(r'\[\d+\]|\*', '', nm) for nm in [parts[0].split()[-1]] + [q.strip() for q in parts[1:]]]
        assert names == [n for n, _ in cls._fields_], cname
    assert ctypes.sizeof(_sg3abi.RangerTensor) == 56


# ---------------------------------------------------------------------------------------------------------------------------

class _StubSynthesis(torch.nn.Module):
    """A differentiable stand-in for the generator's synthesis network: an 8 x 8 'image' from a fixed projection of w."""

    def __init__(self):
        super().__init__()
        self.proj = torch.nn.Parameter(torch.from_numpy(cases._rs('stub_proj', 0).randn(512, 3 * 8 * 8).astype(np.float32) / 64))

    def forward(self, w):
        return torch.tanh(w.mean(dim=1) @ self.proj).reshape(-1, 3, 8, 8)


def _stub_net(o):
    from editing.styleclip_mapper import latent_mappers
    net = torch.nn.Module()
    net.mapper = latent_mappers.LevelsMapper(o)
    net.decoder = torch.nn.Module()
    net.decoder.synthesis = _StubSynthesis()
    return net


def _stub_opts(tmp_path, **kw):
    torch.save(torch.from_numpy(cases.latents(6)), tmp_path / 'train.pt')
    torch.save(torch.from_numpy(cases.latents(3, seed=2)), tmp_path / 'test.pt')
    o = dict(cases.CASES['levels_all'], exp_dir=str(tmp_path / 'exp'), latents_train_path=str(tmp_path / 'train.pt'),
             latents_test_path=str(tmp_path / 'test.pt'), train_dataset_size=6, test_dataset_size=3, batch_size=2, test_batch_size=1,
             workers=0, test_workers=0, learning_rate=0.5, optim_name='ranger', id_lambda=0.0, clip_lambda=1.0, latent_l2_lambda=0.3,
             stylegan_weights=None, truncation_psi=0.7, stylegan_size=64, checkpoint_path=None, max_steps=1, image_interval=1,
             board_interval=1, val_interval=100, save_interval=1, description='a stub', device='cpu')
    o.update(kw)
    return types.SimpleNamespace(**o)


def _stub_clip_loss(image, text):
    return (image ** 2).mean(dim=(1, 2, 3)).reshape(-1, 1) + 0.0 * text.float().sum()


def test_coach_needs_an_id_loss_module_when_id_lambda_is_positive(tmp_path):
    from editing.styleclip_mapper.training.coach import Coach
    o = _stub_opts(tmp_path, id_lambda=0.06)
    with pytest.raises(NotImplementedError, match='--id_lambda 0'):
        Coach(o, net=_stub_net(o), clip_loss=_stub_clip_loss, text_tokens=torch.zeros(1, 4, dtype=torch.long))


def test_coach_two_steps_on_stubs(tmp_path):
    from editing.styleclip_mapper.styleclip_mapper import get_keys
    from editing.styleclip_mapper.training.coach import Coach
    from editing.styleclip_mapper import latent_mappers
    o = _stub_opts(tmp_path)
    net = _stub_net(o)
    before = {k: v.detach().clone() for k, v in net.mapper.named_parameters()}
    calls = []

    class _Id(torch.nn.Module):
        def forward(self, y_hat, y, x):
            calls.append(tuple(y_hat.shape))
            return ((y_hat - y) ** 2).mean(), 0.25, []
    o.id_lambda = 0.5
    coach = Coach(o, id_loss=_Id(), net=net, clip_loss=_stub_clip_loss, text_tokens=torch.zeros(1, 4, dtype=torch.long))
    assert not any(p.requires_grad for p in net.decoder.parameters()) and not net.decoder.training
    coach.train()                                  # max_steps = 1: steps 0 and 1
    assert coach.global_step == 1 and len(calls) >= 2
    assert net.mapper.training
    for k, p in net.mapper.named_parameters():
        assert not torch.equal(p.detach(), before[k]), k
    assert all(p.grad is None for p in net.decoder.parameters())
    with open(os.path.join(o.exp_dir, 'logs', 'metrics.jsonl')) as f:
        rows = [json.loads(line) for line in f]
    assert [r['step'] for r in rows if r['prefix'] == 'train'] == [0, 1]
    assert all(np.isfinite(r['loss']) and {'loss_clip', 'loss_l2_latent', 'loss_id', 'id_improve'} <= set(r) for r in rows)
    assert os.path.exists(os.path.join(o.exp_dir, 'logs', 'images_train', '00000.jpg'))
    # the checkpoint round-trips through get_keys / load_state_dict as StyleCLIPMapper.load_weights reads it
    ckpt = torch.load(os.path.join(o.exp_dir, 'checkpoints', 'iteration_1.pt'), map_location='cpu', weights_only=False)
    assert set(ckpt) == {'state_dict', 'opts'} and ckpt['opts']['description'] == 'a stub'
    m2 = latent_mappers.LevelsMapper(types.SimpleNamespace(**ckpt['opts']))
    m2.load_state_dict(get_keys(ckpt, 'mapper'), strict=True)
    for k, p in net.mapper.named_parameters():
        assert torch.equal(dict(m2.named_parameters())[k].detach(), p.detach()), k
