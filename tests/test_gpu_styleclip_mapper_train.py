"""GPU: StyleCLIP mapper training -- the HIP mapper backward (csrc/sg3_latent_mapper.hip) against the fp64 restatement in
tests/mapper_train_cases.py and the reference's own gradients (tests/golden/styleclip_mapper_train.npz); forward equality with
the inference path, determinism, batch invariance, the path taken, the double backward, the preparation cache, the fused Ranger
step (csrc/sg3_ranger.hip), and the Coach end to end on the mini generators."""
import json
import os
import types

import numpy as np
import pytest
import torch

import mapper_cases as cases
import mapper_train_cases as tc
from helpers import HERE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CASE_OPTS = {
    'levels_all': cases.opts('levels_all'),
    'levels_no_medium': cases.opts('levels_all', no_medium_mapper=True),
    'levels_none': cases.opts('levels_all', no_coarse_mapper=True, no_medium_mapper=True, no_fine_mapper=True),
    'single': cases.opts('single'),
}


def _t(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def grads(m, x_np, d_delta, d_out, train, x_grad=True):
    """(dx, {name: grad}) as numpy (None where autograd left none) of sum(dDelta * delta) + sum(dOut * out).  train=True runs the
    module in training mode (the HIP path): `m(x)` for delta alone, `m.edit(x)` for out alone, both from one call otherwise;
    train=False is the eval-mode composite under autograd (the fp32 yardstick)."""
    m.train(train)
    m.zero_grad(set_to_none=True)
    x = _t(x_np).requires_grad_(x_grad)
    dd, do = _t(d_delta), _t(d_out)
    with torch.enable_grad():
        if not train:
            delta = m(x)
            out = x + tc.ALPHA * delta
        elif dd is not None and do is not None:
            out, delta = m._fused_train(x, tc.ALPHA, True)
        elif do is not None:
            out, delta = m.edit(x, tc.ALPHA), None
        else:
            out, delta = None, m(x)
        loss = 0
        if dd is not None:
            loss = loss + (dd * delta).sum()
        if do is not None:
            loss = loss + (do * out).sum()
        if torch.is_tensor(loss) and loss.requires_grad:       # no enabled group and no dOut: nothing depends on x
            loss.backward()
    m.eval()
    g = {k: (None if p.grad is None else p.grad.detach().cpu().numpy()) for k, p in m.named_parameters()}
    return (None if x.grad is None else x.grad.cpu().numpy()), g


def check_bound(hip, t32, ref, what, ratios=None, cls=None):
    hip = np.zeros_like(ref, dtype=np.float32) if hip is None else hip
    t32 = np.zeros_like(ref, dtype=np.float32) if t32 is None else t32
    assert np.isfinite(hip).all(), what
    e_hip = float(np.abs(hip - ref).max())
    e_t32 = float(np.abs(t32 - ref).max())
    bound = 2 * e_t32 + 1e-7 * float(np.abs(ref).max())
    if ratios is not None and e_t32 > 0:
        ratios.setdefault(cls, []).append(e_hip / e_t32)
    assert e_hip <= bound, f'{what}: max|hip - fp64| = {e_hip:.3e} > {bound:.3e} (torch32 {e_t32:.3e})'


def _cls(key):
    return 'dW' if key.endswith('weight') else 'dB'


def _run_case(case, n, which, x_scale=1.0, w_scale=1.0):
    o = CASE_OPTS[case]
    sd = cases.state_dict(o, w_scale=w_scale)
    m = cases.build_mapper(o, sd, DEV)
    x = cases.latents(n, scale=x_scale)
    dd, do = tc.upstream(n, which)
    hx, hg = grads(m, x, dd, do, True)
    tx, tg = grads(m, x, dd, do, False)
    rx, rg = tc.mapper_grads_fp64(sd, o, x, dd, do)
    ratios = {}
    what = f'{case} N={n} {which} x*{x_scale} w*{w_scale}'
    if case == 'levels_none':
        assert np.array_equal(np.zeros_like(x) if hx is None else hx, np.zeros_like(x) if do is None else do)
    check_bound(hx, tx, rx, f'dx {what}', ratios, 'dx')
    assert set(hg) == set(rg)
    for k in rg:
        check_bound(hg[k], tg[k], rg[k], f'{k} {what}', ratios, _cls(k))
    print(f'{what}: e_hip / e_torch32 max ' + ', '.join(f'{c} {max(v):.3f}' for c, v in sorted(ratios.items())))


@pytest.mark.parametrize('which', ['delta', 'out', 'both'])
@pytest.mark.parametrize('n', [1, 2, 7, 33])
@pytest.mark.parametrize('case', list(CASE_OPTS))
def test_grads_vs_fp64(case, n, which):
    _run_case(case, n, which)


@pytest.mark.parametrize('x_scale', [1e-3, 1.0, 1e3])
@pytest.mark.parametrize('w_scale', [2.0 ** -8, 1.0, 2.0 ** 8])
@pytest.mark.parametrize('case', ['levels_all', 'single'])
def test_grads_vs_fp64_magnitudes(case, x_scale, w_scale):
    _run_case(case, 7, 'both', x_scale, w_scale)


@pytest.mark.parametrize('case', tc.GOLDEN_CASES)
def test_grads_vs_reference_golden(case):
    gold = np.load(os.path.join(HERE, 'golden', 'styleclip_mapper_train.npz'))
    o = cases.opts(case)
    sd = cases.state_dict(o)
    m = cases.build_mapper(o, sd, DEV)
    x = cases.inputs()
    dd, do = tc.upstream(6, 'both')
    hx, hg = grads(m, x, dd, do, True)
    rx, rg = tc.mapper_grads_fp64(sd, o, x, dd, do)
    check_bound(hx, gold[f'{case}/dx'], rx, f'golden dx {case}')
    for k in rg:
        if k.endswith('weight'):
            check_bound(hg[k][tc.W_LATTICE], gold[f'{case}/{k}'], rg[k][tc.W_LATTICE], f'golden {k} {case}')
        else:
            check_bound(hg[k], gold[f'{case}/{k}'], rg[k], f'golden {k} {case}')


@pytest.mark.parametrize('case', ['levels_all', 'levels_no_medium', 'single'])
def test_training_forward_is_bitwise_the_inference_forward(case):
    o = CASE_OPTS[case]
    m = cases.build_mapper(o, cases.state_dict(o), DEV)
    x = _t(cases.latents(7))
    with torch.no_grad():
        delta, w_hat = m(x), m.edit(x, 0.25)
    m.train()
    with torch.enable_grad():
        xg = x.clone().requires_grad_(True)
        assert torch.equal(m(xg).detach(), delta)
        assert torch.equal(m.edit(xg, 0.25).detach(), w_hat)
        out, d = m._fused_train(xg, 0.25, True)
        assert torch.equal(out.detach(), w_hat) and torch.equal(d.detach(), delta)
        assert m(xg).requires_grad and m(x).requires_grad          # parameters alone carry the graph too


@pytest.mark.parametrize('case', ['levels_all', 'single'])
def test_backward_determinism_and_batch_invariance(case):
    o = CASE_OPTS[case]
    m = cases.build_mapper(o, cases.state_dict(o), DEV)
    x = cases.latents(33)
    dd, do = tc.upstream(33, 'both')
    ax, ag = grads(m, x, dd, do, True)
    bx, bg = grads(m, x, dd, do, True)
    assert np.array_equal(ax, bx)
    for k in ag:
        assert np.array_equal(ag[k], bg[k]), k
    for i in (0, 5, 16, 32):
        sx, _ = grads(m, x[i:i + 1], dd[i:i + 1], do[i:i + 1], True)
        assert np.array_equal(sx[0], ax[i]), i


def test_training_path_is_hip_and_eval_path_is_composite():
    from torch_utils import _sg3abi
    o = CASE_OPTS['levels_all']
    m = cases.build_mapper(o, cases.state_dict(o), DEV)
    x = _t(cases.latents(2)).requires_grad_(True)
    m.train()
    m(x).sum().backward()                      # prepares the weights
    torch.cuda.synchronize()
    before = _sg3abi.launch_count
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        m(x).sum().backward()
        m.edit(x).sum().backward()
    torch.cuda.synchronize()
    assert _sg3abi.launch_count - before == 4          # one forward and one backward call each
    names = {e.key for e in prof.key_averages()}
    assert not names & {'aten::mm', 'aten::addmm', 'aten::linear', 'aten::leaky_relu', 'aten::leaky_relu_backward'}, names
    m.eval()
    before = _sg3abi.launch_count
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
        m(x).sum().backward()
    assert _sg3abi.launch_count == before
    names = {e.key for e in prof.key_averages()}
    assert 'aten::leaky_relu' in names and 'aten::leaky_relu_backward' in names, names


def test_double_backward_goes_through_the_composite():
    o = CASE_OPTS['levels_all']
    m = cases.build_mapper(o, cases.state_dict(o), DEV)
    res = {}
    for train in (True, False):
        m.train(train)
        m.zero_grad(set_to_none=True)
        x = _t(cases.latents(2)).requires_grad_(True)
        with torch.enable_grad():
            (gx,) = torch.autograd.grad((m(x) ** 2).sum(), x, create_graph=True)
            assert gx.requires_grad
            (gx ** 2).sum().backward()
        res[train] = [gx.detach(), x.grad] + [p.grad.clone() for p in m.parameters()]
    m.eval()
    # both sides are fp32 through four 512-term layers (relative differences near 1e-5); a missing term is of order one
    for a, b in zip(res[True], res[False]):
        assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())


def test_preparation_follows_an_optimizer_step_and_frozen_parameters_skip_wgrad():
    o = CASE_OPTS['levels_all']
    m = cases.build_mapper(o, cases.state_dict(o), DEV)
    x_np = cases.latents(3)
    x = _t(x_np)
    m.train()
    before = m(x).detach().clone()
    opt = torch.optim.SGD(m.parameters(), lr=50.0)
    m(x).sum().backward()
    opt.step()
    after = m(x).detach()
    assert not torch.equal(before, after)
    m.eval()
    sd2 = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    with torch.enable_grad():
        t32 = m(x).detach()
    ref = cases.mapper_fp64(sd2, o, x_np)
    e_hip, e_t32 = float(np.abs(after.cpu().numpy() - ref).max()), float(np.abs(t32.cpu().numpy() - ref).max())
    assert e_hip <= 2 * e_t32 + 1e-7 * float(np.abs(ref).max()), (e_hip, e_t32)
    # frozen parameters: dx only; frozen input: parameter gradients only
    dd, do = tc.upstream(3, 'both')
    rx, rg = tc.mapper_grads_fp64(sd2, o, x_np, dd, do)
    tx, tg = grads(m, x_np, dd, do, False)
    m.requires_grad_(False)
    hx, hg = grads(m, x_np, dd, do, True)
    assert all(v is None for v in hg.values())
    check_bound(hx, tx, rx, 'dx with frozen parameters')
    m.requires_grad_(True)
    hx, hg = grads(m, x_np, dd, do, True, x_grad=False)
    assert hx is None
    for k in rg:
        check_bound(hg[k], tg[k], rg[k], f'{k} with a frozen input')


# ---------------------------------------------------------------------------------------------------------------------------

def _ranger_params(dtype, device=DEV):
    o = cases.opts('levels_coarse_only')
    sd = cases.state_dict(o)
    return {k: torch.nn.Parameter(torch.from_numpy(v).to(device=device, dtype=dtype)) for k, v in sd.items()}


def test_fused_ranger_vs_torch_and_fp64():
    from torch_utils import _sg3abi
    from utils.ranger import Ranger
    sets = {'fused': _ranger_params(torch.float32), 't32': _ranger_params(torch.float32), 'f64': _ranger_params(torch.float64)}
    opts = {k: Ranger(list(v.values()), lr=tc.RANGER_LR) for k, v in sets.items()}
    opts['t32'].fused = False
    shapes = {k: tuple(v.shape) for k, v in sets['fused'].items()}
    ratios = {}
    for step in range(1, tc.RANGER_STEPS + 1):
        g = tc.ranger_grads(step, shapes)
        for name, ps in sets.items():
            for k, p in ps.items():
                p.grad = torch.from_numpy(g[k]).to(device=DEV, dtype=p.dtype)
            before = _sg3abi.launch_count
            opts[name].step()
            assert _sg3abi.launch_count - before == (1 if name == 'fused' else 0), (name, step)
        for k in shapes:
            ref = sets['f64'][k].detach().cpu().numpy()
            check_bound(sets['fused'][k].detach().cpu().numpy(), sets['t32'][k].detach().cpu().numpy(), ref, f'ranger step {step} {k}',
                        ratios, 'p2' if len(shapes[k]) == 2 else 'p1')
            if len(shapes[k]) == 2:      # the centralised gradient is left in .grad on both paths
                check_bound(sets['fused'][k].grad.cpu().numpy(), sets['t32'][k].grad.cpu().numpy(), sets['f64'][k].grad.cpu().numpy(), f'ranger grad {step} {k}')
    print('ranger e_fused / e_torch32 max ' + ', '.join(f'{c} {max(v):.3f}' for c, v in sorted(ratios.items())))
    st = opts['fused'].state[next(iter(sets['fused'].values()))]
    assert set(st) == {'step', 'exp_avg', 'exp_avg_sq', 'slow_buffer'} and st['step'] == tc.RANGER_STEPS


def test_fused_ranger_skips_gradless_and_leaves_odd_tensors_to_torch():
    from torch_utils import _sg3abi
    from utils.ranger import Ranger
    r = np.random.RandomState(5)
    a = torch.nn.Parameter(torch.from_numpy(r.randn(40, 33).astype(np.float32)).to(DEV))
    b = torch.nn.Parameter(torch.from_numpy(r.randn(17).astype(np.float32)).to(DEV))
    opt = Ranger([a, b], lr=0.1)
    a.grad = torch.ones_like(a) + torch.arange(33, device=DEV)
    b0 = b.detach().clone()
    before = _sg3abi.launch_count
    opt.step()
    assert _sg3abi.launch_count - before == 1
    assert torch.equal(b, b0) and len(opt.state[b]) == 0
    # a 4-D parameter, or a non-contiguous one, sends the whole step to the torch path
    c = torch.nn.Parameter(torch.from_numpy(r.randn(4, 3, 3, 3).astype(np.float32)).to(DEV))
    d = torch.nn.Parameter(torch.from_numpy(r.randn(6, 5).astype(np.float32)).to(DEV).t())
    assert not d.is_contiguous()
    for extra in (c, d):
        opt = Ranger([a, extra], lr=0.1)
        a.grad = torch.ones_like(a) + torch.arange(33, device=DEV)
        extra.grad = torch.ones_like(extra) * 0.5 + torch.rand_like(extra)
        e0 = extra.detach().clone()
        before = _sg3abi.launch_count
        opt.step()
        assert _sg3abi.launch_count == before
        assert not torch.equal(extra, e0)


# ---------------------------------------------------------------------------------------------------------------------------

def _fp32_generator(cfg):
    """The seeded decoder with every layer in fp32 (num_fp16_res=0), as the mapper's inference test builds it: fp16 layers would
    move pixels by fp16 steps for a one-ulp change of w and hide the mapper's own difference."""
    from models.stylegan3.networks_stylegan3 import Generator
    from synth_weights import CONFIGS, synth_state_dict
    G = Generator(**CONFIGS[cfg], num_fp16_res=0).eval().requires_grad_(False)
    man = {k: list(v.shape) for k, v in G.state_dict().items()}
    sd = synth_state_dict(man, seed=0, input_bandwidth=float(G.synthesis.input.bandwidth))
    G.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return G.to(DEV)


def _coach(cfg, tmp_path, max_steps):
    import clip_cases
    import clip_loss_cases as lcases
    from criteria.clip_loss import CLIPLoss
    from editing.styleclip_mapper.training.coach import Coach
    torch.save(torch.from_numpy(cases.latents(6)), tmp_path / 'train.pt')
    torch.save(torch.from_numpy(cases.latents(2, seed=2)), tmp_path / 'test.pt')
    o = types.SimpleNamespace(**dict(
        cases.CASES['levels_all'], exp_dir=str(tmp_path / 'exp'), latents_train_path=str(tmp_path / 'train.pt'),
        latents_test_path=str(tmp_path / 'test.pt'), train_dataset_size=6, test_dataset_size=2, batch_size=2, test_batch_size=1,
        workers=0, test_workers=0, learning_rate=0.5, optim_name='ranger', id_lambda=0.0, clip_lambda=1.0, latent_l2_lambda=0.3,
        stylegan_weights=None, truncation_psi=0.7, stylegan_size=64, checkpoint_path=None, max_steps=max_steps, image_interval=1,
        board_interval=1, val_interval=1000, save_interval=max_steps, description='seeded tokens', device=DEV, clip_checkpoint_path=None))
    net = torch.nn.Module()
    net.mapper = cases.build_mapper(cases.opts('levels_all'), cases.state_dict(cases.opts('levels_all')), DEV)
    net.decoder = _fp32_generator(cfg)
    loss = CLIPLoss(lcases.opts(64), model=clip_cases.build(lcases.CFG, device=DEV))
    return Coach(o, net=net, clip_loss=loss, text_tokens=torch.from_numpy(lcases.tokens())), o


@pytest.mark.parametrize('cfg', ['Rmini', 'Tmini'])
def test_coach_one_step_gradients_equal_the_composite_mappers(cfg, tmp_path):
    """The same step twice from the same state: the mapper in training mode (HIP forward and backward) and in eval mode (the
    composite under autograd); generator, CLIP tower and loss are shared.  A misrouted level or group, a missing alpha or a wrong
    lr_mul / scale changes a gradient by order one.  Bound: 1e-2 of the largest entry per tensor.  The 1e-3 first proposed assumed
    fp32 noise only; measured on a correct build the two runs differ by 8.8e-4 (Rmini) and 1.0e-3 (Tmini), and that is not the
    mapper's: the two w_hat differ by one ulp (8e-8) and the gradient that ARRIVES at w_hat already differs by 7.7e-4, because the
    CLIP tower rounds its GEMM operands to fp16 and a one-ulp change of the image moves some of those roundings.  The bound is
    ten times the measured difference, as the rule for this test says when the measurement is not ten times below 1e-3."""
    from torch_utils import _sg3abi
    coach, _ = _coach(cfg, tmp_path, 1)
    w = _t(cases.latents(2))
    with torch.no_grad():
        x = coach.net.decoder.synthesis(w)
    res, up = {}, {}
    for train in (True, False):
        coach.net.mapper.train(train)
        coach.optimizer.zero_grad(set_to_none=True)
        w_hat = coach.edit(w)
        w_hat.retain_grad()
        loss, _ = coach.calc_loss(w, x, w_hat, coach.net.decoder.synthesis(w_hat))
        loss.backward()
        res[train] = {k: p.grad.detach().clone() for k, p in coach.net.mapper.named_parameters()}
        up[train] = (w_hat.detach().clone(), w_hat.grad.detach().clone())
        assert all(p.grad is None for p in coach.net.decoder.parameters())
    rel = {k: float((res[True][k] - g).abs().max()) / float(g.abs().max()) for k, g in res[False].items()}
    d_w = float((up[True][0] - up[False][0]).abs().max()) / float(up[False][0].abs().max())
    d_g = float((up[True][1] - up[False][1]).abs().max()) / float(up[False][1].abs().max())
    print(f'{cfg}: max over tensors of max|dgrad| / max|grad| = {max(rel.values()):.3e}; w_hat differs by {d_w:.3e}, dL/dw_hat by {d_g:.3e}')
    for k, v in rel.items():
        assert float(res[False][k].abs().max()) > 0 and v <= 1e-2, (k, v)


@pytest.mark.parametrize('cfg', ['Rmini', 'Tmini'])
def test_coach_three_steps_checkpoint_and_inference(cfg, tmp_path):
    from editing.styleclip_mapper import latent_mappers
    from editing.styleclip_mapper.scripts.inference import run_on_batch
    from editing.styleclip_mapper.styleclip_mapper import get_keys
    from torch_utils import _sg3abi
    coach, o = _coach(cfg, tmp_path, 2)
    before = {k: v.detach().clone() for k, v in coach.net.mapper.named_parameters()}
    coach.train()                                     # steps 0, 1, 2
    assert coach.global_step == 2
    with open(os.path.join(o.exp_dir, 'logs', 'metrics.jsonl')) as f:
        rows = [json.loads(line) for line in f if '"train"' in line]
    assert [r['step'] for r in rows] == [0, 1, 2] and all(np.isfinite(r['loss']) and np.isfinite(r['loss_clip']) for r in rows)
    assert all(p.grad is None for p in coach.net.decoder.parameters())
    for k, p in coach.net.mapper.named_parameters():
        assert not torch.equal(p.detach(), before[k]) and bool(torch.isfinite(p).all()), k
    ckpt = torch.load(os.path.join(o.exp_dir, 'checkpoints', 'iteration_2.pt'), map_location='cpu', weights_only=False)
    net2 = torch.nn.Module()
    net2.mapper = latent_mappers.LevelsMapper(types.SimpleNamespace(**ckpt['opts']))
    net2.mapper.load_state_dict(get_keys(ckpt, 'mapper'), strict=True)
    net2.mapper = net2.mapper.eval().to(DEV)
    net2.decoder = coach.net.decoder
    w = _t(cases.latents(2, seed=5))
    x_hat, w_hat = run_on_batch(w, None, net2)
    trained = coach.net.mapper.eval()
    with torch.no_grad():
        assert torch.equal(w_hat, trained.edit(w, 0.1))
        assert torch.equal(x_hat, coach.net.decoder.synthesis(w_hat))
    with torch.enable_grad():
        ref = w + 0.1 * trained(w).detach()
    assert float((w_hat - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
