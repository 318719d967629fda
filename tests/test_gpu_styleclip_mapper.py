"""GPU: the fused StyleCLIP latent mapper kernel (csrc/sg3_latent_mapper.hip) against the fp64 restatement in
tests/mapper_cases.py and the reference's own outputs (tests/golden/styleclip_mapper.npz); batch invariance, determinism, the
HIP path being taken, re-preparation after a parameter edit, graph replay, and run_on_batch end to end."""
import os

import numpy as np
import pytest
import torch

import mapper_cases as cases
from helpers import HERE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

CASE_OPTS = {
    'levels_all': cases.opts('levels_all'),
    'levels_no_coarse': cases.opts('levels_no_coarse'),
    'levels_no_medium': cases.opts('levels_all', no_medium_mapper=True),
    'levels_no_fine': cases.opts('levels_all', no_fine_mapper=True),
    'levels_none': cases.opts('levels_all', no_coarse_mapper=True, no_medium_mapper=True, no_fine_mapper=True),
    'single': cases.opts('single'),
}


def torch_path(m, x):
    """The torch composite on the same device (recording gradients keeps the module off the HIP path)."""
    with torch.enable_grad():
        return m(x).detach()


def check_bound(hip, t32, ref, what):
    e_hip = float(np.abs(hip - ref).max())
    e_t32 = float(np.abs(t32 - ref).max())
    bound = 2 * e_t32 + 1e-7 * float(np.abs(ref).max())
    assert e_hip <= bound, f'{what}: max|hip - fp64| = {e_hip:.3e} > {bound:.3e} (torch32 {e_t32:.3e})'


def _run_case(case, n, x_scale=1.0, w_scale=1.0):
    o = CASE_OPTS[case]
    sd = cases.state_dict(o, w_scale=w_scale)
    m = cases.build_mapper(o, sd, DEV)
    x = torch.from_numpy(cases.latents(n, scale=x_scale)).to(DEV)
    with torch.no_grad():
        hip = m(x)
        w_hat = m.edit(x)
    t32 = torch_path(m, x)
    ref = cases.mapper_fp64(sd, o, x.cpu().numpy())
    check_bound(hip.cpu().numpy(), t32.cpu().numpy(), ref, f'{case} N={n} x*{x_scale} w*{w_scale}')
    xn = x.cpu().numpy().astype(np.float64)
    check_bound(w_hat.cpu().numpy(), (x + 0.1 * t32).cpu().numpy(), xn + 0.1 * ref, f'w_hat {case} N={n}')


@pytest.mark.parametrize('n', [1, 2, 7, 33, 256])
@pytest.mark.parametrize('case', list(CASE_OPTS))
def test_hip_vs_fp64_batch_sizes(case, n):
    _run_case(case, n)


@pytest.mark.parametrize('x_scale', [1e-3, 1.0, 1e3])
@pytest.mark.parametrize('w_scale', [2.0 ** -8, 1.0, 2.0 ** 8])
@pytest.mark.parametrize('case', ['levels_all', 'single'])
def test_hip_vs_fp64_magnitudes(case, x_scale, w_scale):
    _run_case(case, 7, x_scale, w_scale)


@pytest.mark.parametrize('case', list(cases.CASES))
def test_hip_vs_reference_golden(case):
    gold = np.load(os.path.join(HERE, 'golden', 'styleclip_mapper.npz'))[f'{case}/delta']
    o = cases.opts(case)
    sd = cases.state_dict(o)
    x = cases.inputs()
    m = cases.build_mapper(o, sd, DEV)
    with torch.no_grad():
        d = m(torch.from_numpy(x).to(DEV)).cpu().numpy()
        w_hat = m.edit(torch.from_numpy(x).to(DEV)).cpu().numpy()
    ref = cases.mapper_fp64(sd, o, x)
    check_bound(d, gold, ref, f'golden {case}')
    check_bound(w_hat, x + np.float32(0.1) * gold, x.astype(np.float64) + 0.1 * ref, f'golden w_hat {case}')


@pytest.mark.parametrize('case', ['levels_all', 'levels_no_medium', 'single'])
def test_batch_invariance_and_determinism(case):
    o = CASE_OPTS[case]
    m = cases.build_mapper(o, cases.state_dict(o), DEV)
    x = torch.from_numpy(cases.latents(33)).to(DEV)
    with torch.no_grad():
        full = m.edit(x)
        again = m.edit(x)
        assert torch.equal(full, again)
        assert torch.equal(m(x), m(x))
        for i in range(33):
            assert torch.equal(m.edit(x[i:i + 1])[0], full[i]), i


def test_hip_path_is_taken():
    from torch_utils import _sg3abi
    o = CASE_OPTS['levels_all']
    m = cases.build_mapper(o, cases.state_dict(o), DEV)
    x = torch.from_numpy(cases.latents(4)).to(DEV)
    with torch.no_grad():
        m(x)
        torch.cuda.synchronize()
        before = _sg3abi.launch_count
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as prof:
            m(x)
            m.edit(x)
        torch.cuda.synchronize()
    assert _sg3abi.launch_count - before == 2
    names = {e.key for e in prof.key_averages()}
    assert not names & {'aten::linear', 'aten::mm', 'aten::addmm', 'aten::leaky_relu'}, names


def test_weights_reprepared_after_inplace_edit():
    o = CASE_OPTS['levels_all']
    sd = cases.state_dict(o)
    m = cases.build_mapper(o, sd, DEV)
    x = torch.from_numpy(cases.latents(3)).to(DEV)
    with torch.no_grad():
        before = m(x).clone()
        m.medium_mapping.mapping[2].weight.mul_(0.5)
        m.fine_mapping.mapping[4].bias.add_(1.0)
        after = m(x)
    assert not torch.equal(before[:, 5:], after[:, 5:])
    assert torch.equal(before[:, :5], after[:, :5])
    sd2 = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    check_bound(after.cpu().numpy(), torch_path(m, x).cpu().numpy(), cases.mapper_fp64(sd2, o, x.cpu().numpy()), 'after edit')


def test_graph_replay_equals_eager():
    o = CASE_OPTS['levels_all']
    m = cases.build_mapper(o, cases.state_dict(o), DEV)
    x = torch.from_numpy(cases.latents(8)).to(DEV)
    with torch.no_grad():
        eager = m.edit(x).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.edit(x)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m.edit(x)
        x.copy_(torch.from_numpy(cases.latents(8, seed=2)).to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, m.edit(x))
        x.copy_(torch.from_numpy(cases.latents(8)).to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def _transforms(b):
    a = torch.linspace(0.0, 0.4, b)
    t = torch.zeros(b, 3, 3)
    t[:, 0, 0], t[:, 0, 1], t[:, 1, 0], t[:, 1, 1], t[:, 2, 2] = a.cos(), -a.sin(), a.sin(), a.cos(), 1.0
    t[:, 0, 2] = 0.05 * torch.arange(b)
    return t.to(DEV)


def fp32_generator(cfg):
    """build_product_generator's seeded decoder with every layer in fp32 (num_fp16_res=0).  With the default fp16 layers a
    one-ulp change of w moves pixels by fp16 steps (3e-5 at 0.05), which would hide the mapper's own difference."""
    from models.stylegan3.networks_stylegan3 import Generator
    from synth_weights import CONFIGS, synth_state_dict
    G = Generator(**CONFIGS[cfg], num_fp16_res=0).eval().requires_grad_(False)
    man = {k: list(v.shape) for k, v in G.state_dict().items()}
    sd = synth_state_dict(man, seed=0, input_bandwidth=float(G.synthesis.input.bandwidth))
    G.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    return G.to(DEV)


@pytest.mark.parametrize('cfg,b', [('Rmini', 3), ('Tmini', 3), ('R1024', 2)])
def test_run_on_batch_end_to_end(cfg, b):
    from editing.styleclip_mapper.scripts.inference import run_on_batch
    o = CASE_OPTS['levels_all']
    net = torch.nn.Module()
    net.mapper = cases.build_mapper(o, cases.state_dict(o), DEV)
    net.decoder = fp32_generator(cfg)
    w = torch.from_numpy(cases.latents(b)).to(DEV)
    t = _transforms(b)
    x_hat, w_hat, x = run_on_batch(w, t, net, couple_outputs=True)
    assert torch.equal(net.decoder.synthesis.input.transform, t)
    w_t = w + 0.1 * torch_path(net.mapper, w)
    with torch.no_grad():
        ref = net.decoder.synthesis(w_t)
        ref_x = net.decoder.synthesis(w)
    assert float((w_hat - w_t).abs().max()) <= 1e-5 * float(w.abs().max())
    assert float((x_hat - ref).abs().max()) <= 1e-4, float((x_hat - ref).abs().max())
    assert float((x - ref_x).abs().max()) <= 1e-6
    assert x_hat.shape == (b, 3, net.decoder.img_resolution, net.decoder.img_resolution)
