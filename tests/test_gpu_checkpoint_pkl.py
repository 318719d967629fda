"""GPU: a generator unpickled from foreign module source runs on the native graph once `SG3Generator` has adopted it --
no convolution through `conv2d_gradfix` (the library), HIP launches instead, bit-equal to the `.pt` path, capturable by
`GraphedSynthesis`, differentiable -- while the unadopted object keeps computing the same image on the library's grouped
convolution.  Plus `conv2d_resample` on GPU tensors (HIP `upfirdn2d`) against the reference-recorded arrays.
Tiny networks only: nothing here depends on layer size.  The reference is not read."""
import numpy as np
import pytest
import torch

from ckpt_cases import CONV2D_RESAMPLE_CASES, RESAMPLE_FILTER, conv2d_resample_inputs
from ckpt_helpers import sg3_from_state_dict, standin_generator, write_pickle, write_state_dict
from helpers import golden, maxabs
from synth_weights import synth_ws

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TINY_NET_TOL = 1e-4         # tests/test_gpu_net.py::test_tiny_network: fp32 tiny-network image on the GPU against the oracle
UPFIRDN_GPU_TOL = 1e-5      # tests/test_gpu_ops.py::test_upfirdn2d


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def image(G, ws):
    with torch.no_grad():
        return G.synthesis(ws, noise_mode='const', force_fp32=True)


def native_class():
    from models.stylegan3.networks_stylegan3 import Generator
    return Generator


@pytest.fixture(scope='module', params=['Ttiny', 'Rtiny'])
def loaded(request, tmp_path_factory):
    """(cfg, adopted decoder, unadopted decoder, decoder from the .pt of the same weights), all on the GPU; built once."""
    from models.stylegan3.model import SG3Generator
    cfg = request.param
    tmp = tmp_path_factory.mktemp('ckpt_' + cfg)
    foreign = standin_generator(cfg)
    pkl = write_pickle(tmp / 'g.pkl', G_ema=foreign)
    adopted = SG3Generator(checkpoint_path=pkl, device=DEV).decoder
    kept = SG3Generator(checkpoint_path=pkl, device=DEV, adopt=False).decoder
    from_pt = sg3_from_state_dict(write_state_dict(tmp / 'g.pt', foreign), cfg, device=DEV)
    return cfg, adopted, kept, from_pt


@pytest.fixture
def conv_calls(monkeypatch):
    """Counts calls of `torch_utils.ops.conv2d_gradfix.conv2d`: the only way a pickled graph reaches a convolution."""
    from torch_utils.ops import conv2d_gradfix
    calls = []
    real = conv2d_gradfix.conv2d

    def counted(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)
    monkeypatch.setattr(conv2d_gradfix, 'conv2d', counted)
    return calls


def test_adopted_generator_runs_the_native_kernels(loaded, conv_calls):
    from torch_utils import _sg3abi
    cfg, adopted, kept, _ = loaded
    assert type(adopted) is native_class() and type(kept) is not native_class()
    assert all(p.device.type == 'cuda' for p in adopted.parameters())
    ws = T(synth_ws(2, adopted.num_ws, adopted.w_dim, seed=1))
    before = _sg3abi.launch_count
    img = image(adopted, ws)
    torch.cuda.synchronize()
    assert len(conv_calls) == 0
    assert _sg3abi.launch_count - before >= 30          # 15 convolutions + 14 filtered_lrelu + the input, as in smoke()
    assert bool(torch.isfinite(img).all())
    image(kept, ws)
    assert len(conv_calls) == 15                        # one grouped library convolution per layer


@pytest.mark.parametrize('batch', [1, 3])
def test_adopted_image_equals_the_state_dict_path(loaded, batch):
    cfg, adopted, _, from_pt = loaded
    assert type(from_pt) is native_class()
    ws = T(synth_ws(batch, adopted.num_ws, adopted.w_dim, seed=1))
    assert torch.equal(image(adopted, ws), image(from_pt, ws))


def test_unadopted_forward_agrees_with_the_adopted_one(loaded):
    cfg, adopted, kept, _ = loaded
    ws = T(synth_ws(2, adopted.num_ws, adopted.w_dim, seed=1))
    a, b = image(adopted, ws), image(kept, ws)
    err = maxabs(a.cpu().numpy(), b.cpu().numpy())
    print(f'{cfg}: max|adopted - unadopted| = {err:.3e}')
    assert err <= TINY_NET_TOL
    assert maxabs(a.cpu().numpy(), golden('net_tiny')[cfg + '/img']) <= TINY_NET_TOL


def test_graph_replay_over_an_adopted_generator(loaded):
    from sg3_runtime import GraphedSynthesis
    cfg, adopted, _, _ = loaded
    ws = T(synth_ws(2, adopted.num_ws, adopted.w_dim, seed=1))
    ws2 = T(synth_ws(2, adopted.num_ws, adopted.w_dim, seed=2))
    graphed = GraphedSynthesis(adopted, 2)
    assert torch.equal(graphed(ws).clone(), image(adopted, ws))
    assert torch.equal(graphed(ws2).clone(), image(adopted, ws2))


def test_backward_through_an_adopted_generator(loaded):
    cfg, adopted, _, _ = loaded
    ws = T(synth_ws(1, adopted.num_ws, adopted.w_dim, seed=1))
    params = dict(adopted.synthesis.named_parameters())
    assert len(params) == 2 + 1 + 15 * 4 and not any(p.requires_grad for p in params.values())
    try:
        adopted.synthesis.requires_grad_(True)
        adopted.synthesis(ws, noise_mode='const', force_fp32=True).sum().backward()
        for name, p in params.items():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert sum(float(p.grad.abs().sum()) > 0 for p in params.values()) >= len(params) - 2
    finally:
        adopted.synthesis.requires_grad_(False)
        for p in params.values():
            p.grad = None


@pytest.mark.parametrize('up,down', [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_conv2d_resample_on_gpu_tensors(up, down):
    from torch_utils.ops import conv2d_resample, upfirdn2d
    f = upfirdn2d.setup_filter(RESAMPLE_FILTER, device=DEV)
    names = [n for n, c in sorted(CONV2D_RESAMPLE_CASES.items()) if (c['up'], c['down']) == (up, down)]
    assert len(names) == 16
    for name in names:
        c = CONV2D_RESAMPLE_CASES[name]
        x, w = (T(a) for a in conv2d_resample_inputs(c))
        y = conv2d_resample.conv2d_resample(x, w, f=f, up=up, down=down, padding=c['padding'], groups=c['groups'], flip_weight=c['flip_weight'])
        want = golden('ckpt_ops')['conv2d_resample/' + name]
        assert tuple(y.shape) == want.shape, name
        assert maxabs(y.cpu().numpy(), want) <= UPFIRDN_GPU_TOL, name
