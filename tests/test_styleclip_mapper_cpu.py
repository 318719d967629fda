"""CPU: the StyleCLIP latent mapper package (editing/styleclip_mapper) against the reference's own outputs
(tests/golden/styleclip_mapper.npz), the reference's module structure, checkpoint layout and inference-loop item set; and the
argument checks of the sg3_latent_mapper C entry point (nothing is launched)."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import mapper_cases as cases
from helpers import HERE, build_product_generator

ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, 'golden', 'styleclip_mapper.npz'))


def _x():
    return torch.from_numpy(cases.inputs())


def _w_hat(x, delta):
    return x + np.float32(0.1) * delta          # float32: one rounded product, one rounded sum (as the reference's w + 0.1 * m(w))


@pytest.mark.parametrize('case', list(cases.CASES))
def test_state_dict_keys_and_shapes_match_reference(case):
    m = cases.build_mapper(cases.opts(case), cases.state_dict(cases.opts(case)))
    assert [f'{k}:{list(v.shape)}' for k, v in m.state_dict().items()] == list(GOLD[f'{case}/keys'])


def test_level_mapper_module_names():
    from editing.styleclip_mapper import latent_mappers
    m = latent_mappers.LevelsMapper(cases.opts('levels_all'))
    assert [n for n, _ in m.named_children()] == ['course_mapping', 'medium_mapping', 'fine_mapping']
    assert isinstance(m.course_mapping.mapping[0], latent_mappers.PixelNorm)
    from models.stylegan2.model import EqualLinear
    assert latent_mappers.EqualLinear is EqualLinear
    assert all(isinstance(m.course_mapping.mapping[i], EqualLinear) and m.course_mapping.mapping[i].lr_mul == 0.01 for i in range(1, 5))


def test_get_keys_with_and_without_state_dict():
    from editing.styleclip_mapper.styleclip_mapper import get_keys
    d = {'mapper.a.weight': 1, 'mapper.b': 2, 'decoder.x': 3, 'mapperx': 4}
    assert get_keys(d, 'mapper') == {'a.weight': 1, 'b': 2, '': 4}
    assert get_keys({'state_dict': d, 'opts': {}}, 'mapper') == get_keys(d, 'mapper')
    assert get_keys({'decoder.x': 1}, 'mapper') == {}


@pytest.mark.parametrize('wrap', [False, True])
def test_checkpoint_loads_strict(tmp_path, wrap):
    from editing.styleclip_mapper.styleclip_mapper import StyleCLIPMapper
    o = cases.opts('levels_no_coarse')
    sd = {'mapper.' + k: torch.from_numpy(v) for k, v in cases.state_dict(o, seed=5).items()}
    path = tmp_path / 'ckpt.pt'
    torch.save({'state_dict': sd, 'opts': {}} if wrap else sd, path)
    net = StyleCLIPMapper.__new__(StyleCLIPMapper)
    torch.nn.Module.__init__(net)
    net.opts = types.SimpleNamespace(checkpoint_path=str(path), **cases.CASES['levels_no_coarse'])
    net.mapper = net.set_mapper()
    net.load_weights()
    for k, v in sd.items():
        assert torch.equal(net.mapper.state_dict()[k[len('mapper.'):]], v)
    torch.save({'mapper.extra': torch.zeros(1), **sd}, path)
    with pytest.raises(RuntimeError):
        net.load_weights()


def test_set_mapper_rejects_unknown_type():
    from editing.styleclip_mapper.styleclip_mapper import StyleCLIPMapper
    net = StyleCLIPMapper.__new__(StyleCLIPMapper)
    torch.nn.Module.__init__(net)
    net.opts = types.SimpleNamespace(mapper_type='Bogus')
    with pytest.raises(Exception, match='not a valid mapper'):
        net.set_mapper()


@pytest.mark.parametrize('case', list(cases.CASES))
def test_torch_path_matches_reference_golden(case):
    o = cases.opts(case)
    m = cases.build_mapper(o, cases.state_dict(o))
    x = _x()
    with torch.no_grad():
        delta = m(x).numpy()
        w_hat = m.edit(x).numpy()
    gold = GOLD[f'{case}/delta']
    assert np.abs(delta - gold).max() <= 1e-6 * np.abs(gold).max()
    assert np.abs(w_hat - _w_hat(x.numpy(), gold)).max() <= 1e-6 * np.abs(x.numpy()).max()
    ref = cases.mapper_fp64(cases.state_dict(o), o, x.numpy())
    assert np.abs(gold - ref).max() <= 1e-4 * np.abs(ref).max()        # the restatement is the reference's arithmetic


@pytest.mark.parametrize('case', ['levels_all', 'single'])
def test_per_feature_pixelnorm_misses_golden(case):
    o = cases.opts(case)
    sd = cases.state_dict(o)
    x = cases.inputs()
    gold = GOLD[f'{case}/delta']
    right = np.abs(cases.mapper_fp64(sd, o, x) - gold).max()
    wrong = np.abs(cases.mapper_fp64(sd, o, x, per_feature_norm=True) - gold).max()
    assert wrong > 1e3 * max(right, 1e-7) and wrong > 0.05 * np.abs(gold).max(), (right, wrong)


def test_pixelnorm_is_over_dim_1():
    from editing.styleclip_mapper.latent_mappers import PixelNorm
    x = torch.randn(2, 5, 512, dtype=torch.float64)
    y = PixelNorm()(x)
    assert torch.allclose((y ** 2).mean(dim=1), torch.ones(2, 512, dtype=torch.float64), atol=1e-6)
    assert not torch.allclose((y ** 2).mean(dim=2), torch.ones(2, 5, dtype=torch.float64), atol=1e-2)


@pytest.mark.parametrize('case,off', [('levels_no_coarse', [(0, 5)]), ('levels_coarse_only', [(5, 8), (8, 16)])])
def test_disabled_groups_give_zeros(case, off):
    o = cases.opts(case)
    m = cases.build_mapper(o, cases.state_dict(o))
    x = _x()
    with torch.no_grad():
        d = m(x)
        w_hat = m.edit(x)
    for b, e in off:
        assert torch.equal(d[:, b:e], torch.zeros_like(d[:, b:e]))
        assert torch.equal(w_hat[:, b:e], x[:, b:e])
    on = [lv for lv in range(16) if not any(b <= lv < e for b, e in off)]
    assert float(d[:, on].abs().min(dim=2).values.max()) >= 0.0 and float(d[:, on].abs().max()) > 0.1


def test_all_groups_off():
    o = types.SimpleNamespace(mapper_type='LevelsMapper', no_coarse_mapper=True, no_medium_mapper=True, no_fine_mapper=True)
    m = cases.build_mapper(o, {})
    x = _x()
    with torch.no_grad():
        assert torch.equal(m(x), torch.zeros_like(x))


def test_fused_leaky_relu_bias_axis():
    from editing.styleclip_mapper.latent_mappers import FusedLeakyReLU, fused_leaky_relu
    x3, b = torch.randn(2, 3, 4), torch.randn(4)
    assert torch.allclose(fused_leaky_relu(x3, b), torch.nn.functional.leaky_relu(x3 + b.view(1, 1, 4), 0.2) * 2 ** 0.5)
    x4, b4 = torch.randn(2, 4, 3, 3), torch.randn(4)
    assert torch.allclose(fused_leaky_relu(x4, b4), torch.nn.functional.leaky_relu(x4 + b4.view(1, 4, 1, 1), 0.2) * 2 ** 0.5)
    act = FusedLeakyReLU(4)
    assert torch.equal(act(x4), fused_leaky_relu(x4, torch.zeros(4)))


def test_latents_dataset_with_object_transforms(tmp_path):
    from editing.styleclip_mapper.datasets.latents_dataset import LatentsDataset
    lat = torch.randn(4, 16, 512)
    recs = np.empty(4, dtype=object)
    for i in range(4):
        recs[i] = (f'img{i}', i, None, np.full((3, 3), i + 0.5, dtype=np.float64))
    np.save(tmp_path / 't.npy', recs, allow_pickle=True)
    tr = np.load(tmp_path / 't.npy', allow_pickle=True)
    ds = LatentsDataset(lat, opts=None, transforms=tr)
    assert len(ds) == 4
    w, t = ds[2]
    assert torch.equal(w, lat[2]) and t.dtype == torch.float32 and torch.equal(t, torch.full((3, 3), 2.5))
    assert torch.equal(LatentsDataset(lat, opts=None)[3], lat[3])


def test_test_options_defaults():
    from editing.styleclip_mapper.options.test_options import TestOptions
    o = TestOptions().parse(['--exp_dir', 'e'])
    assert o.mapper_type == 'LevelsMapper' and o.test_batch_size == 2 and o.n_images is None and o.stylegan_size == 1024
    assert not (o.no_coarse_mapper or o.no_medium_mapper or o.no_fine_mapper or o.couple_outputs)


# ---- run() / run_on_batch on an injected Rmini net --------------------------------------------------------------------

def make_net(case='levels_all'):
    o = cases.opts(case)
    net = torch.nn.Module()
    net.mapper = cases.build_mapper(o, cases.state_dict(o))
    net.decoder = build_product_generator('Rmini')
    return net.eval()


def run_opts(tmp_path, n, bs, n_images=None, transforms=False, couple=False):
    lat = torch.from_numpy(cases.latents(n))
    torch.save(lat, tmp_path / 'lat.pt')
    tpath = None
    if transforms:
        recs = np.empty(n, dtype=object)
        for i in range(n):
            a = 0.1 * i
            recs[i] = (i, None, None, np.array([[np.cos(a), -np.sin(a), 0.01 * i], [np.sin(a), np.cos(a), 0.0], [0, 0, 1]]))
        tpath = str(tmp_path / 'tr.npy')
        np.save(tpath, recs, allow_pickle=True)
    return types.SimpleNamespace(exp_dir=str(tmp_path / 'exp'), latents_test_path=str(tmp_path / 'lat.pt'), test_batch_size=bs,
                                 test_workers=0, fourier_features_transforms_path=tpath, n_images=n_images, couple_outputs=couple), lat


@pytest.mark.parametrize('n,bs,n_images,expect', [(7, 2, None, 6), (7, 3, 4, 6), (6, 2, 3, 4), (5, 2, 0, 0), (3, 4, None, 0)])
def test_run_item_set(tmp_path, n, bs, n_images, expect):
    from editing.styleclip_mapper.scripts import inference
    o, lat = run_opts(tmp_path, n, bs, n_images)
    net = make_net()
    written = inference.run(o, net=net)
    assert written == list(range(expect))
    files = sorted(os.listdir(os.path.join(o.exp_dir, 'inference_results')))
    assert files == [f'latent_{i:05d}.pt' for i in range(expect)]
    assert open(os.path.join(o.exp_dir, 'stats.txt')).read().startswith('Runtime ')
    with torch.no_grad():
        for i in range(expect):
            b0 = i - i % bs
            assert torch.equal(torch.load(os.path.join(o.exp_dir, 'inference_results', f'latent_{i:05d}.pt')),
                               net.mapper.edit(lat[b0:b0 + bs])[i - b0])


def test_run_on_batch_couple_outputs_and_transform():
    from editing.styleclip_mapper.scripts.inference import run_on_batch
    net = make_net()
    w = torch.from_numpy(cases.latents(2))
    a = torch.tensor([0.0, 0.3])
    t = torch.zeros(2, 3, 3)
    t[:, 0, 0], t[:, 0, 1], t[:, 1, 0], t[:, 1, 1], t[:, 2, 2] = a.cos(), -a.sin(), a.sin(), a.cos(), 1.0
    x_hat, w_hat, x = run_on_batch(w, t, net, couple_outputs=True)
    assert torch.equal(net.decoder.synthesis.input.transform, t)                 # left on the decoder
    with torch.no_grad():
        exp_w = w + 0.1 * net.mapper(w)
        assert torch.equal(w_hat, exp_w)
        assert torch.equal(x_hat, net.decoder.synthesis(exp_w))
        assert torch.equal(x, net.decoder.synthesis(w))
    assert not torch.equal(x_hat, x)
    two = run_on_batch(w, None, net)
    assert len(two) == 2 and torch.equal(two[1], w_hat) and torch.equal(net.decoder.synthesis.input.transform, t)


def _worker(rank, world, port, tmp, n, bs):
    for p in sys.path_extra:
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(2)
    from editing.styleclip_mapper.scripts import inference
    o = types.SimpleNamespace(exp_dir=os.path.join(tmp, 'dist'), latents_test_path=os.path.join(tmp, 'lat.pt'), test_batch_size=bs,
                              test_workers=0, fourier_features_transforms_path=os.path.join(tmp, 'tr.npy'), n_images=None, couple_outputs=False)
    inference.run(o, net=make_net())
    dist.barrier()
    dist.destroy_process_group()


sys.path_extra = [p for p in sys.path if 'stylegan3-editing_amd' in p or p.endswith('tests') or p.endswith('repo')]


def test_run_sharded_over_gloo_writes_the_single_process_files(tmp_path):
    from editing.styleclip_mapper.scripts import inference
    n, bs = 7, 2
    o, _ = run_opts(tmp_path, n, bs, transforms=True)
    inference.run(o, net=make_net())
    port = 29500 + (os.getpid() % 2000) + 57
    mp.spawn(_worker, args=(2, port, str(tmp_path), n, bs), nprocs=2, join=True)
    single = sorted(os.listdir(os.path.join(o.exp_dir, 'inference_results')))
    sharded = sorted(os.listdir(tmp_path / 'dist' / 'inference_results'))
    assert single == sharded == [f'latent_{i:05d}.pt' for i in range(6)]
    for f in single:
        assert torch.equal(torch.load(os.path.join(o.exp_dir, 'inference_results', f)), torch.load(tmp_path / 'dist' / 'inference_results' / f))
    assert (tmp_path / 'dist' / 'stats.txt').exists()


# ---- C entry point: struct layout and argument checks (no launch) -----------------------------------------------------

def test_latent_mapper_struct_matches_header():
    from torch_utils import _sg3abi
    src = open(os.path.join(ROOT, 'include', 'sg3_ops.h')).read()
    cname = 'sg3_latent_mapper_params'
    body = re.search(r'typedef struct ' + cname + r' \{(.*?)\} ' + cname + ';', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        parts = decl.split(',')
        for nm in [parts[0].split()[-1]] + [q.strip() for q in parts[1:]]:
            names.append(re.sub(r'\[\d+\]|\*', '', nm))
    assert names == [n for n, _ in _sg3abi.LatentMapperParams._fields_]
    assert dict(_sg3abi.LatentMapperParams._fields_)['levelBegin']._length_ == 4


def _params(**kw):
    from torch_utils import _sg3abi
    bufs = {k: ctypes.create_string_buffer(64) for k in ('x', 'out', 'delta', 'weight', 'bias', 'scratch')}
    p = _sg3abi.LatentMapperParams()
    for k, b in bufs.items():
        setattr(p, k, ctypes.addressof(b))
    p.N, p.L, p.D, p.groups, p.alpha = 2, 16, 512, 3, 0.1
    for g, (b, e) in enumerate([(0, 5), (5, 8), (8, 16)]):
        p.levelBegin[g], p.levelEnd[g] = b, e
    for k, v in kw.items():
        if k == 'levels':
            for g, (b, e) in enumerate(v):
                p.levelBegin[g], p.levelEnd[g] = b, e
        else:
            setattr(p, k, v)
    return p, bufs


@pytest.mark.parametrize('kw,msg', [
    (dict(x=None), 'null x'),
    (dict(out=None, delta=None), 'neither out nor delta'),
    (dict(weight=None), 'null weight'),
    (dict(scratch=None), 'null weight'),
    (dict(D=256), 'only 512'),
    (dict(N=0), 'bad shape'),
    (dict(groups=5), 'groups'),
    (dict(levels=[(0, 5), (5, 5), (8, 16)]), 'empty or out of range'),
    (dict(levels=[(0, 5), (5, 8), (8, 17)]), 'empty or out of range'),
    (dict(levels=[(0, 6), (5, 8), (8, 16)]), 'overlap'),
])
def test_latent_mapper_rejects_bad_arguments(kw, msg):
    from torch_utils import _sg3abi
    lib = _sg3abi.load()
    p, _keep = _params(**kw)
    before = _sg3abi.launch_count
    rc = lib.sg3_latent_mapper(ctypes.byref(p), None)
    assert rc < -1
    assert msg in _sg3abi.last_error()
    assert _sg3abi.launch_count == before
    assert lib.sg3_latent_mapper(None, None) < -1


def test_latent_mapper_rejects_overlapping_buffers():
    from torch_utils import _sg3abi
    lib = _sg3abi.load()
    p, keep = _params()
    p.out = p.x                                                             # written buffer on top of the input
    assert lib.sg3_latent_mapper(ctypes.byref(p), None) < -1 and 'overlap' in _sg3abi.last_error()
