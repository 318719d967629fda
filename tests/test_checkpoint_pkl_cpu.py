"""CPU: official-style `.pkl` checkpoints through `SG3Generator` -- a generator unpickled from foreign module source is
adopted onto this package's `Generator`, a training snapshot (`G`, `D`, `G_ema`, `augment_pipe`, `training_set_kwargs`)
unpickles whole, and the operator modules a snapshot's sources import (`conv2d_resample`, `fma`, `grid_sample_gradfix`)
compute what the reference's compute.

No pickle made from the reference's classes is committed (it would carry the reference's source): the foreign side is
tests/foreign_generator_src.py, pinned to the reference's images in tests/golden/net_tiny.npz, and -- where the reference
is mounted -- pickles made from it at test time in a child process."""
import io
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from ckpt_cases import CONV2D_RESAMPLE_CASES, RESAMPLE_FILTER, conv2d_resample_inputs, fma_inputs, grid_sample_inputs
from ckpt_helpers import (EXTRA_BUFFER_HOOK, sg3_from_state_dict, source_text, standin_discriminator, standin_generator,
                          write_pickle, write_state_dict)
from helpers import golden, maxabs
from synth_weights import CONFIGS, synth_ws

REFERENCE = os.environ.get('SG3_REFERENCE_ROOT', '/root/reference')
TINY_IMAGE_TOL = 1e-6       # what tests/test_product_cpu.py::test_tiny_network_ref_path asks of the product's image
OP_TOL = 1e-6               # what tests/test_product_cpu.py::test_upfirdn2d_ref_path asks


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def image(G, ws):
    with torch.no_grad():
        return G.synthesis(ws, noise_mode='const', force_fp32=True)


def load(path, **kw):
    from models.stylegan3.model import SG3Generator
    return SG3Generator(checkpoint_path=str(path), device='cpu', **kw).decoder


def native_class():
    from models.stylegan3.networks_stylegan3 import Generator
    return Generator


@pytest.mark.parametrize('cfg', ['Ttiny', 'Rtiny'])
def test_standin_source_meets_the_reference_images(cfg):
    """The stand-in's forward is the reference's forward: same golden images, same tolerance as the product's own CPU test."""
    g = golden('net_tiny')
    G = standin_generator(cfg)
    assert type(G).__module__.startswith('_imported_module_') and type(G) is not native_class()
    ws = T(synth_ws(2, G.num_ws, G.w_dim, seed=1))
    assert maxabs(image(G, ws).numpy(), g[cfg + '/img']) <= TINY_IMAGE_TOL
    z = T(np.random.RandomState(5).randn(3, G.z_dim).astype(np.float32))
    with torch.no_grad():
        assert maxabs(G(z[:1], None, truncation_psi=0.7).numpy(), g[cfg + '/gen_psi07']) <= TINY_IMAGE_TOL


@pytest.mark.parametrize('cfg', ['Ttiny', 'Rtiny'])
def test_foreign_pickle_is_adopted(cfg, tmp_path):
    foreign = standin_generator(cfg)
    foreign.mapping.fc0.weight.requires_grad_(True)            # one flag that differs from the rest must survive
    ws = T(synth_ws(2, foreign.num_ws, foreign.w_dim, seed=1))
    pkl = write_pickle(tmp_path / 'g.pkl', G_ema=foreign)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        G = load(pkl)
    assert type(G) is native_class()
    from_pt = sg3_from_state_dict(write_state_dict(tmp_path / 'g.pt', foreign), cfg)
    assert type(from_pt) is native_class()
    img = image(G, ws)
    assert torch.equal(img, image(from_pt, ws))
    assert dict(G.init_kwargs) == dict(foreign.init_kwargs) == CONFIGS[cfg]
    assert not G.training and all(not m.training for m in G.modules())
    flags = {n: p.requires_grad for n, p in G.named_parameters()}
    assert flags == {n: p.requires_grad for n, p in foreign.named_parameters()}
    assert flags['mapping.fc0.weight'] and sum(flags.values()) == 1
    assert all(p.dtype == torch.float32 for p in G.parameters())
    # re-pickling writes this package's source, and that loads as the native class again
    buf = io.BytesIO()
    pickle.dump(dict(G_ema=G), buf)
    assert b'def synthesis_schedule' in buf.getvalue() and b'conv2d_gradfix.conv2d(input=x.reshape' not in buf.getvalue()
    again = write_pickle(tmp_path / 'again.pkl', G_ema=G)
    G2 = load(again)
    assert type(G2) is native_class() and torch.equal(image(G2, ws), img)


def test_adoption_carries_mode_and_dtype(tmp_path):
    """Train mode and a non-default dtype come over with the weights."""
    foreign = standin_generator('Ttiny').train().requires_grad_(True).to(torch.float64)
    G = load(write_pickle(tmp_path / 'g.pkl', G_ema=foreign))
    assert type(G) is native_class() and G.training
    assert all(p.requires_grad and p.dtype == torch.float64 for p in G.parameters())
    assert all(b.dtype == torch.float64 for b in G.buffers())
    assert torch.equal(G.synthesis.L3_36_12.weight, foreign.synthesis.L3_36_12.weight)


def test_snapshot_layout_loads(tmp_path):
    """The upstream snapshot layout: `D`'s source imports conv2d_resample / fma / grid_sample_gradfix while unpickling."""
    foreign = standin_generator('Ttiny')
    D = standin_discriminator()
    ws = T(synth_ws(1, foreign.num_ws, foreign.w_dim, seed=1))
    want = image(foreign, ws)
    pkl = write_pickle(tmp_path / 'network-snapshot.pkl', G=foreign, D=D, G_ema=foreign, augment_pipe=None,
                       training_set_kwargs=dict(path='ffhq.zip', resolution=64, use_labels=False))
    G = load(pkl)
    assert type(G) is native_class()
    assert maxabs(image(G, ws).numpy(), want.numpy()) <= TINY_IMAGE_TOL
    with open(pkl, 'rb') as fh:
        snap = pickle.load(fh)
    assert set(snap) == {'G', 'D', 'G_ema', 'augment_pipe', 'training_set_kwargs'}
    with torch.no_grad():
        score = snap['D'](want)
        assert score.shape == (1, 1) and bool(torch.isfinite(score).all())
        assert torch.equal(score, D(want))


@pytest.mark.parametrize('cfg', ['Ttiny', 'Rtiny'])
def test_opting_out_returns_the_foreign_object(cfg, tmp_path):
    foreign = standin_generator(cfg)
    ws = T(synth_ws(2, foreign.num_ws, foreign.w_dim, seed=1))
    pkl = write_pickle(tmp_path / 'g.pkl', G_ema=foreign)
    kept = load(pkl, adopt=False)
    assert type(kept) is type(foreign) and type(kept) is not native_class()
    assert maxabs(image(kept, ws).numpy(), image(load(pkl), ws).numpy()) <= TINY_IMAGE_TOL


def _variants():
    text = source_text()
    assert EXTRA_BUFFER_HOOK in text and 'class Generator(' in text
    return {
        'unknown_kwarg': (None, 'Generator', dict(standin_only=1), 'standin_only'),
        'extra_buffer': (text.replace(EXTRA_BUFFER_HOOK, "self.register_buffer('extra_stat', torch.zeros([3]))"), 'Generator', {}, 'extra_stat'),
        'other_class_name': (text.replace('class Generator(', 'class GeneratorV2('), 'GeneratorV2', {}, 'GeneratorV2'),
    }


@pytest.mark.parametrize('variant', ['unknown_kwarg', 'extra_buffer', 'other_class_name'])
def test_unadoptable_generators_fall_through_with_one_warning(variant, tmp_path):
    text, class_name, extra, word = _variants()[variant]
    foreign = standin_generator('Ttiny', text=text, class_name=class_name, **extra)
    ws = T(synth_ws(1, foreign.num_ws, foreign.w_dim, seed=1))
    pkl = write_pickle(tmp_path / 'g.pkl', G_ema=foreign)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        G = load(pkl)
    assert type(G) is type(foreign) and type(G) is not native_class()
    assert len(caught) == 1 and 'not adopted' in str(caught[0].message) and word in str(caught[0].message)
    assert torch.equal(image(G, ws), image(foreign, ws))


def test_helper_leaves_native_and_opted_out_objects_alone():
    from helpers import build_product_generator
    from models.stylegan3.model import adopt_generator
    G = build_product_generator('Ttiny')
    foreign = standin_generator('Ttiny')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert adopt_generator(G) is G
        assert adopt_generator(foreign, adopt=False) is foreign
        assert type(adopt_generator(foreign)) is native_class()


_CHILD = r'''
import pickle, sys
import numpy as np
ref_root, tests_dir, out_dir = sys.argv[1:4]
sys.path.insert(0, tests_dir)
sys.path.insert(0, ref_root)
import torch
from synth_weights import CONFIGS, synth_state_dict, synth_ws
from models.stylegan3.networks_stylegan3 import Generator
for cfg in ('Ttiny', 'Rtiny'):
    G = Generator(**CONFIGS[cfg])
    man = {k: list(v.shape) for k, v in G.state_dict().items()}
    sd = synth_state_dict(man, seed=0, input_bandwidth=float(G.synthesis.input.bandwidth))
    G.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    G = G.eval().requires_grad_(False)
    with open(f'{out_dir}/{cfg}.pkl', 'wb') as fh:
        pickle.dump(dict(G_ema=G), fh)
    ws = torch.from_numpy(synth_ws(2, G.num_ws, G.w_dim, seed=1))
    with torch.no_grad():
        np.save(f'{out_dir}/{cfg}.npy', G.synthesis(ws, noise_mode='const', force_fp32=True).numpy())
'''


@pytest.fixture(scope='module')
def reference_pickles(tmp_path_factory):
    """Pickles of the reference's own `Generator` (T and R at 64^2) and its images, made in a fresh interpreter so that the
    reference's `torch_utils` and this package's never share one."""
    if not os.path.isfile(os.path.join(REFERENCE, 'models', 'stylegan3', 'networks_stylegan3.py')):
        pytest.skip('the reference is not mounted')
    out = tmp_path_factory.mktemp('reference_pickles')
    env = {k: v for k, v in os.environ.items() if k != 'PYTHONPATH'}
    subprocess.run([sys.executable, '-c', _CHILD, REFERENCE, os.path.dirname(os.path.abspath(__file__)), str(out)], check=True, env=env,
                   cwd=str(out))
    return out


@pytest.mark.parametrize('cfg', ['Ttiny', 'Rtiny'])
def test_reference_pickle_is_adopted_and_equals_the_reference_forward(cfg, reference_pickles):
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        G = load(reference_pickles / f'{cfg}.pkl')
    assert type(G) is native_class()
    ws = T(synth_ws(2, G.num_ws, G.w_dim, seed=1))
    assert torch.equal(image(G, ws), T(np.load(reference_pickles / f'{cfg}.npy')))
    foreign = load(reference_pickles / f'{cfg}.pkl', adopt=False)
    assert type(foreign).__module__.startswith('_imported_module_')


# ---------------------------------------------------------------------------------------------------------------------
# the operator modules a snapshot's sources import

def _resample(c, x, w, f):
    from torch_utils.ops import conv2d_resample
    return conv2d_resample.conv2d_resample(x, w, f=f, up=c['up'], down=c['down'], padding=c['padding'], groups=c['groups'],
                                           flip_weight=c['flip_weight'])


@pytest.mark.parametrize('name', sorted(CONV2D_RESAMPLE_CASES))
def test_conv2d_resample_against_the_reference(name):
    from torch_utils.ops import upfirdn2d
    c = CONV2D_RESAMPLE_CASES[name]
    x, w = (T(a) for a in conv2d_resample_inputs(c))
    y = _resample(c, x, w, upfirdn2d.setup_filter(RESAMPLE_FILTER))
    want = golden('ckpt_ops')['conv2d_resample/' + name]
    assert tuple(y.shape) == want.shape
    assert maxabs(y.numpy(), want) <= OP_TOL


@pytest.mark.parametrize('name', sorted(CONV2D_RESAMPLE_CASES))
def test_conv2d_resample_equals_the_plain_composition(name):
    """Whatever ordering the op picks: zero-insert + pad + filter (gain up^2), convolve, filter + decimate -- in fp64."""
    from torch_utils.ops import upfirdn2d
    c = CONV2D_RESAMPLE_CASES[name]
    x, w = (T(a) for a in conv2d_resample_inputs(c, dtype=np.float64))
    f = upfirdn2d.setup_filter(RESAMPLE_FILTER)
    up, down, p = c['up'], c['down'], c['padding']
    fw = len(RESAMPLE_FILTER)
    lo = hi = p
    if up > 1:
        lo, hi = lo + (fw + up - 1) // 2, hi + (fw - up) // 2
    if down > 1:
        lo, hi = lo + (fw - down + 1) // 2, hi + (fw - down) // 2
    t = upfirdn2d.upfirdn2d(x, f if up > 1 else None, up=up, padding=[lo, hi, lo, hi], gain=up ** 2, impl='ref')
    t = torch.nn.functional.conv2d(t, w if c['flip_weight'] else w.flip([2, 3]), groups=c['groups'])
    if down > 1:
        t = upfirdn2d.upfirdn2d(t, f, down=down, impl='ref')
    y = _resample(c, x, w, f)
    assert y.shape == t.shape and maxabs(y.numpy(), t.numpy()) <= 1e-12


@pytest.mark.parametrize('name', sorted(CONV2D_RESAMPLE_CASES))
def test_conv2d_resample_gradcheck(name):
    from torch_utils.ops import upfirdn2d
    c = CONV2D_RESAMPLE_CASES[name]
    x, w = (T(a).requires_grad_(True) for a in conv2d_resample_inputs(c, h=5, w=6, dtype=np.float64))
    f = upfirdn2d.setup_filter(RESAMPLE_FILTER)
    assert torch.autograd.gradcheck(lambda x_, w_: _resample(c, x_, w_, f), (x, w))


def test_fma_against_the_reference_and_gradients():
    from torch_utils.ops import fma
    a, b, c = (T(v) for v in fma_inputs())
    y = fma.fma(a, b, c)
    assert maxabs(y.numpy(), golden('ckpt_ops')['fma']) <= OP_TOL and torch.equal(y, torch.addcmul(c, a, b))
    a, b, c = (T(v).requires_grad_(True) for v in fma_inputs(dtype=np.float64, spatial=(5, 6)))
    ga, gb, gc = torch.autograd.grad(fma.fma(a, b, c).sum(), (a, b, c))
    assert ga.shape == a.shape and gb.shape == b.shape and gc.shape == c.shape       # reduced back to each operand
    assert torch.autograd.gradcheck(fma.fma, (a, b, c))
    assert torch.autograd.gradgradcheck(fma.fma, (a, b, c))


def test_grid_sample_against_the_reference_and_gradients():
    from torch_utils.ops import grid_sample_gradfix as gs
    img, grid = (T(v) for v in grid_sample_inputs())
    want = golden('ckpt_ops')['grid_sample']
    assert gs.enabled is False
    assert maxabs(gs.grid_sample(img, grid).numpy(), want) <= OP_TOL
    gs.enabled = True
    try:
        assert maxabs(gs.grid_sample(img, grid).numpy(), want) <= OP_TOL
        assert float((gs.grid_sample(img, grid) == 0).float().mean()) > 0.02       # some samples fall in the zero padding
        img, grid = (T(v).requires_grad_(True) for v in grid_sample_inputs(dtype=np.float64, hw=(5, 6)))
        assert torch.autograd.gradcheck(gs.grid_sample, (img, grid))
        assert torch.autograd.gradgradcheck(gs.grid_sample, (img, grid))
    finally:
        gs.enabled = False
    # the library's own op agrees with the written-out one on first derivatives
    gi, gg = torch.autograd.grad(gs.grid_sample(img, grid).square().sum(), (img, grid))
    gs.enabled = True
    try:
        hi, hg = torch.autograd.grad(gs.grid_sample(img, grid).square().sum(), (img, grid))
    finally:
        gs.enabled = False
    assert maxabs(gi.numpy(), hi.numpy()) <= 1e-12 and maxabs(gg.numpy(), hg.numpy()) <= 1e-12


def test_names_pickled_sources_use_exist():
    from torch_utils import misc, persistence
    from torch_utils.ops import conv2d_resample, fma, grid_sample_gradfix
    for name in ('constant', 'assert_shape', 'profiled_function', 'suppress_tracer_warnings', 'copy_params_and_buffers'):
        assert callable(getattr(misc, name))
    for name in ('persistent_class', 'is_persistent', 'import_hook', '_reconstruct_persistent_obj'):
        assert callable(getattr(persistence, name))
    assert callable(conv2d_resample.conv2d_resample)
    assert callable(fma.fma) and callable(grid_sample_gradfix.grid_sample) and grid_sample_gradfix.enabled is False
