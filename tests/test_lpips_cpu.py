"""The LPIPS criterion without a GPU: state-dict layout against the reference's manifest, the weight routes, the composite against
the golden values of the reference (float64 to 1e-10 relative, float32 within twice the reference's own float32 deviation), the size
limit, and PTI built from the two weight options."""
import json

import numpy as np
import pytest
import torch

import lpips_cases as cases


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(cases.GOLDEN))


def test_state_dict_matches_the_reference_manifest():
    from criteria.lpips import LPIPS
    from criteria.lpips.networks import AlexNet, BaseNet, LinLayers
    m = LPIPS(pretrained=False)
    with open(cases.MANIFEST) as f:
        man = json.load(f)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == man
    assert list(m.state_dict().keys()) == list(man.keys())
    assert isinstance(m.net, AlexNet) and isinstance(m.net, BaseNet) and isinstance(m.lin, LinLayers)
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    assert all(p.device.type == 'cpu' for p in m.parameters())
    assert m.net.mean.flatten().tolist() == pytest.approx(cases.MEAN) and m.net.std.flatten().tolist() == pytest.approx(cases.STD)


def test_upstream_style_weights_load_strictly(tmp_path):
    """torchvision's `features.N.*` (classifier ignored) and the published `lin{k}.model.1.weight`, as dicts and as files; the
    renamed linear keys too."""
    from criteria.lpips import LPIPS
    from criteria.lpips.utils import get_state_dict
    sd = cases.state_dict()
    alex, lin = cases.upstream_dicts(sd)
    assert any(k.startswith('classifier.') for k in alex) and 'lin0.model.1.weight' in lin
    assert list(get_state_dict(lin).keys()) == [f'{i}.1.weight' for i in range(5)]
    torch.save(alex, tmp_path / 'alexnet.pth')
    torch.save(lin, tmp_path / 'alex_lin.pth')
    renamed = {k[4:]: v for k, v in sd.items() if k.startswith('lin.')}
    for a, l in ((alex, lin), (str(tmp_path / 'alexnet.pth'), str(tmp_path / 'alex_lin.pth')), (alex, renamed)):
        m = LPIPS(net_type='alex', alexnet_weights=a, lin_weights=l)
        got = m.state_dict()
        assert list(got.keys()) == list(sd.keys())
        for k in sd:
            assert torch.equal(got[k], sd[k]), k
        assert not m.training and not any(p.requires_grad for p in m.parameters())
    broken = dict(alex)
    del broken['features.3.bias']
    with pytest.raises(RuntimeError):
        LPIPS(alexnet_weights=broken, lin_weights=lin)


def test_constructor_errors():
    from criteria.lpips import LPIPS
    alex, lin = cases.upstream_dicts(cases.state_dict())
    for kw in ({}, {'alexnet_weights': alex}, {'lin_weights': lin}):
        with pytest.raises(ValueError, match='alexnet_weights.*lin_weights'):
            LPIPS(**kw)
    for net_type in ('vgg', 'squeeze'):
        with pytest.raises(NotImplementedError):
            LPIPS(net_type=net_type, alexnet_weights=alex, lin_weights=lin)


@pytest.mark.parametrize('name', list(cases.CASES))
def test_composite_reproduces_the_reference(golden, name):
    x, y = torch.from_numpy(golden[f'{name}_x']), torch.from_numpy(golden[f'{name}_y'])
    gx, gy = cases.case_inputs(name)
    assert torch.equal(x, gx) and torch.equal(y, gy)
    ref = {k: golden[f'{name}_{k}'] for k in ('loss', 'terms', 'grad')}
    m64 = cases.build(torch.float64)
    assert cases.min_pixel_norm(m64.net, x.double()) > 0.5 and cases.min_pixel_norm(m64.net, y.double()) > 0.5
    assert not m64.uses_hip(x.double())
    x64 = x.double().requires_grad_(True)
    loss = m64(x64, y.double())
    assert loss.ndim == 0 and loss.dtype == torch.float64
    grad, = torch.autograd.grad(loss, x64)
    terms = m64.layer_terms(x.double(), y.double())
    for key, got in (('loss', loss.detach()), ('terms', terms), ('grad', grad)):
        err, top = float(np.abs(got.numpy() - ref[key]).max()), float(np.abs(ref[key]).max())
        print(f'{name} float64 {key}: err {err:.3e} of {top:.3e}')
        assert err <= 1e-10 * top, key
    m32 = cases.build(torch.float32)
    assert not m32.uses_hip(x)
    x32 = x.clone().requires_grad_(True)
    loss = m32(x32, y)
    assert loss.ndim == 0 and loss.dtype == torch.float32
    grad, = torch.autograd.grad(loss, x32)
    terms = m32.layer_terms(x, y)
    for key, got in (('loss', loss.detach()), ('terms', terms), ('grad', grad)):
        err = float(np.abs(got.double().numpy() - ref[key]).max())
        bound = cases.whole_bound(golden[f'{name}_{key}_err32'], ref[key])
        print(f'{name} float32 {key}: err {err:.3e} bound {bound:.3e}')
        assert err <= bound, key


def test_images_below_31_pixels_are_refused():
    m = cases.build()
    for h, w in ((30, 64), (64, 30), (8, 8)):
        x = cases.images(1, h, w, seed=1)
        with pytest.raises(RuntimeError, match='at least 31'):
            m(x, x)
    x = cases.images(1, 31, 31, seed=2)
    assert float(m(x, cases.perturbed(x, seed=3))) > 0
    with pytest.raises(RuntimeError):
        m(x, cases.images(1, 31, 33, seed=2))


def _pti_target(res, seed):
    r = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.linspace(-1, 1, res), np.linspace(-1, 1, res), indexing='ij')
    base = np.stack([np.sin(3 * xx + s) * np.cos(2 * yy - s) for s in (0.0, 0.7, 1.9)])
    return (0.6 * base + 0.05 * r.randn(3, res, res)).astype(np.float32)


def _tunable_generator(cfg, device='cpu'):
    from helpers import build_product_generator
    G = build_product_generator(cfg, device=device)
    G.requires_grad_(True)
    return G


def test_pti_builds_the_criterion_from_the_weight_options(tmp_path):
    from criteria.lpips import LPIPS
    from inversion.scripts.run_pti_images import PTI, default_opts
    from inversion.video.run_pti_video import VideoPTI
    from synth_weights import synth_ws
    alex, lin = cases.upstream_dicts(cases.state_dict())
    torch.save(alex, tmp_path / 'alexnet.pth')
    torch.save(lin, tmp_path / 'alex_lin.pth')
    G = _tunable_generator('Ttiny')
    ws = synth_ws(1, G.num_ws, G.w_dim, seed=6)[0]
    target = _pti_target(64, 40)
    histories = []
    for a, l in ((alex, lin), (str(tmp_path / 'alexnet.pth'), str(tmp_path / 'alex_lin.pth'))):
        pti = PTI(default_opts(device='cpu', steps=2, lpips_threshold=0.0, lpips_alexnet_weights=a, lpips_lin_weights=l))
        assert isinstance(pti.lpips_loss, LPIPS)
        pti.optimize_model(_tunable_generator('Ttiny'), ws, target)
        assert len(pti.history) == 2 and all(h[2] is not None and np.isfinite(h[2]) and h[2] > 0 for h in pti.history)
        histories.append(pti.history)
    assert histories[0] == histories[1]
    # the value PTI recorded at step 0 is the criterion's on the untouched generator's image
    with torch.no_grad():
        img = G.synthesis(torch.from_numpy(np.asarray(ws)).unsqueeze(0), noise_mode='const', force_fp32=True)
        want = float(cases.build()(img, torch.from_numpy(np.asarray(target)).float().unsqueeze(0)))
    assert histories[0][0][2] == pytest.approx(want, rel=1e-5)
    # a callable still wins, the video tuner inherits the rule, and nothing changes without the options
    marker = lambda a, b: (a - b).abs().mean()          # noqa: E731
    assert PTI(default_opts(device='cpu', lpips_alexnet_weights=alex, lpips_lin_weights=lin), lpips_loss=marker).lpips_loss is marker
    assert isinstance(VideoPTI(default_opts(device='cpu', lpips_alexnet_weights=alex, lpips_lin_weights=lin)).lpips_loss, LPIPS)
    assert PTI(default_opts(device='cpu', lpips_lambda=0.0, lpips_alexnet_weights=alex, lpips_lin_weights=lin)).lpips_loss is None


def test_pti_without_callable_or_options_still_raises():
    from inversion.scripts.run_pti_images import PTI, default_opts
    alex, lin = cases.upstream_dicts(cases.state_dict())
    for kw in ({}, {'lpips_alexnet_weights': alex}, {'lpips_lin_weights': lin}):
        with pytest.raises(RuntimeError):
            PTI(default_opts(device='cpu', **kw))
