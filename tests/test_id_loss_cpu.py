"""CPU: the IR-SE50 Backbone and the identity loss against golden vectors of the reference implementation
(tests/golden/make_golden_id_loss.py), the pool / crop / pool map as two banded matrices, the closed-form backward of a residual
unit that the HIP kernels implement, and the Coach building the loss from a checkpoint path."""
import argparse

import numpy as np
import pytest
import torch

import id_loss_cases as cases


@pytest.fixture(scope='module')
def golden():
    return np.load(cases.GOLDEN)


@pytest.fixture(scope='module')
def net():
    return cases.build_backbone('cpu')


def test_state_dict_keys_and_shapes_equal_the_manifest(net):
    man = cases.manifest()
    sd = net.state_dict()
    assert sorted(sd) == sorted(man)
    for k, v in sd.items():
        assert tuple(v.shape) == man[k], k
    assert any(k.startswith('input_layer.') for k in sd) and 'body.23.res_layer.5.fc2.weight' in sd
    assert {k.split('.')[1] for k in sd if k.startswith('output_layer.')} == {'0', '3', '4'}


def test_constructors():
    from models.setgan.encoder.encoders import model_irse as m
    assert len(m.IR_50(112).body) == 24 and len(m.IR_SE_50(112).body) == 24
    assert m.IR_SE_50(112).output_layer[4].weight is None                      # affine=False
    assert m.Backbone(224, 50).output_layer[3].in_features == 512 * 14 * 14
    with pytest.raises(AssertionError):
        m.Backbone(128, 50)


@pytest.mark.parametrize('name', ['s64', 's96'])
def test_id_loss_matches_the_reference_golden(net, golden, name):
    """float32 on the CPU against the reference in float64: at most twice the error of the reference's own float32 run (stored by
    the golden script) plus 1e-7 of the largest reference value."""
    from criteria.id_loss import IDLoss
    crit = IDLoss(facenet=net)
    x = torch.from_numpy(golden[f'{name}_x'])
    y = torch.from_numpy(golden[f'{name}_y']) if f'{name}_y' in golden else x
    y_hat = torch.from_numpy(golden[f'{name}_y_hat']).requires_grad_(True)
    loss, sim, logs = crit(y_hat, y, x)
    assert isinstance(loss, torch.Tensor) and loss.ndim == 0 and isinstance(sim, float) and isinstance(logs, list)
    assert all(sorted(d) == ['diff_input', 'diff_target', 'diff_views'] and all(isinstance(v, float) for v in d.values()) for d in logs)
    grad, = torch.autograd.grad(loss, y_hat)

    def bound(key, ref):
        return 2 * float(golden[f'{name}_{key}_err32']) + 1e-7 * float(np.abs(ref).max())

    with torch.no_grad():
        feats = torch.stack([crit.extract_feats(x), crit.extract_feats(y), crit.extract_feats(y_hat)]).double().numpy()
    ref = golden[f'{name}_feats']
    assert np.abs(feats - ref).max() <= bound('feats', ref)
    assert abs(float(loss) - float(golden[f'{name}_loss'])) <= bound('loss', golden[f'{name}_loss'])
    assert abs(sim - float(golden[f'{name}_sim'])) <= bound('sim', golden[f'{name}_logs'])      # a difference of two log values
    assert np.abs(cases.logs_array(logs) - golden[f'{name}_logs']).max() <= bound('logs', golden[f'{name}_logs'])
    ref = golden[f'{name}_grad']
    assert np.abs(grad.double().numpy() - ref).max() <= bound('grad', ref)


def test_shared_target_features_are_extracted_once(net, golden):
    from criteria.id_loss import IDLoss
    crit = IDLoss(facenet=net)
    x = torch.from_numpy(golden['s64_x'])
    y_hat = torch.from_numpy(golden['s64_y_hat'])
    calls = []
    extract = crit.extract_feats
    crit.extract_feats = lambda t: (calls.append(1), extract(t))[1]
    with torch.no_grad():
        a = crit(y_hat, x, x)
        n_same = len(calls)
        b = crit(y_hat, x.clone(), x)
    assert n_same == 2 and len(calls) == 5
    assert float(a[0]) == float(b[0]) and a[1] == b[1] and a[2] == b[2]


def test_features_of_x_and_y_are_constants(net, golden):
    from criteria.id_loss import IDLoss
    crit = IDLoss(facenet=net)
    x = torch.from_numpy(golden['s96_x']).requires_grad_(True)
    y_hat = torch.from_numpy(golden['s96_y_hat']).requires_grad_(True)
    loss, _, _ = crit(y_hat, x, x)
    gy, gx = torch.autograd.grad(loss, [y_hat, x], allow_unused=True)
    assert gx is None and gy is not None and float(gy.abs().max()) > 0


def test_idloss_needs_weights_or_a_module():
    from criteria.id_loss import IDLoss
    with pytest.raises(ValueError, match='ir_se50_weights'):
        IDLoss(argparse.Namespace())


@pytest.mark.parametrize('h', [64, 96, 256, 512, 1024])
def test_pool_matrices_equal_the_two_pools(h):
    from torch_utils.ops import face_pool as fp
    w = h if h != 512 else 384                                  # one case with unequal sides
    ay, ax = fp.matrices(h, w)
    assert ay.shape == (112, h) and ax.shape == (112, w)
    r = np.random.RandomState(h)
    x = torch.from_numpy(r.randn(1, 2, h, w))
    ref = cases.extract_feats(lambda t: t, x)
    out = torch.from_numpy(ay) @ x @ torch.from_numpy(ax).t()
    assert float((out - ref).abs().max()) <= 4e-15 * float(ref.abs().max() + 1)
    assert float((fp.composite(x) - ref).abs().max()) == 0
    taps = (ay != 0).sum(axis=1)
    assert taps.min() >= 1 and taps.max() <= {64: 2, 96: 2, 256: 3, 512: 6, 1024: 12}[h]
    # banded: the non-zeros of every row are contiguous, and nothing outside the crop's footprint is touched
    for m in (ay, ax):
        for row in m:
            nz = np.flatnonzero(row)
            assert nz[-1] - nz[0] + 1 == len(nz)
    assert abs(ay.sum(axis=1) - 1).max() < 1e-14 and abs(ax.sum(axis=1) - 1).max() < 1e-14


def test_face_pool_cpu_is_the_composite_and_differentiable():
    from torch_utils.ops.face_pool import face_pool
    x = cases.images(1, 64, 3).double().requires_grad_(True)
    y = face_pool(x)
    assert tuple(y.shape) == (1, 3, 112, 112)
    g, = torch.autograd.grad(y.sum(), x)
    from torch_utils.ops.face_pool import matrices
    ay, ax = matrices(64, 64)
    ref = np.outer(ay.sum(axis=0), ax.sum(axis=0))
    assert np.abs(g[0, 0].numpy() - ref).max() < 1e-13


@pytest.mark.parametrize('shape', cases.UNIT_SHAPES)
@pytest.mark.parametrize('negate', [False, True])
def test_unit_backward_closed_form_equals_float64_autograd(shape, negate):
    cin, depth, stride, h, w = shape
    unit = cases.build_unit(cin, depth, stride, negate=negate)
    r = np.random.RandomState(cin + depth + h)
    x = torch.from_numpy(r.randn(2, cin, h, w)).requires_grad_(True)
    out = unit(x)
    dout = torch.from_numpy(r.randn(*out.shape))
    ref, = torch.autograd.grad(out, x, dout)
    got = cases.unit_backward_closed_form(unit, x.detach(), dout)
    assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    if negate:
        # what the closed form must NOT do: read the PReLU branch from the sign of the saved output
        bn1, conv1, prelu = unit.res_layer[0], unit.res_layer[1], unit.res_layer[2]
        pre = conv1(bn1(x.detach()))
        assert float(((prelu(pre) > 0) != (pre > 0)).double().mean()) > 0.05


def test_coach_builds_the_id_loss_from_a_checkpoint_path(tmp_path, net):
    from criteria.id_loss import IDLoss
    from editing.styleclip_mapper.training.coach import Coach
    import test_styleclip_mapper_train_cpu as t
    path = tmp_path / 'model_ir_se50.pth'
    torch.save(net.state_dict(), path)
    tokens = torch.zeros(1, 4, dtype=torch.long)
    o = t._stub_opts(tmp_path, id_lambda=0.06, ir_se50_weights=str(path))
    coach = Coach(o, net=t._stub_net(o), clip_loss=t._stub_clip_loss, text_tokens=tokens)
    assert isinstance(coach.id_loss, IDLoss) and not coach.id_loss.facenet.training
    # frozen when loaded from a path: the condition of the HIP path, and no weight gradient is ever built for it
    assert not any(q.requires_grad for q in coach.id_loss.parameters()) and coach.id_loss.facenet.hip_ready()
    assert torch.equal(coach.id_loss.facenet.body[3].res_layer[1].weight, net.body[3].res_layer[1].weight)
    w = next(iter(coach.train_dataloader))
    x = coach.net.decoder.synthesis(w).detach()
    w_hat = coach.edit(w)
    loss, d = coach.calc_loss(w, x, w_hat, coach.net.decoder.synthesis(w_hat))
    assert np.isfinite(float(d['loss_id'])) and np.isfinite(float(d['id_improve'])) and loss.requires_grad
    loss.backward()
    assert all(q.grad is None for q in coach.id_loss.parameters()) and any(q.grad is not None for q in coach.net.mapper.parameters())
    # without a file the message of old stays: a default path that does not exist, or no path at all
    for missing in (str(tmp_path / 'missing.pth'), '/path/to/model_ir_se50.pth', None):
        o2 = t._stub_opts(tmp_path, id_lambda=0.06, ir_se50_weights=missing)
        with pytest.raises(NotImplementedError, match='--id_lambda 0'):
            Coach(o2, net=t._stub_net(o2), clip_loss=t._stub_clip_loss, text_tokens=tokens)
