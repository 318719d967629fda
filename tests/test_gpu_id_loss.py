"""The identity loss on the GPU: the fused image preparation and its adjoint, the data-gradient convolution alone against float64
with the element-wise bound of the GEMM tests, the squeeze-and-excitation backward alone, one residual unit recorded and
differentiated, and the whole loss (golden at 64 x 64, float64 autograd on the device at 256 and 1024) with the composite's float32
autograd on the same device as the yardstick; launch counts, repeatability, batch invariance, the overflow repeat, a shared leaf,
and one Coach step with the reference's id_lambda.

General rule: |hip - fp64| <= 2 max|torch32 - fp64| + 1e-7 max|fp64|.  Measured on an MI355X: see DESIGN.md 3.11."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import id_loss_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U32 = 2.0 ** -24
# e_hip / e_torch32 of the image gradient under the split-precision recording forward: twice the largest ratio measured on an
# MI355X over the whole-loss cases below, rounded up to a power of two, capped at 16.  Measured: 0.51 (64 x 64), 0.01 (256 x 256),
# 1.18 (1024 x 1024); 2 x 1.18 = 2.4 -> 4
GRAD_FACTOR = 4


def _abi():
    from torch_utils import _sg3abi as abi
    return abi


def _randn(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape)).to(DEV)          # float64


def _no_miopen():
    return torch.backends.cudnn.flags(enabled=False)             # the torch yardsticks: no MIOpen search per convolution shape


# ---- 1. face_pool ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('H', [64, 96, 256, 512, 1024])
def test_face_pool_forward_and_adjoint_against_fp64(H):
    """Forward and adjoint on strided views, one launch each; the adjoint bit-equal on repeat and exactly zero where float64's is."""
    from torch_utils.ops.face_pool import composite, face_pool
    abi = _abi()
    B = 1 if H >= 1024 else 2
    base = _randn(H, B, 3, H + 1, H + 2).float()
    x = base[:, :, 1:, 1:-1]
    assert not x.is_contiguous()
    x64 = x.double().requires_grad_(True)
    x32 = x.detach().clone().requires_grad_(True)
    xh = x.detach().requires_grad_(True)
    y64, y32 = composite(x64), composite(x32)
    before = abi.launch_count
    yh = face_pool(xh)
    assert abi.launch_count - before == 1
    assert yh.dtype == torch.float32 and tuple(yh.shape) == tuple(y64.shape) == (B, 3, 112, 112)
    e_hip, e_t32 = float((yh.double() - y64).abs().max()), float((y32.double() - y64).abs().max())
    print(f'face_pool {H}: forward e_hip {e_hip:.3e} e_torch32 {e_t32:.3e}')
    assert e_hip <= 2 * e_t32 + 1e-7 * float(y64.abs().max())
    dy = _randn(H + 1, B, 3, 112, 113).float()[..., :-1]
    g64, = torch.autograd.grad(y64, x64, dy.double())
    g32, = torch.autograd.grad(y32, x32, dy)
    before = abi.launch_count
    gh, = torch.autograd.grad(yh, xh, dy, retain_graph=True)
    assert abi.launch_count - before == 1
    gh2, = torch.autograd.grad(yh, xh, dy)
    assert torch.equal(gh, gh2)
    e_hip, e_t32 = float((gh.double() - g64).abs().max()), float((g32.double() - g64).abs().max())
    print(f'face_pool {H}: adjoint e_hip {e_hip:.3e} e_torch32 {e_t32:.3e}')
    assert e_hip <= 2 * e_t32 + 1e-7 * float(g64.abs().max())
    assert bool((g64 == 0).any()) and bool((gh[g64 == 0] == 0).all()) and bool((gh[g64 != 0] != 0).all())


# ---- 2. sg3_conv2d_dgrad alone ------------------------------------------------------------------------------------------------------

# (k, stride, I, O, H, W): the issue's shapes, then sizes that are no multiple of a tile (channels, K chunk, more than one column tile)
DGRAD_SHAPES = [(3, 2, 64, 64, 13, 9), (3, 2, 64, 64, 20, 24), (3, 2, 128, 128, 7, 7), (3, 2, 128, 128, 14, 14),
                (1, 2, 64, 128, 13, 9), (1, 2, 64, 128, 20, 24), (3, 1, 64, 64, 9, 13), (3, 1, 3, 64, 12, 12),
                (3, 1, 40, 20, 5, 70), (3, 2, 40, 20, 7, 131), (1, 1, 40, 20, 5, 70), (1, 2, 70, 20, 6, 67),
                # two x tiles, a ragged last chunk, unequal parity classes.  That the list reaches all eight kernels (two tiles per
                # (k, stride)) is checked without a GPU: tests/test_conv2d_dispatch_cpu.py::test_gpu_case_lists_reach_every_kernel
                (3, 2, 3, 20, 7, 35), (1, 1, 3, 20, 5, 35), (1, 2, 3, 20, 6, 35)]
GUARD = 4096
SENTINEL = 777.0


def _conv_transpose64(dy, w, stride, hw):
    k = w.shape[2]
    pad = k // 2
    op = tuple(n - ((o - 1) * stride - 2 * pad + k) for n, o in zip(hw, dy.shape[2:]))
    return F.conv_transpose2d(dy, w, stride=stride, padding=pad, output_padding=op)


@pytest.mark.parametrize('k,stride,I,O,H,W', DGRAD_SHAPES)
@pytest.mark.parametrize('mag', [1.0, 1e-6])
def test_conv2d_dgrad_against_fp64(k, stride, I, O, H, W, mag):
    """Against float64 conv_transpose2d with output_padding, element by element:
        |hip - ref| <= (K + 2) 2^-24 (|dy| * |w|) (+ 2^-24 |addend|),   K = O x the most taps any pixel parity accumulates,
    plain, then with the PReLU-derivative and addend epilogues.  Upstream gradients of magnitude 1e-6 meet the same relative bound:
    a split-precision operand would leave an absolute floor near 2^-23.  The memory around the output stays untouched."""
    from torch_utils.ops.plain_conv_grad import PackedDgrad
    abi = _abi()
    N = 2
    seed = k * 1000 + stride * 100 + I + H
    w = (_randn(seed, O, I, k, k) / np.sqrt(I * k * k)).float()
    oh, ow = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    dy = (_randn(seed + 1, N, O, oh, ow) * mag).float()
    pd = PackedDgrad(w, stride=stride)
    assert pd.out_size(H, W) == (oh, ow)
    K = O * (k * k if stride == 1 else (4 if k == 3 else 1))
    ref = _conv_transpose64(dy.double(), w.double(), stride, (H, W))
    mags = _conv_transpose64(dy.double().abs(), w.double().abs(), stride, (H, W))
    buf = torch.full([N * I * H * W + 2 * GUARD], SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[GUARD:-GUARD].view(N, I, H, W)
    before = abi.launch_count
    got = pd.run(dy, (H, W), out=out)
    assert abi.launch_count - before == 1 and got.data_ptr() == out.data_ptr()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    err = (got.double() - ref).abs()
    bound = (K + 2) * U32 * mags
    print(f'dgrad k{k} s{stride} {I}<-{O} {H}x{W} mag {mag:g}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, max|ref| {float(ref.abs().max()):.3e}')
    assert bool((err <= bound).all())
    if stride == 2 and k == 1:
        assert bool((got[:, :, 1::2] == 0).all()) and bool((got[:, :, :, 1::2] == 0).all())
    # epilogues: addend through element strides (a transposed layout), then the PReLU derivative from a saved activation
    addend = (_randn(seed + 2, N, I, W, H) * mag).float().permute(0, 1, 3, 2)
    assert not addend.is_contiguous()
    act = _randn(seed + 3, N, I, H, W).float()
    slope = (_randn(seed + 4, I) * 0.3).float()
    factor = torch.where(act > 0, torch.ones_like(act), slope.view(1, -1, 1, 1).expand_as(act)).double()
    buf.fill_(SENTINEL)
    got = pd.run(dy, (H, W), act=act, slope=slope, addend=addend, out=out)
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    err = (got.double() - (ref + addend.double()) * factor).abs()
    assert bool((err <= ((K + 2) * U32 * mags + U32 * addend.double().abs()) * factor.abs()).all())
    # a per-input-channel scale folded into the pack (the BatchNorm in front) and a per-output-channel one (the BatchNorm behind)
    a_in, a_out = (1 + 0.2 * _randn(seed + 5, I)).float(), (1 + 0.2 * _randn(seed + 6, O)).float()
    got = PackedDgrad(w, k_scale=a_out, out_scale=a_in, stride=stride).run(dy, (H, W))
    wf = ((w * a_out.view(-1, 1, 1, 1)) * a_in.view(1, -1, 1, 1)).double()          # the folded fp32 weights, rounded as the pack rounds them
    err = (got.double() - _conv_transpose64(dy.double(), wf, stride, (H, W))).abs()
    assert bool((err <= (K + 2) * U32 * _conv_transpose64(dy.double().abs(), wf.abs(), stride, (H, W))).all())


def test_conv2d_dgrad_refuses_a_wrong_size():
    from torch_utils.ops.plain_conv_grad import PackedDgrad
    pd = PackedDgrad(_randn(1, 8, 8, 3, 3).float(), stride=2)
    with pytest.raises(RuntimeError, match='conv2d_dgrad'):
        pd.run(_randn(2, 1, 8, 7, 5).float(), (15, 9))              # a 15 x 9 input gives 8 x 5


# ---- 3. the squeeze-and-excitation backward alone ---------------------------------------------------------------------------------

@pytest.mark.parametrize('C', [64, 512])
@pytest.mark.parametrize('H,W', [(7, 7), (20, 24)])
@pytest.mark.parametrize('shortcut', ['identity', 'strided_even', 'strided_odd'])
def test_se_backward_against_fp64(C, H, W, shortcut):
    """sg3_se_residual_bwd from what the recording forward keeps, against float64 autograd; one library call (its two kernels:
    the plane reduction and the apply pass), as the forward."""
    from torch_utils.ops import se_ops
    abi = _abi()
    N, R = 2, C // 16
    seed = C + H
    res = _randn(seed, N, C, H, W).float()
    fc1 = (_randn(seed + 1, R, C, 1, 1) / np.sqrt(C)).float()
    fc2 = (_randn(seed + 2, C, R, 1, 1) / np.sqrt(R)).float()
    dout = _randn(seed + 3, N, C, H, W).float()
    ih, iw = (H, W) if shortcut == 'identity' else ((2 * H, 2 * W) if shortcut == 'strided_even' else (2 * H - 1, 2 * W - 1))
    xin = _randn(seed + 4, N, C, ih, iw).float()

    def composite(res_, xin_, dtype):
        sc = xin_ if shortcut == 'identity' else xin_[:, :, ::2, ::2]
        m = res_.mean(dim=(2, 3))
        g = torch.sigmoid(torch.relu(m @ fc1.to(dtype).flatten(1).t()) @ fc2.to(dtype).flatten(1).t())
        return sc + res_ * g.view(N, C, 1, 1)

    grads = {}
    for dtype in (torch.float64, torch.float32):
        r_, x_ = res.to(dtype).requires_grad_(True), xin.to(dtype).requires_grad_(True)
        out = composite(r_, x_, dtype)
        grads[dtype] = (out.detach(),) + torch.autograd.grad(out, [r_, x_], dout.to(dtype))
    sc = xin if shortcut == 'identity' else xin[:, :, ::2, ::2]
    before = abi.launch_count
    out, mean = se_ops.se_residual_record(res, sc, fc1, fc2)
    assert abi.launch_count - before == 1
    before = abi.launch_count
    dres, dsc = se_ops.se_residual_bwd(dout, res, mean, fc1, fc2, scatter_hw=None if shortcut == 'identity' else (ih, iw))
    assert abi.launch_count - before == 1
    if shortcut == 'identity':
        assert dsc is None
        dsc = dout
    else:
        assert bool((dsc[:, :, 1::2] == 0).all()) and bool((dsc[:, :, :, 1::2] == 0).all())
    for name, got, i in (('out', out, 0), ('dres', dres, 1), ('dshortcut', dsc, 2)):
        ref = grads[torch.float64][i]
        e_hip, e_t32 = float((got.double() - ref).abs().max()), float((grads[torch.float32][i].double() - ref).abs().max())
        print(f'se_bwd C{C} {H}x{W} {shortcut}: {name} e_hip {e_hip:.3e} e_torch32 {e_t32:.3e}')
        assert e_hip <= 2 * e_t32 + 1e-7 * float(ref.abs().max()), name


# ---- 4. one residual unit, recorded and differentiated --------------------------------------------------------------------------

def _unit_case(shape, negate, precision, se=True):
    from torch_utils.ops import plain_conv
    cin, depth, stride, h, w = shape
    unit64 = cases.build_unit(cin, depth, stride, negate=negate, device=DEV, se=se)
    unit32 = cases.build_unit(cin, depth, stride, negate=negate, dtype=torch.float32, device=DEV, se=se)
    x = _randn(cin + depth + h, 2, cin, h, w).float()
    grads = {}
    with _no_miopen():
        for unit, dtype in ((unit64, torch.float64), (unit32, torch.float32)):
            x_ = x.to(dtype).requires_grad_(True)
            out = unit(x_)
            dout = _randn(cin + depth + h + 1, *out.shape)
            grads[dtype] = (out.detach(), torch.autograd.grad(out, x_, dout.to(dtype))[0])
    saved_precision, plain_conv.precision = plain_conv.precision, precision
    try:
        abi = _abi()
        with torch.no_grad():
            unit32.backward_hip(unit32.forward_hip_record(x)[1], dout.float())          # packs the weights (launches of their own)
        before = abi.launch_count
        with torch.no_grad():
            out, saved = unit32.forward_hip_record(x)
        fwd = abi.launch_count - before
        dx = unit32.backward_hip(saved, dout.float())
        bwd = abi.launch_count - before - fwd
    finally:
        plain_conv.precision = saved_precision
    return unit32, x, dout.float(), grads, out, dx, saved, fwd, bwd


@pytest.mark.parametrize('shape', cases.UNIT_SHAPES)
@pytest.mark.parametrize('negate', [False, True])
@pytest.mark.parametrize('precision', ['fp32', 'f16x3'])
def test_unit_record_and_backward_against_fp64(shape, negate, precision):
    """forward_hip_record + backward_hip of a bottleneck_IR_SE against float64 autograd of the torch module, float32 autograd as the
    yardstick, by the general rule (factor 2) under both forward precisions, output and gradient.  Launch budget: forward at most
    4 kernels (+ 1 with a projection), backward at most 6 (+ 1); sg3_se_residual and its backward are one call, two kernels each."""
    unit, x, dout, grads, out, dx, saved, fwd, bwd = _unit_case(shape, negate, precision)
    proj = isinstance(unit.shortcut_layer, torch.nn.Sequential)
    assert fwd == 3 + proj and fwd + 1 <= 4 + proj                       # conv1, conv2, (shortcut,) se: + 1 kernel inside the se call
    assert bwd == 3 + proj and bwd + 1 <= 6 + proj                       # se backward (two kernels), dgrad2, (shortcut dgrad,) dgrad1
    for name, got, i in (('out', out, 0), ('dx', dx, 1)):
        ref = grads[torch.float64][i]
        e_hip, e_t32 = float((got.double() - ref).abs().max()), float((grads[torch.float32][i].double() - ref).abs().max())
        print(f'unit {shape} negate {negate} {precision}: {name} e_hip {e_hip:.3e} e_torch32 {e_t32:.3e} max|ref| {float(ref.abs().max()):.3e}')
        assert e_hip <= 2 * e_t32 + 1e-7 * float(ref.abs().max()), name


@pytest.mark.parametrize('shape', cases.UNIT_SHAPES[:3])
def test_unit_without_squeeze_and_excitation(shape):
    """bottleneck_IR (mode='ir'): the same convolution kernels around a plain residual add; identity stride 1 and 2, projection."""
    unit, x, dout, grads, out, dx, saved, fwd, bwd = _unit_case(shape, True, 'fp32', se=False)
    proj = isinstance(unit.shortcut_layer, torch.nn.Sequential)
    assert (fwd, bwd) == (2 + proj, 2 + proj)
    for name, got, i in (('out', out, 0), ('dx', dx, 1)):
        ref = grads[torch.float64][i]
        e_hip, e_t32 = float((got.double() - ref).abs().max()), float((grads[torch.float32][i].double() - ref).abs().max())
        print(f'unit (ir) {shape}: {name} e_hip {e_hip:.3e} e_torch32 {e_t32:.3e}')
        assert e_hip <= 2 * e_t32 + 1e-7 * float(ref.abs().max()), name


@pytest.mark.parametrize('shape', cases.UNIT_SHAPES)
def test_unit_mixed_sign_slopes_need_the_pre_activation(shape):
    """With a third of the slopes negative the recording forward keeps the pre-activation; a mask read from the sign of the PReLU
    output, which is what the non-negative case saves, gives a gradient that is wrong by order one."""
    unit, x, dout, grads, out, dx, saved, fwd, bwd = _unit_case(shape, True, 'fp32')
    act = saved[0]
    h1 = F.prelu(act, unit.res_layer[2].weight)
    assert float(((h1 > 0) != (act > 0)).float().mean()) > 0.05
    wrong = unit.backward_hip((h1.contiguous(),) + tuple(saved[1:]), dout)
    ref = grads[torch.float64][1]
    assert float((wrong.double() - ref).abs().max()) > 1e-2 * float(ref.abs().max())
    assert float((dx.double() - ref).abs().max()) < 1e-4 * float(ref.abs().max())


# ---- 5. the whole loss ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def nets():
    """(hip float32, torch float32 yardstick, float64) Backbones on the device with the same synthetic weights."""
    return cases.build_backbone(DEV), cases.build_backbone(DEV), cases.build_backbone(DEV, dtype=torch.float64)


@pytest.fixture(scope='module')
def golden():
    return np.load(cases.GOLDEN)


def _loss_case(nets, golden, size):
    """inputs and the float64 reference (golden at 64, autograd on the device otherwise) and the float32 composite yardstick."""
    net, net32, net64 = nets
    if size == 64:
        x, y, y_hat = (torch.from_numpy(golden[f's64_{n}']).to(DEV) for n in ('x', 'y', 'y_hat'))
        ref = dict(loss=float(golden['s64_loss']), logs=golden['s64_logs'], grad=torch.from_numpy(golden['s64_grad']).to(DEV))
    else:
        x = cases.images(1, size, seed=size).to(DEV)
        y, y_hat = x, cases.perturbed(x.cpu(), seed=size + 2).to(DEV)
        with _no_miopen():
            loss, _, logs, _, grad = cases.loss_and_grad(net64, y_hat.double(), y.double(), x.double())
        ref = dict(loss=float(loss), logs=cases.logs_array(logs), grad=grad)
    with _no_miopen():
        loss, _, logs, _, grad = cases.loss_and_grad(net32, y_hat, y, x)
    return x, y, y_hat, ref, dict(loss=float(loss), logs=cases.logs_array(logs), grad=grad)


def _warm(crit, image):
    """One forward and backward, so that the weights are packed (launches of their own) before a test counts launches."""
    leaf = image.clone().requires_grad_(True)
    torch.autograd.grad(crit.extract_feats(leaf).sum(), leaf)


@pytest.mark.parametrize('size', [64, 256, 1024])
def test_id_loss_against_fp64(nets, golden, size, monkeypatch):
    """Loss and logs within the general rule, the image gradient within GRAD_FACTOR x the composite's float32 error; no composite
    runs; launch totals; the gradient bit-equal on repeat and reaching a leaf that also feeds a plain torch op.  DEVIATION from the
    general rule, for the loss alone: its 1e-7 term is taken of max(|loss|, 1), not of |loss|.  The loss is 1 - cos with cos within
    1e-3 of one and is formed in float32 as the reference forms it, so its rounding floor is that of cos (half an ulp of one,
    6e-8), whatever computes the features; the literal rule holds only where the float32 yardstick lands within 1e-9 of float64 by
    chance, as it does at 256 x 256 (below), where the kernels' 5.8e-8 misses 2 x 2.0e-9 + 1e-7 x 7e-4.
    Measured on an MI355X (e_hip / e_torch32): loss 2.5e-9 / 2.7e-8, 5.8e-8 / 2.0e-9, 8.5e-8 / 9.4e-8; logs 7.1e-8 / 5.5e-8, 5.8e-8 / 2.0e-9,
    1.2e-7 / 9.4e-8; gradient 2.7e-7 / 5.3e-7, 2.2e-9 / 2.9e-7, 1.5e-10 / 1.3e-10 at 64, 256 and 1024."""
    from criteria.id_loss import IDLoss
    from torch_utils.ops import face_pool as fp
    abi = _abi()
    net = nets[0]
    x, y, y_hat, ref, t32 = _loss_case(nets, golden, size)

    def refuse(*a, **k):
        raise AssertionError('a composite ran')

    monkeypatch.setattr(net, 'forward', refuse)
    monkeypatch.setattr(fp, 'composite', refuse)
    crit = IDLoss(facenet=net)
    _warm(crit, y_hat[:1])
    leaf = y_hat.clone().requires_grad_(True)
    before = abi.launch_count
    loss, sim, logs = crit(leaf, y, x)
    fwd = abi.launch_count - before
    grad, = torch.autograd.grad(loss, leaf, retain_graph=True)
    bwd = abi.launch_count - before - fwd
    lf, lb = net.launches()
    assert (fwd, bwd) == ((2 if y is x else 3) * (1 + lf), lb + 1)
    assert loss.dtype == torch.float32 and loss.ndim == 0 and isinstance(sim, float) and len(logs) == x.shape[0]
    (loss + 0.5 * (leaf * leaf).sum()).backward()
    assert torch.allclose(leaf.grad, grad + leaf.detach(), rtol=1e-6, atol=0)
    leaf2 = y_hat.clone().requires_grad_(True)
    loss2, _, logs2 = crit(leaf2, y, x)
    assert torch.equal(loss2, loss) and logs2 == logs and torch.equal(torch.autograd.grad(loss2, leaf2)[0], grad)
    e_hip, e_t32 = abs(float(loss) - ref['loss']), abs(t32['loss'] - ref['loss'])
    print(f'IDLoss {size}: loss e_hip {e_hip:.3e} e_torch32 {e_t32:.3e} loss {ref["loss"]:.6e}')
    assert e_hip <= 2 * e_t32 + 1e-7 * max(abs(ref['loss']), 1.0)
    e_hip, e_t32 = float(np.abs(cases.logs_array(logs) - ref['logs']).max()), float(np.abs(t32['logs'] - ref['logs']).max())
    print(f'IDLoss {size}: logs e_hip {e_hip:.3e} e_torch32 {e_t32:.3e}')
    assert e_hip <= 2 * e_t32 + 1e-7 * float(np.abs(ref['logs']).max())
    assert abs(sim - float((ref['logs'][:, 0] - ref['logs'][:, 2]).mean())) <= 2 * (2 * e_t32 + 1e-7)
    scale = float(ref['grad'].abs().max())
    e_hip, e_t32 = float((grad.double() - ref['grad']).abs().max()), float((t32['grad'].double() - ref['grad']).abs().max())
    print(f'IDLoss {size}: gradient e_hip {e_hip:.3e} e_torch32 {e_t32:.3e} ratio {e_hip / e_t32:.2f} max|g64| {scale:.3e} rms {float(ref["grad"].pow(2).mean().sqrt()):.3e}')
    assert e_hip <= GRAD_FACTOR * e_t32 + 1e-7 * scale


def test_id_loss_with_negative_slopes_against_fp64(monkeypatch):
    """The whole backbone with every third PReLU slope negative, stem included (synthetic slopes are otherwise all positive): the
    stem and every unit keep their pre-activation, unit 0's data gradient takes the stem's derivative from it, and the no_grad
    forward of the target runs the fused-activation stem.  B = 1, 64 x 64, recording forward on the exact fp32 kernels (the
    split-precision forward is the subject of the cases above; this one is about the route).

    Features of x and y_hat: the general rule.  The gradient of a PReLU network jumps where a pre-activation changes sign, by
    (1 - slope) of the gradient there -- up to 1.4 with these slopes -- and a float32 forward cannot tell the sign of a
    pre-activation smaller than its own rounding error.  So the branches the kernels took are compared with float64's first: they
    may differ only where |float64 pre-activation| <= 1e-5 of the layer's largest (the float32 forward's error through up to 50
    layers).  The gradient is then compared with float64 autograd TAKING THE KERNELS' BRANCHES, within GRAD_FACTOR x the float32
    composite's own error.  Measured on an MI355X: 1 of 3 713 024 branches differs; e_hip 1.8e-8 on the kernels' branches (7.3e-7
    against float64's own), e_torch32 1.0e-8, of 3.6e-4."""
    from criteria.id_loss import IDLoss
    from torch_utils.ops import plain_conv
    from torch_utils.ops.face_pool import face_pool
    monkeypatch.setattr(plain_conv, 'precision', 'fp32')
    net, net32, net64 = (cases.build_backbone(DEV, negate=True), cases.build_backbone(DEV, negate=True),
                         cases.build_backbone(DEV, dtype=torch.float64, negate=True))
    assert bool((net.input_layer[2].weight < 0).any())
    x = cases.images(1, 64, seed=31).to(DEV)
    y_hat = cases.perturbed(x.cpu(), seed=32).to(DEV)
    with _no_miopen():
        _, _, _, feats64, grad64 = cases.loss_and_grad(net64, y_hat.double(), x.double(), x.double())
        _, _, _, feats32, grad32 = cases.loss_and_grad(net32, y_hat, x, x)

    def refuse(*a, **k):
        raise AssertionError('a composite ran')

    monkeypatch.setattr(net, 'forward', refuse)
    crit = IDLoss(facenet=net)
    leaf = y_hat.clone().requires_grad_(True)
    loss, _, logs = crit(leaf, x, x)
    grad, = torch.autograd.grad(loss, leaf)
    assert net._packed['mixed'] and all(u._packed['grad']['mixed'] for u in net.body)
    # features: of x from the no_grad forward (fused-activation stem), of y_hat from the recording forward (pre-activation kept)
    with torch.no_grad():
        fx = crit.extract_feats(x)
        _, stem_act, saved = net._forward_record(face_pool(y_hat), True)               # the same bits as the run above
    fy = crit.extract_feats(y_hat.clone().requires_grad_(True)).detach()
    for name, got, i in (('x', fx, 0), ('y_hat', fy, 2)):
        e_hip, e_t32 = float((got.double() - feats64[i]).abs().max()), float((feats32[i].double() - feats64[i]).abs().max())
        print(f'IDLoss negative slopes: features of {name} e_hip {e_hip:.3e} e_torch32 {e_t32:.3e} max|f64| {float(feats64[i].abs().max()):.3e}')
        assert e_hip <= 2 * e_t32 + 1e-7 * float(feats64[i].abs().max()), name
    # float64 autograd on the branches the kernels took
    masks = [stem_act > 0] + [s[0] > 0 for s in saved]
    prelus = [net64.input_layer[2]] + [u.res_layer[2] for u in net64.body]
    pre64 = []
    for m, mask in zip(prelus, masks):
        def forward(t, m=m, mask=mask):
            pre64.append(t.detach())
            return torch.where(mask, t, t * m.weight.view(1, -1, 1, 1))
        monkeypatch.setattr(m, 'forward', forward)
    yh = y_hat.double().requires_grad_(True)
    with _no_miopen():
        ref, = torch.autograd.grad(1 - (cases.extract_feats(net64, yh) * feats64[0]).sum(), yh)
    flips = 0
    for mask, pre in zip(masks, pre64):
        differ = mask != (pre > 0)
        flips += int(differ.sum())
        assert not bool(differ.any()) or float(pre[differ].abs().max()) <= 1e-5 * float(pre.abs().max())
    scale = float(grad64.abs().max())
    e_own = float((grad.double() - grad64).abs().max())
    e_hip, e_t32 = float((grad.double() - ref).abs().max()), float((grad32.double() - grad64).abs().max())
    print(f'IDLoss negative slopes: {flips} of {sum(m.numel() for m in masks)} branches differ from float64; gradient e_hip {e_hip:.3e} '
          f'(against float64 on its own branches {e_own:.3e}) e_torch32 {e_t32:.3e} max|g64| {scale:.3e}')
    assert e_hip <= GRAD_FACTOR * e_t32 + 1e-7 * scale


def test_backward_uses_the_packs_of_its_forward(nets):
    """Dropping the module's packed weights between forward and backward (`.eval()`, `.to()`, `load_state_dict` do) leaves the
    gradient what it was: the record holds the packs it ran on.  Differentiating the gradient again raises."""
    from criteria.id_loss import IDLoss
    net = nets[0]
    crit = IDLoss(facenet=net)
    y_hat = cases.images(1, 64, seed=41).to(DEV)
    x = cases.perturbed(y_hat.cpu(), seed=42).to(DEV)

    def grad(invalidate):
        leaf = y_hat.clone().requires_grad_(True)
        loss = crit(leaf, x, x)[0]
        if invalidate:
            net.eval()
            assert net._packed is None and net.body[0]._packed is None
        return torch.autograd.grad(loss, leaf)[0]

    assert torch.equal(grad(False), grad(True))
    leaf = y_hat.clone().requires_grad_(True)
    g, = torch.autograd.grad(crit(leaf, x, x)[0], leaf, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_id_loss_batch_invariance(nets):
    """Sample 0 of a batch of two against the sample alone.  The trunk is bit-identical, forward and backward: every workgroup of
    the kernels sees one sample and sums in one fixed order.  The head's GEMM is torch's and may pick another reduction order for
    another row count, which moves a feature by a few units of (25088 + 2) 2^-24 of its terms; the loss gradient is therefore
    compared to 1e-5 of its largest entry."""
    from criteria.id_loss import IDLoss
    net = nets[0]
    x = cases.images(2, 64, seed=9).to(DEV)
    y_hat = cases.perturbed(x.cpu(), seed=10).to(DEV)
    from torch_utils.ops.face_pool import face_pool
    img = face_pool(y_hat)
    with torch.no_grad():
        body2, act2, saved2 = net._forward_record(img, True)
        body1, act1, saved1 = net._forward_record(img[:1].contiguous(), True)
        assert torch.equal(body2[:1], body1)
        d = _randn(3, 2, 512, 7, 7).float() * 1e-4
        pk = net._packed
        assert torch.equal(net._trunk_backward(pk, act2, saved2, d)[:1], net._trunk_backward(pk, act1, saved1, d[:1].contiguous()))
    crit = IDLoss(facenet=net)

    def grad(yh, xs):
        leaf = yh.clone().requires_grad_(True)
        return torch.autograd.grad(crit(leaf, xs, xs)[0] * xs.shape[0], leaf)[0]

    g2, g1 = grad(y_hat, x), grad(y_hat[:1], x[:1])
    print(f'batch invariance of the loss gradient: max|g(B=2)[0] - g(B=1)| = {float((g2[:1] - g1).abs().max()):.3e} of {float(g1.abs().max()):.3e}')
    assert float((g2[:1] - g1).abs().max()) <= 1e-5 * float(g1.abs().max())


def test_id_loss_overflow_repeats_on_fp32(nets):
    """One stem filter scaled up until an activation leaves the fp16 range (the weights themselves stay inside it): the flag rises,
    the recording forward is repeated on the fp32 kernels, and loss and gradient are those of a run with precision 'fp32' bit for
    bit."""
    from criteria.id_loss import IDLoss
    from torch_utils.ops import plain_conv
    abi = _abi()
    net = cases.build_backbone(DEV)
    with torch.no_grad():
        net.input_layer[0].weight[5] = 2e4              # a smooth image sums to more than 3.3 over 27 taps somewhere: |output| > 65504
    net.invalidate_packed()
    crit = IDLoss(facenet=net)
    x = cases.images(1, 64, seed=21).to(DEV)
    y_hat = cases.perturbed(x.cpu(), seed=22).to(DEV)

    def run():
        leaf = y_hat.clone().requires_grad_(True)
        before = abi.launch_count
        loss = crit(leaf, x, x)[0]
        return loss.detach(), torch.autograd.grad(loss, leaf)[0], abi.launch_count - before

    assert plain_conv.precision == 'f16x3'
    run()                                                                          # packs both forms
    loss, grad, calls = run()
    assert calls == 2 * (1 + 2 * net.launches()[0]) + net.launches()[1] + 1          # both forwards ran twice
    plain_conv.precision = 'fp32'
    try:
        loss32, grad32, calls32 = run()
    finally:
        plain_conv.precision = 'f16x3'
    assert calls32 == 2 * (1 + net.launches()[0]) + net.launches()[1] + 1
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad).all())
    assert torch.equal(loss, loss32) and torch.equal(grad, grad32)


def test_extract_feats_path_rule(nets):
    """The HIP path needs eval mode, frozen parameters and float32; everything else is the composite under autograd."""
    from criteria.id_loss import IDLoss
    abi = _abi()
    net = cases.build_backbone(DEV)
    crit = IDLoss(facenet=net)
    x = cases.images(1, 64, seed=5).to(DEV)
    assert crit.uses_hip(x) and not crit.uses_hip(x.double()) and not crit.uses_hip(x.cpu())
    with torch.no_grad():
        f = crit.extract_feats(x)
    net.body[0].res_layer[1].weight.requires_grad_(True)
    assert not crit.uses_hip(x)
    before = abi.launch_count
    with _no_miopen():
        g = crit.extract_feats(x)
    assert abi.launch_count - before == 1 and g.requires_grad                    # face_pool only; the network under autograd
    assert float((g - f).abs().max()) < 1e-4
    net.body[0].res_layer[1].weight.requires_grad_(False)
    net.train()
    assert not crit.uses_hip(x)


# ---- 6. the Coach ---------------------------------------------------------------------------------------------------------------------

def test_coach_step_with_the_reference_id_lambda(tmp_path):
    """One real training run (steps 0 and 1) of the Tmini mapper with id_lambda = 0.06: the mapper moves, loss_id is finite and logged,
    and every step's identity loss ran on the kernels."""
    import json
    import os
    from criteria.id_loss import IDLoss
    from test_gpu_styleclip_mapper_train import _coach
    abi = _abi()
    coach, o = _coach('Tmini', tmp_path, 1)
    torch.save(cases.build_backbone('cpu').state_dict(), tmp_path / 'model_ir_se50.pth')
    coach.opts.ir_se50_weights = str(tmp_path / 'model_ir_se50.pth')
    crit = IDLoss(coach.opts).to(DEV).eval()                        # built as Coach builds it: from the checkpoint path
    assert not any(q.requires_grad for q in crit.parameters()) and crit.uses_hip(cases.images(1, 64, seed=1).to(DEV))
    crit.facenet.forward = None                                     # the composite must not run
    _warm(crit, cases.images(1, 64, seed=1).to(DEV))               # packs the weights
    calls = []
    forward = crit.forward

    def counted(y_hat, y, x):
        before = abi.launch_count
        out = forward(y_hat, y, x)
        calls.append(abi.launch_count - before)
        return out

    crit.forward = counted
    coach.opts.id_lambda, coach.id_loss = 0.06, crit
    before = {k: v.detach().clone() for k, v in coach.net.mapper.named_parameters()}
    coach.train()
    lf = crit.facenet.launches()[0]
    assert len(calls) >= 2 and all(c == 2 * (1 + lf) for c in calls)
    for k, p in coach.net.mapper.named_parameters():
        assert not torch.equal(p.detach(), before[k]) and bool(torch.isfinite(p).all()), k
    with open(os.path.join(o.exp_dir, 'logs', 'metrics.jsonl')) as f:
        rows = [json.loads(line) for line in f if '"train"' in line]
    assert [r['step'] for r in rows] == [0, 1] and all(np.isfinite(r['loss_id']) and np.isfinite(r['id_improve']) for r in rows)
