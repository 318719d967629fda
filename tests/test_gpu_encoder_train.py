"""Training the encoder trunk on the GPU: the batch-summed weight gradient alone against float64 with the element-wise bound of the
GEMM tests, training-mode BatchNorm forward / backward / running statistics alone, and one residual unit recorded and differentiated
with respect to its input and every parameter, with the composite's float32 autograd on the same device as the yardstick.

General rule: |hip - fp64| <= F max|torch32 - fp64| + 1e-7 max|fp64|, F = 2.  Measured on an MI355X: see DESIGN.md 3.15."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_train_cases as cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U32 = 2.0 ** -24
GUARD = 4096
SENTINEL = 777.0


def _abi():
    from torch_utils import _sg3abi as abi
    return abi


def _randn(seed, *shape):
    return cases.randn(seed, *shape).to(DEV)             # float64


def _no_miopen():
    return torch.backends.cudnn.flags(enabled=False)             # the torch yardsticks: no MIOpen search per convolution shape


def _rule(name, hip, t32, ref, factor=2):
    hip, t32, ref = hip.detach(), t32.detach(), ref.detach()
    e_hip, e_t32, top = float((hip.double() - ref).abs().max()), float((t32.double() - ref).abs().max()), float(ref.abs().max())
    print(f'{name}: e_hip {e_hip:.3e} e_torch32 {e_t32:.3e} max|fp64| {top:.3e}')
    assert e_hip <= factor * e_t32 + 1e-7 * top, name


# ---- 1. sg3_conv2d_wgrad_sum alone ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k,stride,I,O,H,W,N', [s + (2,) for s in cases.WGRAD_SHAPES] + [(3, 1, 40, 20, 5, 70, 3)])
def test_conv2d_wgrad_sum_against_fp64(k, stride, I, O, H, W, N):
    """Against float64 torch.nn.grad.conv2d_weight, element by element:
        |hip - ref| <= (K + 2) 2^-24 (|dy| * |xt|),   K = N OH OW,
    plain and with the input affine (non-zero shifts: padding that is not kept at zero fails), upstream gradients of magnitude 1 and
    1e-6 under the same relative bound, guard bands around the output untouched, one ABI call, bit-equal on repeat."""
    from torch_utils.ops.plain_conv_wgrad import wgrad
    abi = _abi()
    seed = k * 1000 + stride * 100 + I + H + N
    oh, ow = cases.out_hw(H, W, k, stride)
    K = N * oh * ow
    assert K >= 24
    x = _randn(seed, N, I, H, W).float()
    a, b = (1 + 0.3 * _randn(seed + 2, I)).float(), (0.5 + 0.4 * _randn(seed + 3, I)).float()
    buf = torch.full([O * I * k * k + 2 * GUARD], SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[GUARD:-GUARD].view(O, I, k, k)
    for mag in (1.0, 1e-6):
        dy = (_randn(seed + 1, N, O, oh, ow) * mag).float()
        for affine in (False, True):
            xt = cases.padded_affine(x.double(), a.double(), b.double()) if affine else x.double()
            ref = cases.wgrad64(xt, dy.double(), k, stride)
            mags = cases.wgrad64(xt.abs(), dy.double().abs(), k, stride)
            buf.fill_(SENTINEL)
            before = abi.launch_count
            got = wgrad(x, dy, k, stride, in_scale=a if affine else None, in_shift=b if affine else None, out=out)
            assert abi.launch_count - before == 1 and got.data_ptr() == out.data_ptr()
            assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
            err = (got.double() - ref).abs()
            bound = (K + 2) * U32 * mags
            print(f'wgrad k{k} s{stride} {I}->{O} {H}x{W} N{N} mag {mag:g} affine {affine}: max err / bound '
                  f'{float((err / bound.clamp_min(1e-300)).max()):.3f}, max|ref| {float(ref.abs().max()):.3e}')
            assert bool((err <= bound).all())
            again = wgrad(x, dy, k, stride, in_scale=a if affine else None, in_shift=b if affine else None)
            assert torch.equal(again, got)


def test_conv2d_wgrad_sum_rejects_wrong_shapes():
    from torch_utils.ops.plain_conv_wgrad import wgrad
    x = torch.zeros([2, 4, 9, 9], device=DEV)
    with pytest.raises(RuntimeError, match='conv2d_wgrad_sum'):
        wgrad(x, torch.zeros([2, 5, 9, 9], device=DEV), 3, 2)
    with pytest.raises(RuntimeError, match='conv2d_wgrad_sum'):
        wgrad(x, torch.zeros([3, 5, 9, 9], device=DEV), 3, 1)


# ---- 2. training-mode BatchNorm alone -----------------------------------------------------------------------------------------------

def _bn_input(seed, C, H, W, offset):
    x = _randn(seed, 2, C, H, W)
    return (100.0 + 0.01 * x if offset else x).float()


@pytest.mark.parametrize('offset', [False, True])
@pytest.mark.parametrize('C,H,W', [(5, 7, 9), (64, 7, 9), (70, 7, 9), (5, 32, 32), (64, 32, 32), (70, 32, 32)])
def test_batchnorm_train_forward_backward_against_fp64(C, H, W, offset):
    """Statistics, apply, backward sums and backward pass against float64 F.batch_norm(training=True) and its autograd, on values of
    magnitude 1 and on mean 100 with spread 0.01 (a variance formed as E[x^2] - E[x]^2 is lost there)."""
    from torch_utils.ops import batchnorm_train as bt
    abi = _abi()
    seed = C * 10 + H + (5 if offset else 0)
    x = _bn_input(seed, C, H, W, offset)
    gamma, beta = (1 + 0.3 * _randn(seed + 1, C)).float(), (0.2 * _randn(seed + 2, C)).float()
    dy = _randn(seed + 3, 2, C, H, W).float()
    eps = 1e-5
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y64 = F.batch_norm(x64, None, None, g64, b64, True, 0.1, eps)
    r64 = torch.autograd.grad(y64, [x64, g64, b64], dy.double())
    x32, g32, b32 = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    with _no_miopen():
        y32 = F.batch_norm(x32, None, None, g32, b32, True, 0.1, eps)
        r32 = torch.autograd.grad(y32, [x32, g32, b32], dy)

    before = abi.launch_count
    st = bt.stats(x, gamma, beta, eps)
    y = bt.apply(x, st.a, beta, centre=st.mean, centre_lo=st.mean_lo)
    assert abi.launch_count - before == 2 and st.count == 2 * H * W
    mean64 = x.double().mean(dim=(0, 2, 3))
    var64 = x.double().var(dim=(0, 2, 3), unbiased=False)
    assert float((st.mean.double() - mean64).abs().max()) <= U32 * float(mean64.abs().max())           # one rounding of an exact sum
    assert float(((st.var.double() - var64) / var64).abs().max()) <= 4 * U32
    assert float(((st.invstd.double() - (var64 + eps) ** -0.5) * (var64 + eps) ** 0.5).abs().max()) <= 4 * U32
    tag = f'bn C{C} {H}x{W} offset {offset}'
    _rule(tag + ' y', y, y32, y64.detach())
    # the affine form a x + b that the convolutions fuse: exact a and b to one rounding each
    a64 = gamma.double() * (var64 + eps) ** -0.5
    assert float(((st.a.double() - a64) / a64).abs().max()) <= 4 * U32
    b_ref = beta.double() - mean64 * a64
    assert float((st.b.double() - b_ref).abs().max()) <= 4 * U32 * float((beta.double().abs() + (mean64 * a64).abs()).max())

    before = abi.launch_count
    dbeta, dgamma = bt.backward_reduce(dy, x, st)
    dx = bt.backward_apply(dy, x, st, dbeta, dgamma)
    assert abi.launch_count - before == 2
    _rule(tag + ' dx', dx, r32[0], r64[0])
    _rule(tag + ' dgamma', dgamma, r32[1], r64[1])
    _rule(tag + ' dbeta', dbeta, r32[2], r64[2])
    st2 = bt.stats(x, gamma, beta, eps)
    assert all(torch.equal(p, q) for p, q in zip(st[:6], st2[:6]))
    assert torch.equal(bt.apply(x, st.a, beta, centre=st.mean, centre_lo=st.mean_lo), y) and torch.equal(bt.backward_apply(dy, x, st, dbeta, dgamma), dx)
    d2 = bt.backward_reduce(dy, x, st)
    assert torch.equal(d2[0], dbeta) and torch.equal(d2[1], dgamma)


@pytest.mark.parametrize('C,H,W', [(5, 7, 9), (70, 32, 32)])
def test_batchnorm_train_prelu_apply_and_backward_epilogues(C, H, W):
    """u -> x = PReLU(u) -> BatchNorm -> PReLU -> out, with a second consumer of x: the apply with its activation and returned
    pre-activation, the slope gradient from the reduction kernel, and the backward pass with the strided addend (the second consumer's
    gradient) and the PReLU-derivative mask (the activation in front).  Every third slope is zero or negative."""
    from torch_utils.ops import batchnorm_train as bt
    seed = 300 + C
    u = _randn(seed, 2, C, H, W).float()
    gamma, beta = (1 + 0.3 * _randn(seed + 1, C)).float(), (0.2 * _randn(seed + 2, C)).float()
    s_in, s_out = (0.25 + 0.1 * _randn(seed + 3, C)).float(), (0.25 + 0.1 * _randn(seed + 4, C)).float()
    for s in (s_in, s_out):
        s[0::3] = 0.0
        s[1::6] = -0.2
    dout = _randn(seed + 5, 2, C, H, W).float()
    addend = _randn(seed + 6, 2, C, W, H).float().permute(0, 1, 3, 2)
    assert not addend.is_contiguous()
    eps = 1e-5

    def composite(dt):
        uu = u.to(dt).requires_grad_(True)
        ps = [t.to(dt).requires_grad_(True) for t in (gamma, beta, s_out)]
        xx = F.prelu(uu, s_in.to(dt))
        pre = F.batch_norm(xx, None, None, ps[0], ps[1], True, 0.1, eps)
        out = F.prelu(pre, ps[2])
        grads = torch.autograd.grad((out * dout.to(dt)).sum() + (xx * addend.to(dt)).sum(), [uu] + ps)
        return out.detach(), pre.detach(), grads

    out64, pre64, r64 = composite(torch.float64)
    with _no_miopen():
        out32, pre32, r32 = composite(torch.float32)
    x = F.prelu(u, s_in)
    st = bt.stats(x, gamma, beta, eps)
    out, pre = bt.apply(x, st.a, beta, centre=st.mean, centre_lo=st.mean_lo, slope=s_out, want_pre=True)
    _rule('prelu apply out', out, out32, out64)
    _rule('prelu apply pre', pre, pre32, pre64)
    dslope, dpre = bt.slope_grad(dout, pre, s_out)
    assert torch.equal(dpre, torch.where(pre > 0, dout, dout * s_out.view(1, -1, 1, 1)))
    dbeta, dgamma = bt.backward_reduce(dpre, x, st)
    du, raw = bt.backward_apply(dpre, x, st, dbeta, dgamma, addend=addend, act=u, slope=s_in, want_raw=True)
    _rule('epilogue du', du, r32[0], r64[0])
    _rule('epilogue dgamma', dgamma, r32[1], r64[1])
    _rule('epilogue dbeta', dbeta, r32[2], r64[2])
    _rule('epilogue dslope', dslope, r32[3], r64[3])
    assert torch.equal(du, torch.where(u > 0, raw, raw * s_in.view(1, -1, 1, 1)))
    assert torch.equal(bt.slope_grad(dout, pre), dslope)


@pytest.mark.parametrize('momentum', [0.1, None])
def test_batchnorm_train_running_statistics(momentum):
    """Two forwards: running mean, running variance (unbiased) and num_batches_tracked against float64 torch.nn.BatchNorm2d."""
    from torch_utils.ops import batchnorm_train as bt
    C = 70
    mods = {dt: torch.nn.BatchNorm2d(C, momentum=momentum).to(DEV, dt).train() for dt in (torch.float64, torch.float32)}
    ours = torch.nn.BatchNorm2d(C, momentum=momentum).to(DEV).train()
    for step in range(2):
        x = (_randn(40 + step, 2, C, 7, 9) * (1 + step) + 0.5).float()
        for dt, m in mods.items():
            with _no_miopen():
                m(x.to(dt))
        bt.update_running([ours], [bt.stats(x, ours.weight, ours.bias, ours.eps)])
    assert int(ours.num_batches_tracked) == int(mods[torch.float64].num_batches_tracked) == 2
    _rule(f'running_mean momentum {momentum}', ours.running_mean, mods[torch.float32].running_mean, mods[torch.float64].running_mean)
    _rule(f'running_var momentum {momentum}', ours.running_var, mods[torch.float32].running_var, mods[torch.float64].running_var)


# ---- 3. one residual unit, recorded and differentiated ----------------------------------------------------------------------------------

def _unit_launches(kind, projection):
    """ABI calls of (forward_train_record, backward_train) with warm packs: the numbers their docstrings state."""
    return (7 if kind == 'ir_se' else 6) + (3 if projection else 0), (10 if kind == 'ir_se' else 9) + (4 if projection else 0)


@pytest.mark.parametrize('prec', ['fp32', 'f16x3'])
@pytest.mark.parametrize('H,W', [(13, 9), (16, 16)])
@pytest.mark.parametrize('kind', ['ir', 'ir_se'])
@pytest.mark.parametrize('cin,depth,stride', [(64, 64, 1), (64, 64, 2), (64, 128, 2)])
def test_unit_train_record_and_backward(monkeypatch, cin, depth, stride, kind, H, W, prec):
    """Identity, stride-2 identity and projection shortcuts: the output, the input gradient and every parameter gradient meet the
    rule (F = 2) under exact and split-precision forward convolutions; the 13 x 9 cases have every third PReLU slope zero or
    negative.  Launch counts as documented, bit-equal on repeat, running statistics left to the caller."""
    import copy
    from torch_utils.ops import plain_conv
    abi = _abi()
    seed = cin + depth + 10 * stride + H
    unit64 = cases.make_unit(kind, cin, depth, stride, seed, negative_slopes=(H == 13)).to(DEV)
    unit32, unit = copy.deepcopy(unit64).float(), copy.deepcopy(unit64).float()
    x = _randn(seed + 2, 2, cin, H, W).float()
    oh, ow = cases.out_hw(H, W, 3, stride)
    dout = _randn(seed + 3, 2, depth, oh, ow).float()
    out64, dx64, g64 = cases.unit_autograd(unit64, x.double(), dout.double())
    with _no_miopen():
        out32, dx32, g32 = cases.unit_autograd(unit32, x, dout)
    monkeypatch.setattr(plain_conv, 'precision', prec)
    plain_conv.reset_overflow(DEV)
    pairs = []
    out, saved = unit.forward_train_record(x, pairs)            # builds the packs
    unit.backward_train(saved, dout)
    fwd, bwd = _unit_launches(kind, cin != depth)
    before = abi.launch_count
    out2, saved = unit.forward_train_record(x)
    assert abi.launch_count - before == fwd
    before = abi.launch_count
    dx, g = unit.backward_train(saved, dout)
    assert abi.launch_count - before == bwd
    dx2, g2 = unit.backward_train(saved, dout)
    assert not plain_conv.overflowed(DEV)
    assert torch.equal(out, out2) and torch.equal(dx, dx2) and all(torch.equal(g[k], g2[k]) for k in g)
    assert len(pairs) == (3 if cin != depth else 2) and int(unit.res_layer[0].num_batches_tracked) == 0
    assert sorted(g) == sorted(g64)
    tag = f'unit {kind} {cin}->{depth} s{stride} {H}x{W} {prec}'
    _rule(tag + ' out', out, out32, out64)
    _rule(tag + ' dx', dx, dx32, dx64)
    for name in g64:
        assert g[name].shape == g64[name].shape
        _rule(f'{tag} {name}', g[name], g32[name], g64[name])


# ---- 4. the whole trunk through the public switch ---------------------------------------------------------------------------------------

# e_hip / e_torch32 of the trunk's parameter and input gradients: the largest per-tensor ratio measured on an MI355X, doubled, rounded up
# to a power of two, capped at 16 (the idiom of GRAD_FACTOR in test_gpu_id_loss.py).  Measured under the 'fp32' recorded forward: 2.60
# (cotangent on the map, at body.2.res_layer.4.bias) and 5.50 (scalar through the heads, at body.0.res_layer.5.fc1.weight, where the
# float32 yardstick itself is at 3e-7 of the tensor's maximum); 2 x 5.5 = 11 -> 16.  Under 'f16x3' the same tensor measured 20.1, past
# the cap, so the training forward defaults to 'fp32' (`BackboneEncoder.native_training_precision`); DESIGN.md 3.15
TRUNK_GRAD_FACTOR = 16
ENC_SEED = 7


@pytest.fixture(scope='module')
def trunk():
    """The float64 encoder, its float32 copy on torch autograd, the input, and both of their results for a cotangent on the trunk's
    map ('map') and for a scalar through the style heads ('heads'); computed once."""
    import copy
    enc64 = cases.make_encoder(ENC_SEED).to(DEV)
    x = _randn(ENC_SEED + 5, 2, 6, 64, 64).float()
    alive = cases.se_hidden_alive(enc64, x.double())
    assert len(alive) == 24 and all(alive)
    enc32 = copy.deepcopy(enc64).float()
    state32 = copy.deepcopy(enc32.state_dict())
    cot = _randn(ENC_SEED + 6, 2, 512, 4, 4).float()
    wcode = _randn(ENC_SEED + 7, 2, 2, 512).float()
    ref = {}
    for enc, dt in ((enc64, torch.float64), (enc32, torch.float32)):
        state = copy.deepcopy(enc.state_dict())
        params = [p for _, p in cases.trunk_named_parameters(enc)]
        with _no_miopen():
            xr = x.to(dt).requires_grad_(True)
            feat = enc._trunk_torch(xr)
            gm = torch.autograd.grad(feat, [xr] + params, cot.to(dt))
            stats = {k: v.clone() for k, v in enc.state_dict().items() if 'running' in k or 'num_batches' in k}
            enc.load_state_dict(state)
            xr = x.to(dt).requires_grad_(True)
            gh = torch.autograd.grad((enc(xr) * wcode.to(dt)).sum(), [xr] + params)
            enc.load_state_dict(state)
        ref[dt] = dict(feat=feat.detach(), map=gm, heads=gh, stats=stats)
    return dict(enc64=enc64, state32=state32, x=x, cot=cot, wcode=wcode, ref=ref)


def _native_encoder(trunk, monkeypatch):
    import copy
    enc = copy.deepcopy(trunk['enc64']).float()
    enc.load_state_dict(trunk['state32'])
    enc.native_training = True
    enc.train()

    def no_torch_trunk(_x):
        raise AssertionError('_trunk_torch was called with native_training on')
    monkeypatch.setattr(enc, '_trunk_torch', no_torch_trunk)
    return enc


def _native_grads(enc, trunk, which):
    params = [p for _, p in cases.trunk_named_parameters(enc)]
    xr = trunk['x'].clone().requires_grad_(True)
    with _no_miopen():               # the torch heads: deterministic library kernels, as for the yardsticks
        if which == 'map':
            seen = []
            hook = enc.styles[0].register_forward_pre_hook(lambda mod, inp: seen.append(inp[0]))
            enc(xr)
            hook.remove()
            return seen[0].detach(), torch.autograd.grad(seen[0], [xr] + params, trunk['cot'])
        return None, torch.autograd.grad((enc(xr) * trunk['wcode']).sum(), [xr] + params)


def _check_trunk_grads(tag, enc, got, r32, r64):
    names = ['input'] + [n for n, _ in cases.trunk_named_parameters(enc)]
    assert len(names) == 230 and len(got) == 230
    suffix = lambda n: n.split('.', 2)[2] if n.startswith('body.') else n          # noqa: E731
    top = {}
    for n, g in zip(names, r64):
        top[suffix(n)] = max(top.get(suffix(n), 0.0), float(g.abs().max()))
    exits, worst = [], (0.0, None)
    for n, gh, g32, g64 in zip(names, got, r32, r64):
        assert gh.shape == g64.shape and gh.dtype == torch.float32, n
        if float(g64.abs().max()) < 1e-9 * top[suffix(n)]:
            # structurally zero (a per-channel constant in front of a train-mode BatchNorm): float32 autograd leaves rounding noise
            exits.append(n)
            assert float(gh.abs().max()) <= 16 * float(g32.abs().max()), n
            continue
        e_hip, e_t32, mx = float((gh.double() - g64).abs().max()), float((g32.double() - g64).abs().max()), float(g64.abs().max())
        ratio = (e_hip - 1e-7 * mx) / e_t32 if e_t32 > 0 else 0.0
        if ratio > worst[0]:
            worst = (ratio, n)
        assert e_hip <= TRUNK_GRAD_FACTOR * e_t32 + 1e-7 * mx, f'{tag} {n}: e_hip {e_hip:.3e} e_torch32 {e_t32:.3e} max {mx:.3e}'
    print(f'{tag}: largest (e_hip - 1e-7 max) / e_torch32 = {worst[0]:.3f} at {worst[1]}; structural zeros: {exits}')
    assert len(exits) <= 4


@pytest.mark.parametrize('which', ['map', 'heads'])
def test_trunk_native_training_gradients(trunk, monkeypatch, which):
    """`BackboneEncoder(50, 'ir_se')` with `native_training` in train mode at [2, 6, 64, 64], under the default
    `native_training_precision` ('fp32': the cap of 16 was hit under 'f16x3', see TRUNK_GRAD_FACTOR): all 229 trunk parameters and the
    input receive gradients from the native node (no `_trunk_torch` call) for a cotangent on the [2,512,4,4] map and for a scalar
    through the torch heads; the output meets the rule with F = 2, the gradients with TRUNK_GRAD_FACTOR; everything bit-equal on
    repeat; the running statistics meet the rule and advance by one batch per forward."""
    prec = 'fp32'
    abi = _abi()
    enc = _native_encoder(trunk, monkeypatch)
    assert enc.native_training_precision == prec
    r64, r32 = trunk['ref'][torch.float64], trunk['ref'][torch.float32]
    before = abi.launch_count
    feat, got = _native_grads(enc, trunk, which)
    assert abi.launch_count - before > 400
    if which == 'map':
        _rule(f'trunk {prec} map', feat, r32['feat'], r64['feat'])
        for k, v in r64['stats'].items():
            if 'num_batches' in k:
                assert int(enc.state_dict()[k]) == int(v) == 1
            elif k.startswith(('input_layer', 'body')):
                _rule(f'trunk {prec} {k}', enc.state_dict()[k], r32['stats'][k], v)
    _check_trunk_grads(f'trunk {prec} {which}', enc, got, r32[which], r64[which])
    enc2 = _native_encoder(trunk, monkeypatch)
    feat2, got2 = _native_grads(enc2, trunk, which)
    assert all(torch.equal(a, b) for a, b in zip(got, got2)) and (feat is None or torch.equal(feat, feat2))
    assert all(p.grad is None for p in enc.parameters())          # torch.autograd.grad: nothing accumulated behind the test's back


def test_trunk_native_training_default_is_torch(trunk):
    """The switch is off by default: training takes `_trunk_torch` under autograd as before."""
    import copy
    enc = copy.deepcopy(trunk['enc64']).float().train()
    assert enc.native_training is False
    calls = []
    inner = enc._trunk_torch
    enc._trunk_torch = lambda x: (calls.append(1), inner(x))[1]
    abi = _abi()
    before = abi.launch_count
    with _no_miopen():
        enc(trunk['x'].clone().requires_grad_(True)).sum().backward()
    assert calls == [1] and abi.launch_count == before


def test_trunk_native_training_overflow_repeat(trunk, monkeypatch):
    """An input past the fp16 range flags the split-precision forward: it is repeated on the exact kernels, gives the bits of an
    'fp32' run, and the running statistics advance by exactly one batch."""
    from torch_utils.ops import plain_conv
    big = dict(trunk, x=trunk['x'] * 1e5)
    results = {}
    for prec in ('f16x3', 'fp32'):
        enc = _native_encoder(trunk, monkeypatch)
        enc.native_training_precision = prec
        feat, got = _native_grads(enc, big, 'map')
        if prec == 'f16x3':
            assert plain_conv.overflowed(DEV)
        assert all(int(v) == 1 for k, v in enc.state_dict().items() if 'num_batches' in k and k.startswith(('input_layer', 'body')))
        results[prec] = (feat, got, {k: v.clone() for k, v in enc.state_dict().items() if 'running' in k})
    assert plain_conv.precision == 'f16x3'          # the module-wide setting is untouched
    a, b = results['f16x3'], results['fp32']
    assert torch.equal(a[0], b[0]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1])) and all(torch.equal(a[2][k], b[2][k]) for k in a[2])
    assert bool(torch.isfinite(a[0]).all())


# ---- 5. one optimizer step ------------------------------------------------------------------------------------------------------------

def test_ranger_step_after_native_backward(trunk, monkeypatch):
    """Ranger over encoder.parameters() after a native backward and after a torch backward from the same start: the parameters agree
    within the rule (float64 model and float64 Ranger as the reference); the next eval-mode forward re-packs -- its output differs
    from the pre-step output and meets the rule against the float64 model with the stepped weights."""
    import copy
    from utils.ranger import Ranger
    x, wcode = trunk['x'], trunk['wcode']
    encs = {'hip': _native_encoder(trunk, monkeypatch), 't32': copy.deepcopy(trunk['enc64']).float().train(), 'f64': copy.deepcopy(trunk['enc64']).train()}
    encs['t32'].load_state_dict(trunk['state32'])
    with torch.no_grad():
        before_step = encs['hip'].eval()(x)
    encs['hip'].train()
    for key, enc in encs.items():
        dt = torch.float64 if key == 'f64' else torch.float32
        opt = Ranger(enc.parameters(), lr=1e-3)
        with _no_miopen():
            (enc(x.to(dt)) * wcode.to(dt)).sum().backward()
        assert all(p.grad is not None and p.grad.shape == p.shape for p in enc.parameters()), key
        opt.step()
    for (n, ph), (_, p32), (_, p64) in zip(encs['hip'].named_parameters(), encs['t32'].named_parameters(), encs['f64'].named_parameters()):
        e_hip, e_t32 = float((ph.double() - p64).abs().max()), float((p32.double() - p64).abs().max())
        assert e_hip <= 2 * e_t32 + 1e-7 * float(p64.abs().max()), f'{n}: e_hip {e_hip:.3e} e_torch32 {e_t32:.3e}'
    with torch.no_grad(), _no_miopen():
        after = encs['hip'].eval()(x)
        ref64 = encs['f64'].eval()._forward_torch(x.double())          # the fused eval path is float32 only
        ref32 = encs['t32'].eval()(x)
    assert not torch.equal(after, before_step)
    _rule('eval forward after the step', after, ref32, ref64)
