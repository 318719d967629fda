"""The CLIP loss on the GPU: the fused image preparation and its adjoint, every backward kernel of the image tower alone against
float64, the whole image gradient against float64 autograd through tests/clip_cases.encode_image64 with the float16-weight
composite's autograd on the same device as the yardstick, the power-of-two gradient scale, batch invariance, and CLIPLoss itself
(launch counts, no composite fallback, the gradient reaching a shared leaf).

Measured on an MI355X: see DESIGN.md 3.10 for e_hip / e_half per case."""
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clip_cases as cases
import clip_loss_cases as lcases
from helpers import golden

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U32, U16 = 2.0 ** -24, 2.0 ** -11            # unit roundoffs of float32 and float16


def _abi():
    from torch_utils import _sg3abi as abi
    return abi


def _ct():
    from torch_utils.ops import clip_transformer as ct
    return ct


def _randn(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape)).to(DEV)          # float64


# ---- 1. nearest_up_avg_pool ---------------------------------------------------------------------------------------------------

RESAMPLE_SHAPES = [(7, 1, 32, 32, 3), (7, 2, 64, 64, 3), (7, 3, 96, 96, 3), (7, 8, 256, 256, 3), (3, 2, 5, 9, 3), (2, 5, 7, 6, 3), (7, 32, 1024, 1024, 2)]


@pytest.mark.parametrize('up,k,H,W,C', RESAMPLE_SHAPES)
def test_resample_forward_and_adjoint_against_fp64(up, k, H, W, C):
    """Forward and adjoint on strided views: |hip - fp64| <= 2 max|torch32 - fp64| + 1e-7 max|fp64|, torch32 and fp64 being the two
    torch modules (the definition) in float32 and float64 on the same device; one launch each; the adjoint bit-equal on repeat
    and exactly zero where a source pixel lies in no window."""
    from torch_utils.ops.clip_resample import composite, nearest_up_avg_pool
    abi = _abi()
    B = 1 if H >= 1024 else 2
    base = _randn(up * 1000 + k, B, C, H + 1, W + 2).float()
    x = base[:, :, 1:, 1:-1]                                                    # strided view
    assert not x.is_contiguous()
    x64 = x.double().requires_grad_(True)
    x32 = x.detach().clone().requires_grad_(True)
    xh = x.detach().requires_grad_(True)
    y64, y32 = composite(x64, up, k), composite(x32, up, k)
    before = abi.launch_count
    yh = nearest_up_avg_pool(xh, up, k)
    assert abi.launch_count - before == 1
    assert yh.dtype == torch.float32 and yh.shape == y64.shape == (B, C, up * H // k, up * W // k)
    e_hip, e_t32 = float((yh.double() - y64).abs().max()), float((y32.double() - y64).abs().max())
    print(f'resample up {up} k {k} {H}x{W}: forward e_hip {e_hip:.3e} e_torch32 {e_t32:.3e}')
    assert e_hip <= 2 * e_t32 + 1e-7 * float(y64.abs().max())
    dyb = _randn(up * 1000 + k + 1, B, C, yh.shape[2], yh.shape[3] + 1).float()
    dy = dyb[..., :-1]                                                          # strided upstream gradient
    g64, = torch.autograd.grad(y64, x64, dy.double())
    g32, = torch.autograd.grad(y32, x32, dy)
    before = abi.launch_count
    gh, = torch.autograd.grad(yh, xh, dy, retain_graph=True)
    assert abi.launch_count - before == 1
    gh2, = torch.autograd.grad(yh, xh, dy)
    assert torch.equal(gh, gh2)
    e_hip, e_t32 = float((gh.double() - g64).abs().max()), float((g32.double() - g64).abs().max())
    print(f'resample up {up} k {k} {H}x{W}: adjoint e_hip {e_hip:.3e} e_torch32 {e_t32:.3e}')
    assert e_hip <= 2 * e_t32 + 1e-7 * float(g64.abs().max())
    assert bool((gh[g64 == 0] == 0).all())


def test_resample_double_backward_takes_the_composite():
    from torch_utils.ops.clip_resample import composite, nearest_up_avg_pool
    x = _randn(1, 1, 3, 5, 9).float().requires_grad_(True)
    dy = _randn(2, 1, 3, 7, 13).float().requires_grad_(True)
    g, = torch.autograd.grad(nearest_up_avg_pool(x, 3, 2), x, dy, create_graph=True)
    gg, = torch.autograd.grad(g.sum(), dy)
    ref, = torch.autograd.grad(composite(x, 3, 2), x, dy, create_graph=True)
    rr, = torch.autograd.grad(ref.sum(), dy)
    assert torch.allclose(gg, rr, rtol=1e-6, atol=0)


# ---- 2. the GEMM epilogues of the recording forward and of the backward ------------------------------------------------------------

GUARD = 2
SENTINEL = 777.0


def _dgelu64(u):
    s = torch.sigmoid(1.702 * u)
    return s * (1 + 1.702 * u * (1 - s))


def _grad_gemm_case(K, N, M, epi, mag, seed, a32):
    """One sg3_clip_gemm_grad call; operands as test_gpu_clip._gemm_case draws them (~ mag * N(0, 1), W over sqrt(K), side terms
    ~ mag^2 / 4).  Returns [(hip, ref, bound)], guard_ok, with the elementwise bound of test_gemm_against_fp64:
    (K + 2) 2^-24 (|A| |W|^T + |bias| + |residual|), plus 2^-11 |ref| + 2^-25 for a float16 result."""
    abi, ct = _abi(), _ct()
    w16 = (_randn(seed, N, K) * (mag / math.sqrt(K))).half()
    a = (_randn(seed + 2, M, K) * mag).float()
    a = a if a32 else a.half()
    a64 = a.half().double()
    out_dtype = ct._OUT_DTYPE[epi]
    buf = torch.full([GUARD + M + 66, N], SENTINEL, dtype=out_dtype, device=DEV)
    out = buf[GUARD:GUARD + M]
    acc, mags = a64 @ w16.double().T, a64.abs() @ w16.double().abs().T
    checks = []
    if epi == abi.SG3_CLIP_EPI_RESIDUAL:
        bias, res = (_randn(seed + 1, N) * mag * mag / 4).float(), (_randn(seed + 5, M, N) * mag * mag / 4).float()
        ct.gemm(a, w16, bias, out, epi, M, aux=res)
        checks.append((out.double(), res.double() + acc + bias.double(), (K + 2) * U32 * (mags + bias.double().abs() + res.double().abs())))
    elif epi == abi.SG3_CLIP_EPI_QUICKGELU_SAVE_F16:
        bias = (_randn(seed + 1, N) * mag * mag / 4).float()
        auxbuf = torch.full([GUARD + M + 66, N], SENTINEL, dtype=torch.float16, device=DEV)
        aux = auxbuf[GUARD:GUARD + M]
        ct.gemm(a, w16, bias, out, epi, M, aux=aux)
        v, b = acc + bias.double(), (K + 2) * U32 * (mags + bias.double().abs())
        ref = v * torch.sigmoid(1.702 * v)
        checks.append((out.double(), ref, b + U16 * ref.abs() + 2.0 ** -25))
        checks.append((aux.double(), v, b + U16 * v.abs() + 2.0 ** -25))
        if not (bool((auxbuf[:GUARD] == SENTINEL).all()) and bool((auxbuf[GUARD + M:] == SENTINEL).all())):
            return checks, False
    elif epi == abi.SG3_CLIP_EPI_DQUICKGELU_F16:
        u = (_randn(seed + 6, M, N) * 2).half()
        ct.gemm(a, w16, None, out, epi, M, aux=u)
        d = _dgelu64(u.double())
        ref = acc * d
        # the derivative in float32: a few roundings of terms of size 1 + 1.702 |u| (it passes through zero near u = -1.1, where the
        # error does not shrink with it): 8 * 2^-24 (1 + 1.702 |u|), times |acc|
        checks.append((out.double(), ref, (K + 2) * U32 * mags * d.abs() + 8 * U32 * (1 + 1.702 * u.double().abs()) * acc.abs() + U16 * ref.abs() + 2.0 ** -25))
    else:
        assert epi == abi.SG3_CLIP_EPI_F16
        ct.gemm(a, w16, None, out, epi, M)
        checks.append((out.double(), acc, (K + 2) * U32 * mags + U16 * acc.abs() + 2.0 ** -25))
    return checks, bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + M:] == SENTINEL).all())


@pytest.mark.parametrize('epi,a32', [(3, False), (5, False), (6, False), (6, True), (1, True)],
                         ids=['residual_from', 'quickgelu_save', 'dquickgelu', 'dquickgelu_a32', 'f16_a32'])
@pytest.mark.parametrize('K,N', [(64, 64), (768, 3072), (3072, 768)])
def test_grad_gemm_epilogues_against_fp64(K, N, epi, a32):
    """sg3_clip_gemm_grad alone, |hip - ref| <= the elementwise bound of `_grad_gemm_case`, ref being float64 arithmetic on the same
    float16-rounded operands; M = 1, 50 and 257 (one row, a partial tile, five tile rows), operand magnitudes 1e-2, 1 and 1e2."""
    worst = 0.0
    for M in (1, 50, 257):
        for mag in (1e-2, 1.0, 1e2):
            checks, guard_ok = _grad_gemm_case(K, N, M, epi, mag, seed=M + 1000 * epi + 7 * int(a32), a32=a32)
            assert guard_ok, f'M {M} mag {mag}: wrote outside its rows'
            for hip, ref, bound in checks:
                assert torch.isfinite(hip).all() and torch.isfinite(ref).all()
                ratio = float(((hip - ref).abs() / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, f'M {M} mag {mag}: error / bound = {ratio:.3f}'
    print(f'grad gemm K {K} N {N} epilogue {epi} a32 {a32}: worst error / bound = {worst:.4f}')


@pytest.mark.parametrize('R', [96, 224])
@pytest.mark.parametrize('K', [64, 768])
def test_patch_adjoint_against_fp64(K, R):
    """dTokens[:, 1:] . Wconv scattered to the image, P = 32: bound (K + 2) 2^-24 |A| |W|^T |scale| (float32 result), guard values
    before and after the image gradient untouched, the class-token rows never read into it, with and without the per-sample scale
    and with float16 and float32 token gradients."""
    abi, ct = _abi(), _ct()
    P, B = 32, 3
    g = R // P
    N, M = 3 * P * P, B * g * g
    for mag in (1e-2, 1.0, 1e2):
        for a32 in (False, True):
            wt16 = (_randn(K + R, N, K) * (mag / math.sqrt(K))).half()                       # conv1.weight transposed: [3 P P][K]
            tok = (_randn(K + R + 1, B, g * g + 1, K) * mag).float()
            tok[:, 0] = float('nan')                                                     # the class rows must not be read
            tok = tok if a32 else tok.half()
            scale = torch.tensor([0.5, 4.0, 2.0 ** -20], dtype=torch.float32, device=DEV)
            for sc in (None, scale):
                buf = torch.full([B * 3 * R * R + 2 * 64], SENTINEL, dtype=torch.float32, device=DEV)
                out = buf[64:64 + B * 3 * R * R].view(B, 3, R, R)
                ct.gemm(tok, wt16, None, out, abi.SG3_CLIP_EPI_PATCH_ADJOINT, M, patch=P, resolution=R, scale=sc)
                assert bool((buf[:64] == SENTINEL).all()) and bool((buf[-64:] == SENTINEL).all())
                a64 = tok[:, 1:].half().double().reshape(M, K)
                s64 = (sc.double() if sc is not None else torch.ones(B, dtype=torch.float64, device=DEV)).view(B, 1, 1, 1)

                def fold(t):                                                            # [M, 3 P P] -> [B, 3, R, R]
                    return t.view(B, g, g, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, 3, R, R)

                ref = fold(a64 @ wt16.double().T) * s64
                bound = (K + 2) * U32 * fold(a64.abs() @ wt16.double().abs().T) * s64
                assert torch.isfinite(out).all()
                ratio = float(((out.double() - ref).abs() / bound).max())
                assert ratio <= 1.0, f'mag {mag} a32 {a32} scale {sc is not None}: error / bound = {ratio:.3f}'


# ---- 3. LayerNorm backward -------------------------------------------------------------------------------------------------------

def _ln_bwd_refs(x, dy, gamma):
    """(float64 dx, float32 torch dx) of LayerNorm(x) * gamma (+ beta) for the upstream gradient dy."""
    D = x.shape[-1]
    x64 = x.double().requires_grad_(True)
    ref, = torch.autograd.grad(F.layer_norm(x64, (D,), gamma.double(), None, 1e-5), x64, dy.double())
    x32 = x.clone().requires_grad_(True)
    t32, = torch.autograd.grad(F.layer_norm(x32, (D,), gamma, None, 1e-5), x32, dy)
    return ref, t32


@pytest.mark.parametrize('kind', ['plain', 'offset'])
@pytest.mark.parametrize('rows,D', [(1, 128), (7, 128), (50, 768)])
def test_layernorm_bwd_against_fp64(rows, D, kind):
    """e_hip <= 2 e_torch32 + 1e-7 max|ref|, torch32 being torch's float32 LayerNorm backward on the same inputs.  'plain': rows
    ~ N(0, 1) times 1, 1e-3, 1e3 in turn; 'offset': rows of 1e3 + N(0, 1), where statistics taken on the raw values cancel.  Dense
    rows, strided class rows of a token stream (written into a gradient stream whose other rows stay as they were), accumulating,
    and in place."""
    ct = _ct()
    x64 = _randn(rows * D + 1, rows, D)
    if kind == 'offset':
        x64 = 1e3 + x64
    else:
        x64 = x64 * torch.tensor([1.0, 1e-3, 1e3], dtype=torch.float64, device=DEV)[torch.arange(rows, device=DEV) % 3][:, None]
    x, dy = x64.float(), _randn(rows * D + 2, rows, D).float()
    gamma = (1 + 0.2 * _randn(3, D)).float()
    ref, t32 = _ln_bwd_refs(x, dy, gamma)
    e_t32, scale = float((t32.double() - ref).abs().max()), float(ref.abs().max())
    tol = 2 * e_t32 + 1e-7 * scale
    buf = torch.full([rows + 1, D], 9.0, dtype=torch.float32, device=DEV)
    out = ct.layernorm_bwd(dy, x, gamma, buf[:rows], rows, D)
    assert bool((buf[rows] == 9.0).all())
    e_hip = float((out.double() - ref).abs().max())
    print(f'layernorm_bwd {rows}x{D} {kind}: e_hip {e_hip:.3e} e_torch32 {e_t32:.3e} max|ref| {scale:.3e}')
    assert e_hip <= tol
    # strided: x is the class row of a [rows, 3, D] stream, dx the class row of a gradient stream
    stream = torch.stack([x, x + 1, x * 2], dim=1).contiguous()
    gs = torch.full([rows, 3, D], 5.0, dtype=torch.float32, device=DEV)
    ct.layernorm_bwd(dy, stream, gamma, gs, rows, D, x_stride=3 * D, dx_stride=3 * D)
    assert torch.equal(gs[:, 0], out) and bool((gs[:, 1:] == 5.0).all())
    # accumulating: one more float32 addition
    prev = _randn(rows * D + 4, rows, D).float() * scale
    acc = prev.clone()
    ct.layernorm_bwd(dy, x, gamma, acc, rows, D, accumulate=True)
    assert float(((acc.double() - (prev.double() + ref)).abs() - U32 * (prev.double() + ref).abs()).max()) <= tol
    # in place on dy
    inplace = dy.clone()
    ct.layernorm_bwd(inplace, x, gamma, inplace, rows, D)
    assert torch.equal(inplace, out)


# ---- 4. attention backward ---------------------------------------------------------------------------------------------------------

def _attention_bwd_refs(qkv16, dout16, B, L, heads, dtype):
    qkv = qkv16.to(dtype).requires_grad_(True)
    q, k, v = qkv.view(B, L, 3, heads, 64).unbind(2)
    s = torch.einsum('nihd,njhd->nhij', q, k) / 8.0
    o = torch.einsum('nhij,njhd->nihd', torch.softmax(s, dim=-1), v).reshape(B, L, heads * 64)
    g, = torch.autograd.grad(o, qkv, dout16.to(dtype))
    return g, s.detach()


def _check_attention_bwd(qkv16, dout16, B, L, heads, what):
    ct = _ct()
    D = 64 * heads
    ref, scores = _attention_bwd_refs(qkv16, dout16, B, L, heads, torch.float64)
    yard = _attention_bwd_refs(qkv16, dout16, B, L, heads, torch.float32)[0].half()
    buf = torch.full([B * L + 1, 3 * D], 9.0, dtype=torch.float16, device=DEV)
    out = ct.attention_bwd(qkv16, dout16, buf[:B * L], B, L, heads).view(B, L, 3 * D)
    assert bool((buf[B * L] == 9.0).all())
    assert torch.isfinite(out).all()
    for i, part in enumerate(('dq', 'dk', 'dv')):
        sl = slice(i * D, (i + 1) * D)
        r = ref[..., sl]
        e_hip, e_yard, scale = float((out[..., sl].double() - r).abs().max()), float((yard[..., sl].double() - r).abs().max()), float(r.abs().max())
        print(f'attention_bwd {what} {part}: e_hip {e_hip:.3e} e_yard {e_yard:.3e} max|ref| {scale:.3e}')
        assert e_hip <= 2 * e_yard + U16 * scale, part
    return scores


@pytest.mark.parametrize('heads', [2, 12])
@pytest.mark.parametrize('L', [1, 10, 50, 128])
def test_attention_bwd_against_fp64(L, heads):
    """Per part (dq, dk, dv): e_hip <= 2 e_yard + 2^-11 max|ref|; ref is float64 autograd on the float16-rounded inputs, the yardstick
    float32 torch autograd on the same inputs, rounded to float16 as the kernel's result is."""
    B = 2
    qkv = _randn(L * 7 + heads, B, L, 3 * 64 * heads).half()
    dout = _randn(L * 7 + heads + 1, B, L, 64 * heads).half()
    _check_attention_bwd(qkv, dout, B, L, heads, f'L {L} heads {heads}')


def test_attention_bwd_large_scores_stay_finite():
    """Scores of +-60: the recomputed softmax subtracts the row maximum in both sweeps, nothing overflows, the bound holds."""
    B, L, heads = 2, 50, 2
    sign = torch.where(_randn(5, B, L, 1, heads, 1) > 0, 1.0, -1.0)
    qk = sign * math.sqrt(480.0 / 64) * torch.ones(B, L, 2, heads, 64, dtype=torch.float64, device=DEV) + 0.01 * _randn(6, B, L, 2, heads, 64)
    qkv = torch.cat([qk, _randn(7, B, L, 1, heads, 64)], dim=2).reshape(B, L, 3 * 64 * heads).half()
    dout = _randn(8, B, L, 64 * heads).half()
    scores = _check_attention_bwd(qkv, dout, B, L, heads, 'large scores')
    assert float(scores.max()) > 55 and float(scores.min()) < -55


def test_attention_bwd_refuses_causal():
    ct = _ct()
    abi = _abi()
    qkv, dout = _randn(1, 1, 4, 384).half(), _randn(2, 1, 4, 128).half()
    before = abi.launch_count
    with pytest.raises(RuntimeError, match='causal'):
        ct.attention_bwd(qkv, dout, torch.empty_like(qkv), 1, 4, 2, causal=True)
    assert abi.launch_count == before


# ---- 5. the whole gradient ---------------------------------------------------------------------------------------------------------

_sd, _ref = {}, {}
MAX_BATCH = {'tiny96': 33, 'small': 33, 'b32x2': 3}


def _state(cfg, w_scale):
    if cfg not in _sd:
        _sd[cfg] = cases.state_dict(cfg)
    block = lambda k: 'resblocks' in k and k.endswith('weight') and '.ln_' not in k          # noqa: E731
    return {k: (v * np.float32(w_scale) if block(k) else v) for k, v in _sd[cfg].items()}


def _head64(feats, text64):
    """The loss of CLIPLoss on image features, in float64: [B, E] -> [B, n_text]."""
    f = feats.double()
    f = f / f.norm(dim=-1, keepdim=True)
    return 1 - (1 / 0.07) * f @ text64.t() / 100


def _reference(cfg, w_scale):
    """Once per (cfg, w_scale): images, normalised float64 text features and the float64 gradient of sum(loss) through encode_image64."""
    key = (cfg, w_scale)
    if key not in _ref:
        sd, n = _state(cfg, w_scale), MAX_BATCH[cfg]
        x = torch.from_numpy(cases.images(cfg, n)).to(DEV)
        t = cases.encode_text64(sd, cfg, torch.from_numpy(cases.tokens(cfg, lcases.N_TEXT)), device=DEV)
        t = (t / t.norm(dim=-1, keepdim=True)).detach()
        x64 = x.double().requires_grad_(True)
        g64, = torch.autograd.grad(_head64(cases.encode_image64(sd, cfg, x64, device=DEV), t).sum(), x64)
        _ref[key] = (x, t, g64)
    return _ref[key]


def _models(cfg, w_scale):
    from models.clip import convert_weights
    m = cases.build(cfg, _state(cfg, w_scale), DEV)
    return m, convert_weights(copy.deepcopy(m))


def _image_grad(model, x, text64, impl, mult=1.0):
    """d (mult * mean(loss)) / d image through `impl`, and the launches of (forward, backward).  The composite's patch convolution
    runs on torch's own im2col + GEMM path (still float16 weights and activations): through MIOpen its backward is compiled at first
    use for every batch size where no kernel cache is installed, which took more than the suite's whole budget for one case."""
    abi = _abi()
    xr = x.detach().clone().requires_grad_(True)
    with torch.backends.cudnn.flags(enabled=impl != 'torch'):
        before = abi.launch_count
        loss = _head64(model.encode_image(xr, impl=impl), text64).mean() * mult
        mid = abi.launch_count
        g, = torch.autograd.grad(loss, xr)
    return g, (mid - before, abi.launch_count - mid)


@pytest.mark.parametrize('w_scale', [1, 3])
@pytest.mark.parametrize('cfg', ['tiny96', 'small', 'b32x2'])
def test_image_gradient_against_fp64(cfg, w_scale):
    """d mean(loss) / d image: e_hip <= 2 e_half + 1e-6 max|g64| at every batch; e_half is the autograd of the 'torch' composite with
    float16 weights on the same device and inputs, g64 float64 autograd through encode_image64.  Launches: `launches` forward,
    `launches_backward` backward, nothing else."""
    ct = _ct()
    x, t, g64_sum = _reference(cfg, w_scale)
    m, mh = _models(cfg, w_scale)
    layers = cases.CONFIGS[cfg]['vision_layers']
    for b in (1, 3, 33):
        if b > MAX_BATCH[cfg]:
            continue
        g64 = g64_sum[:b] / (b * lcases.N_TEXT)
        hip, counts = _image_grad(m, x[:b], t, 'hip')
        half, none = _image_grad(mh, x[:b], t, 'torch')
        assert counts == (ct.launches(layers), ct.launches_backward(layers)) and none == (0, 0)
        assert hip.dtype == torch.float32 and hip.shape == x[:b].shape and torch.isfinite(hip).all()
        e_hip, e_half, scale = float((hip.double() - g64).abs().max()), float((half.double() - g64).abs().max()), float(g64.abs().max())
        zeros = float((half == 0).double().mean())
        print(f'{cfg} w_scale {w_scale} batch {b}: e_hip {e_hip:.3e}  e_half {e_half:.3e}  ratio {e_hip / e_half:.3f}  max|g64| {scale:.3e}  '
              f'median|g64| {float(g64.abs().median()):.3e}  zero entries: half {zeros:.4f} hip {float((hip == 0).double().mean()):.4f}')
        assert math.isfinite(e_half) and e_half > 0
        assert e_hip <= 2 * e_half + 1e-6 * scale


@pytest.mark.parametrize('cfg', ['small', 'b32x2'])
def test_gradient_scale_carries_small_and_large_upstream_gradients(cfg, monkeypatch):
    """An upstream gradient times 2^-20 or 2^10, rescaled, meets the bound of the unscaled one (the power of two taken from it on the
    device makes the three runs the same arithmetic); with the scale switched off the 2^-20 run does not (its float16 operands are
    zero)."""
    ct = _ct()
    x, t, g64_sum = _reference(cfg, 1)
    m, mh = _models(cfg, 1)
    b = 3
    g64 = g64_sum[:b] / (b * lcases.N_TEXT)
    half, _ = _image_grad(mh, x[:b], t, 'torch')
    tol = 2 * float((half.double() - g64).abs().max()) + 1e-6 * float(g64.abs().max())
    base, _ = _image_grad(m, x[:b], t, 'hip')
    for mult in (2.0 ** -20, 2.0 ** 10):
        g, _ = _image_grad(m, x[:b], t, 'hip', mult=mult)
        e = float((g.double() / mult - g64).abs().max())
        print(f'{cfg} upstream x {mult:g}: error {e:.3e}, bound {tol:.3e}')
        assert e <= tol
        assert torch.equal(g / mult, base)
    monkeypatch.setattr(ct, 'GRAD_SCALE', False)
    g, _ = _image_grad(m, x[:b], t, 'hip', mult=2.0 ** -20)
    assert float((g.double() * 2.0 ** 20 - g64).abs().max()) > tol


@pytest.mark.parametrize('cfg', ['small', 'b32x2'])
def test_gradient_batch_invariance_and_repeatability(cfg):
    """With a fixed upstream gradient per sample, a sample's image gradient at batch 33 is bit-identical to its gradient alone, and a
    repeat gives the same bits."""
    m = cases.build(cfg, _state(cfg, 1), DEV)
    x = torch.from_numpy(cases.images(cfg, 33)).to(DEV)
    up = _randn(11, 33, cases.CONFIGS[cfg]['embed_dim']).float() * torch.logspace(-6, 2, 33, device=DEV)[:, None]       # every sample its own size

    def grad(xs, ups):
        xr = xs.detach().clone().requires_grad_(True)
        g, = torch.autograd.grad(m.encode_image(xr, impl='hip'), xr, ups)
        return g

    full = grad(x, up)
    assert torch.equal(full, grad(x, up))
    for i in (0, 1, 16, 32):
        assert torch.equal(grad(x[i:i + 1], up[i:i + 1])[0], full[i]), i
    assert torch.equal(grad(x[5:12], up[5:12]), full[5:12])


# ---- 6. the public interface -------------------------------------------------------------------------------------------------------

def test_impl_hip_with_gradient_and_its_refusals():
    """impl='hip' by name records a gradient for an image that requires one; features equal the no_grad kernels' bit for bit; a
    parameter of the image tower that requires a gradient, or an image that does not, keep the present error; the default stays the
    composite; double backward raises."""
    abi, ct = _abi(), _ct()
    m = cases.build('tiny96', device=DEV)
    x = torch.from_numpy(cases.images('tiny96', 2)).to(DEV)
    with torch.no_grad():
        plain = m.encode_image(x, impl='hip')
    xr = x.clone().requires_grad_(True)
    before = abi.launch_count
    f = m.encode_image(xr, impl='hip')
    assert abi.launch_count - before == ct.launches(2) and f.requires_grad and torch.equal(f, plain)
    w = torch.ones_like(f).requires_grad_(True)
    g, = torch.autograd.grad((f * w).sum(), xr, create_graph=True)
    assert g.shape == x.shape and float(g.abs().max()) > 0
    with pytest.raises(RuntimeError, match='differentiate twice'):
        g.sum().backward()
    before = abi.launch_count
    y = m.encode_image(xr)                                                      # the default with gradients on: the composite
    assert abi.launch_count == before and y.requires_grad
    with pytest.raises(RuntimeError, match="impl='hip' needs"):
        m.text_projection.requires_grad_(True)
        m.encode_image(x, impl='hip')                                           # gradients on, image records none
    m.text_projection.requires_grad_(False)
    m.visual.ln_post.weight.requires_grad_(True)
    with pytest.raises(RuntimeError, match="impl='hip' needs"):
        m.encode_image(xr, impl='hip')                                          # a weight gradient is asked for: not this path
    m.visual.ln_post.weight.requires_grad_(False)
    m.text_projection.requires_grad_(True)                                      # a text parameter does not matter to the image tower
    assert m.encode_image(xr, impl='hip').requires_grad
    # the transposed copies follow the prepared weights
    prep = m.__dict__['_sg3_prepared_visual']
    assert prep._grad is not None
    with torch.no_grad():
        m.visual.transformer.resblocks[0].mlp.c_fc.weight.mul_(0.5)
    g2, = torch.autograd.grad(m.encode_image(xr, impl='hip').sum(), xr)
    assert m.__dict__['_sg3_prepared_visual'] is not prep and not torch.equal(g2, g.detach())


@pytest.mark.parametrize('size', [64, 256])
def test_clip_loss_module(size, monkeypatch):
    """CLIPLoss at stylegan_size 64 (against the reference's fixture) and 256 (against float64 through encode_image64): loss and
    d mean(loss) / d image within 2 x the float16-weight composite's error + 1e-6 of the largest entry; launches: 1 + image + text
    forward, backward + 1 backward; no composite runs; the gradient reaches a leaf that also feeds a plain torch op."""
    from criteria.clip_loss import CLIPLoss
    from torch_utils.ops import clip_resample
    abi, ct = _abi(), _ct()
    w_scale, n = 3, 2
    sd = cases.state_dict(lcases.CFG, w_scale=w_scale)
    m = cases.build(lcases.CFG, sd, DEV)
    from models.clip import convert_weights
    mh = convert_weights(copy.deepcopy(m))
    mh.impl = 'torch'                                                           # the yardstick: CLIPLoss on the composite
    text = torch.from_numpy(lcases.tokens()).to(DEV)
    image = torch.from_numpy(lcases.images(size, n)).to(DEV)
    if size == 64:
        g = golden('clip_loss')
        loss64, grad64 = torch.from_numpy(g[f'w{w_scale}/loss64']).to(DEV), torch.from_numpy(g[f'w{w_scale}/grad64']).to(DEV)
    else:
        x64 = image.double().requires_grad_(True)
        t = cases.encode_text64(sd, lcases.CFG, text, device=DEV)
        loss64 = _head64(cases.encode_image64(sd, lcases.CFG, clip_resample.composite(x64, 7, size // 32), device=DEV), t / t.norm(dim=-1, keepdim=True))
        grad64, = torch.autograd.grad(loss64.mean(), x64)
        loss64 = loss64.detach()
    lh = image.clone().requires_grad_(True)
    with torch.backends.cudnn.flags(enabled=False):                              # as in _image_grad: no MIOpen compile for the yardstick's patch convolution
        loss_half = CLIPLoss(lcases.opts(size), model=mh)(lh, text)
        grad_half, = torch.autograd.grad(loss_half.double().mean(), lh)

    def refuse(*a, **k):
        raise AssertionError('a composite ran')

    monkeypatch.setattr(m.visual, 'forward', refuse)
    monkeypatch.setattr(clip_resample, 'composite', refuse)
    loss_fn = CLIPLoss(lcases.opts(size), model=m)
    leaf = image.clone().requires_grad_(True)
    before = abi.launch_count
    loss = loss_fn(leaf, text)
    fwd = abi.launch_count - before
    grad, = torch.autograd.grad(loss.mean(), leaf, retain_graph=True)
    bwd = abi.launch_count - before - fwd
    (loss.mean() + 0.5 * (leaf * leaf).sum()).backward()                        # the leaf also feeds a plain torch op: both gradients arrive
    assert torch.allclose(leaf.grad, grad + leaf.detach(), rtol=1e-6, atol=0)
    assert (fwd, bwd) == (1 + ct.launches(2) + ct.launches(2, 'text'), ct.launches_backward(2) + 1)
    assert loss.dtype == torch.float32 and tuple(loss.shape) == (n, lcases.N_TEXT)
    e_hip, e_half = float((loss.double() - loss64).abs().max()), float((loss_half.double() - loss64).abs().max())
    print(f'CLIPLoss {size}: loss e_hip {e_hip:.3e} e_half {e_half:.3e}')
    assert e_hip <= 2 * e_half + 1e-6 * float(loss64.abs().max())
    e_hip, e_half, scale = float((grad.double() - grad64).abs().max()), float((grad_half.double() - grad64).abs().max()), float(grad64.abs().max())
    print(f'CLIPLoss {size}: gradient e_hip {e_hip:.3e} e_half {e_half:.3e} max|g64| {scale:.3e}')
    assert e_hip <= 2 * e_half + 1e-6 * scale
