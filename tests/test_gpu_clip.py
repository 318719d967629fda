"""CLIP encoders on the GPU: each transformer kernel alone against float64 with derived bounds, the whole encoders against the
float64 restatement of tests/clip_cases.py with the float16-weight composite's error on the same device as the yardstick, batch
invariance, the launch pattern, graph replay, the composite for shapes the kernels refuse, and the delta_i_c sweep on the native
encoder.

Measured on an MI355X: e_hip / e_half is 0.33 - 0.89 over the cases below except small text at w_scale 3,
batch 33 (3.2e-2 against 2.4e-2: 1.36) and b32 text at w_scale 3 (1.7e-1 against 1.7e-1: 1.03); the GEMM's worst error / bound is
0.004 for float32 results at K >= 512 and 0.97 for float16 results (the result's own rounding)."""
import copy
import math

import numpy as np
import pytest
import torch

import clip_cases as cases

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


# ---- 1. GEMM ------------------------------------------------------------------------------------------------------------------

GEMM_SHAPES = [(64, 64), (768, 2304), (768, 3072), (3072, 768), (512, 512)]
GEMM_MS = [1, 50, 77, 150, 257]
PATCH_GRID = {1: (1, 1), 50: (2, 5), 77: (77, 1), 150: (6, 5), 257: (257, 1)}          # M -> (samples, patches per side)
GUARD = 2


def _gemm_case(K, N, M, epi, mag, seed):
    """Runs one GEMM.  Returns (hip float64 [rows, N], ref float64, bound float64, guard_ok).  Operands ~ mag * N(0, 1) with W
    divided by sqrt(K), so the product is ~ mag^2 (1e-4, 1, 1e4); bias, residual and positional terms ~ mag^2 / 4, which keeps
    the largest of the 790 000 results of a case (~ 5.2 sigma) inside float16's 65504 for the float16 epilogues."""
    abi, ct = _abi(), _ct()
    w16 = (_randn(seed, N, K) * (mag / math.sqrt(K))).half()
    bias = (_randn(seed + 1, N) * mag * mag / 4).float()
    out_dtype = ct._OUT_DTYPE[epi]
    sentinel = 777.0
    if epi == abi.SG3_CLIP_EPI_PATCH:
        B, g = PATCH_GRID[M]
        P = int(round(math.sqrt(K // 3)))
        R = g * P
        image = (_randn(seed + 2, B, 3, R, R) * mag).float()
        a64 = image.half().double().view(B, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(M, K)
        pos, cls = (_randn(seed + 3, g * g + 1, N) * mag * mag / 4).float(), (_randn(seed + 4, N) * mag * mag / 4).float()
        rows = B * (g * g + 1)
        buf = torch.full([GUARD + rows + 66, N], sentinel, dtype=torch.float32, device=DEV)
        out = buf[GUARD:GUARD + rows]
        ct.gemm(image, w16, bias, out, epi, M, pos=pos, cls=cls, patch=P, resolution=R)
        acc = a64 @ w16.double().T
        mag_terms = a64.abs() @ w16.double().abs().T + bias.double().abs()
        ref = torch.empty([B, g * g + 1, N], dtype=torch.float64, device=DEV)
        ref[:, 1:] = (acc + bias.double()).view(B, g * g, N) + pos.double()[1:]
        ref[:, 0] = cls.double() + pos.double()[0]
        bound = torch.empty_like(ref)
        bound[:, 1:] = (K + 2) * U32 * (mag_terms.view(B, g * g, N) + pos.double()[1:].abs())
        bound[:, 0] = 2 * U32 * (cls.double().abs() + pos.double()[0].abs())
        ref, bound = ref.view(rows, N), bound.view(rows, N)
    else:
        a16 = (_randn(seed + 2, M, K) * mag).half()
        rows = M
        buf = torch.full([GUARD + rows + 66, N], sentinel, dtype=out_dtype, device=DEV)
        out = buf[GUARD:GUARD + rows]
        res = (_randn(seed + 5, M, N) * mag * mag / 4).float()
        if epi == abi.SG3_CLIP_EPI_RESIDUAL:
            out.copy_(res)
        ct.gemm(a16, w16, bias, out, epi, M)
        v = a16.double() @ w16.double().T + bias.double()
        bound = (K + 2) * U32 * (a16.double().abs() @ w16.double().abs().T + bias.double().abs())
        if epi == abi.SG3_CLIP_EPI_RESIDUAL:
            ref, bound = res.double() + v, bound + (K + 2) * U32 * res.double().abs()
        elif epi == abi.SG3_CLIP_EPI_QUICKGELU_F16:
            ref = v * torch.sigmoid(1.702 * v)
        else:
            ref = v
        if out_dtype == torch.float16:
            bound = bound + U16 * ref.abs() + 2.0 ** -25          # float16 rounding of the result; half a subnormal step near zero
    guard_ok = bool((buf[:GUARD] == sentinel).all()) and bool((buf[GUARD + rows:] == sentinel).all())
    return out.double(), ref, bound, guard_ok


@pytest.mark.parametrize('epi', [0, 1, 2, 3, 4], ids=['f32', 'f16', 'quickgelu', 'residual', 'patch'])
@pytest.mark.parametrize('K,N', GEMM_SHAPES)
def test_gemm_against_fp64(K, N, epi):
    """|hip - ref| <= (K + 2) 2^-24 (|A| |W|^T + |bias| + |residual|) elementwise, plus 2^-11 |ref| for a float16 result; ref is
    float64 arithmetic on the same float16-rounded operands.  K + 2: K products accumulated one at a time in float32, the bias and
    the residual add.  The patch-embedding epilogue exists where K = 3 P^2 with P a multiple of 8 (768, 3072)."""
    abi = _abi()
    if epi == abi.SG3_CLIP_EPI_PATCH and K not in (768, 3072):
        assert math.isqrt(K // 3) ** 2 * 3 != K or math.isqrt(K // 3) % 8
        return
    worst = 0.0
    for M in GEMM_MS:
        for mag in (1e-2, 1.0, 1e2):
            hip, ref, bound, guard_ok = _gemm_case(K, N, M, epi, mag, seed=M + 1000 * epi)
            assert guard_ok, f'M {M} mag {mag}: wrote outside its rows'
            assert torch.isfinite(hip).all() and torch.isfinite(ref).all()
            ratio = float(((hip - ref).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f'M {M} mag {mag}: error / bound = {ratio:.3f}'
    print(f'gemm K {K} N {N} epilogue {epi}: worst error / bound = {worst:.4f}')


def test_gemm_is_row_independent():
    """Row i of a 257-row product is bit-identical to the 1-row product of row i (fixed accumulation order, no split-K)."""
    abi, ct = _abi(), _ct()
    a, w = _randn(1, 257, 768).half(), (_randn(2, 768, 768) / 27.0).half()
    full = ct.gemm(a, w, None, torch.empty([257, 768], dtype=torch.float32, device=DEV), abi.SG3_CLIP_EPI_F32, 257)
    for i in (0, 63, 64, 200, 256):
        one = ct.gemm(a[i:i + 1].contiguous(), w, None, torch.empty([1, 768], dtype=torch.float32, device=DEV), abi.SG3_CLIP_EPI_F32, 1)
        assert torch.equal(one[0], full[i]), i


# ---- 2. LayerNorm and attention -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', [128, 512, 768])
@pytest.mark.parametrize('rows', [1, 50, 151])
def test_layernorm_against_fp64(rows, D):
    """float16 result within 2^-10 relative of float64 (2^-11 is the float16 rounding alone), plus a float32 floor of
    2^-18 (|gamma| (1 + |xhat|) + |beta|): the normalised value carries a few float32 roundings of terms of the size of the row's
    spread (<= 2^-24 * ~8 * max|d| / sigma, max|d| / sigma ~ 4..8 for these rows), and gamma * xhat + beta two more.  Rows: plain
    N(0, 1); 1e3 + N(0, 1) (the cancellation case: the statistics must not be taken on the raw values); scaled by 1e-3 and 1e3.
    Also with a row stride (the class-token rows of a token stream) and in place to float32."""
    ct = _ct()
    x64 = _randn(rows * D, rows, D)
    kinds = torch.arange(rows, device=DEV) % 4
    x64 = torch.where((kinds == 1)[:, None], 1e3 + x64, x64) * torch.where(kinds == 2, 1e-3, 1.0)[:, None] * torch.where(kinds == 3, 1e3, 1.0)[:, None]
    x = x64.float()
    gamma, beta = (1 + 0.2 * _randn(3, D)).float(), (0.1 * _randn(4, D)).float()

    def ref_of(xx):
        xx = xx.double()
        d = xx - xx.mean(-1, keepdim=True)
        xhat = d / (d.pow(2).mean(-1, keepdim=True) + 1e-5).sqrt()
        return xhat * gamma.double() + beta.double(), 2.0 ** -18 * (gamma.double().abs() * (1 + xhat.abs()) + beta.double().abs())

    ref, floor = ref_of(x)
    buf = torch.full([rows + 1, D], 9.0, dtype=torch.float16, device=DEV)
    out = ct.layernorm(x, gamma, beta, buf[:rows], rows, D)
    assert bool((buf[rows] == 9.0).all())
    assert float(((out.double() - ref).abs() / (2.0 ** -10 * ref.abs() + floor)).max()) <= 1.0
    # strided rows: every third row of a [rows, 3, D] stream
    stream = torch.stack([x, x + 1, x * 2], dim=1).contiguous()
    out_s = ct.layernorm(stream, gamma, beta, torch.empty([rows, D], dtype=torch.float16, device=DEV), rows, D, row_stride=3 * D)
    assert torch.equal(out_s, out)
    # in place, float32
    y = x.clone()
    ct.layernorm(y, gamma, beta, y, rows, D)
    assert float(((y.double() - ref).abs() / (2 * U32 * ref.abs() + floor)).max()) <= 1.0


def _attention_ref(qkv, B, L, heads, causal):
    q, k, v = qkv.double().view(B, L, 3, heads, 64).unbind(2)
    s = torch.einsum('nihd,njhd->nhij', q, k) / 8.0
    if causal:
        s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=DEV).triu(1), float('-inf'))
    o = torch.einsum('nhij,njhd->nihd', torch.softmax(s, dim=-1), v).reshape(B, L, heads * 64)
    # float32 score error: 64 products summed one at a time, the scale -- (64 + 2) 2^-24 sum |q| |k| / 8; exp turns an absolute
    # score error e into a relative weight error ~ e, twice over the normalisation
    ds = 66 * U32 * float(torch.einsum('nihd,njhd->nhij', q.abs(), k.abs()).max()) / 8.0
    return o, (2.0 ** -10 + 2 * ds) * float(v.abs().max())


@pytest.mark.parametrize('heads', [2, 12])
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('L', [2, 10, 50, 77])
def test_attention_against_fp64(L, causal, heads):
    """Within 2^-10 max|v| of float64 attention on the same float16 q, k, v (the float16 result's rounding is 2^-11 of it), plus
    the float32 score error carried through the softmax."""
    ct = _ct()
    B = 3
    qkv = _randn(L * 7 + heads, B, L, 3 * 64 * heads).half()
    buf = torch.full([B * L + 1, 64 * heads], 9.0, dtype=torch.float16, device=DEV)
    out = ct.attention(qkv, buf[:B * L], B, L, heads, causal)
    assert bool((buf[B * L] == 9.0).all())
    ref, tol = _attention_ref(qkv, B, L, heads, causal)
    err = float((out.view(B, L, -1).double() - ref).abs().max())
    print(f'attention L {L} causal {causal} heads {heads}: error {err:.3e}, bound {tol:.3e}')
    assert err <= tol


def test_attention_large_scores_stay_finite():
    """Causal, scores of +-60 (q . k / 8): the softmax is taken after subtracting the row maximum, so nothing overflows."""
    ct = _ct()
    B, L, heads = 2, 77, 2
    sign = torch.where(_randn(5, B, L, 1, heads, 1) > 0, 1.0, -1.0)
    qk = sign * math.sqrt(480.0 / 64) * torch.ones(B, L, 2, heads, 64, dtype=torch.float64, device=DEV) + 0.01 * _randn(6, B, L, 2, heads, 64)
    qkv = torch.cat([qk, _randn(7, B, L, 1, heads, 64)], dim=2).reshape(B, L, 3 * 64 * heads).half()
    out = ct.attention(qkv, torch.empty([B * L, 64 * heads], dtype=torch.float16, device=DEV), B, L, heads, True)
    ref, tol = _attention_ref(qkv, B, L, heads, True)
    q, k, _ = qkv.double().view(B, L, 3, heads, 64).unbind(2)
    s = torch.einsum('nihd,njhd->nhij', q, k) / 8.0
    assert float(s.max()) > 55 and float(s.min()) < -55
    assert torch.isfinite(out).all()
    assert float((out.view(B, L, -1).double() - ref).abs().max()) <= tol


# ---- 3. whole encoders ----------------------------------------------------------------------------------------------------------

_sd = {}


def _state(cfg, w_scale):
    """Seeded weights, generated once per configuration; `w_scale` multiplies the block matrices (as cases.state_dict does)."""
    if cfg not in _sd:
        _sd[cfg] = cases.state_dict(cfg)
    block = lambda k: 'resblocks' in k and k.endswith('weight') and '.ln_' not in k          # noqa: E731
    return {k: (v * np.float32(w_scale) if block(k) else v) for k, v in _sd[cfg].items()}


def _encoder_errors(cfg, tower, w_scale, batches):
    sd = _state(cfg, w_scale)
    from models.clip import convert_weights
    m = cases.build(cfg, sd, DEV)
    mh = convert_weights(copy.deepcopy(m))
    n = max(batches)
    x = torch.from_numpy(cases.images(cfg, n) if tower == 'image' else cases.tokens(cfg, n)).to(DEV)
    ref = (cases.encode_image64 if tower == 'image' else cases.encode_text64)(sd, cfg, x, device=DEV)
    abi = _abi()
    for b in batches:
        with torch.no_grad():
            before = abi.launch_count
            hip = (m.encode_image if tower == 'image' else m.encode_text)(x[:b], impl='hip')
            launched = abi.launch_count - before
            half = (mh.encode_image if tower == 'image' else mh.encode_text)(x[:b], impl='torch')
        assert hip.dtype == torch.float32 and half.dtype == torch.float16 and tuple(hip.shape) == (b, cases.CONFIGS[cfg]['embed_dim'])
        layers = cases.CONFIGS[cfg]['vision_layers' if tower == 'image' else 'transformer_layers']
        assert launched == _ct().launches(layers, 'visual' if tower == 'image' else 'text')
        e_hip, e_half = float((hip.double() - ref[:b]).abs().max()), float((half.double() - ref[:b]).abs().max())
        scale = float(ref[:b].abs().max())
        print(f'{cfg} {tower} w_scale {w_scale} batch {b}: e_hip {e_hip:.3e}  e_half {e_half:.3e}  max|ref| {scale:.3f}')
        assert math.isfinite(e_half) and e_half > 0
        assert e_hip <= 2 * e_half + 1e-6 * scale


@pytest.mark.parametrize('w_scale', [1, 3])
@pytest.mark.parametrize('tower', ['image', 'text'])
@pytest.mark.parametrize('cfg', ['small', 'tiny96', 'b32x2'])
def test_encoders_against_fp64(cfg, tower, w_scale):
    """e_hip <= 2 e_half + 1e-6 max|ref| at batches 1, 3 and 33: e_half is the error of the 'torch' composite with float16 weights
    (the reference's convert_weights arithmetic; the composite is pinned to the reference by tests/test_clip_cpu.py) on the same
    device and inputs; the kernels keep the residual stream in float32 and round only GEMM operands, so they sit below it."""
    _encoder_errors(cfg, tower, w_scale, (1, 3, 33))


@pytest.mark.parametrize('w_scale', [1, 3])
@pytest.mark.parametrize('tower', ['image', 'text'])
def test_full_depth_encoders_against_fp64(tower, w_scale):
    """All twelve layers at the ViT-B/32 widths, batch 2."""
    _encoder_errors('b32', tower, w_scale, (2,))


# ---- 4. batch invariance and launch pattern ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('cfg', ['small', 'b32x2'])
def test_batch_invariance_and_repeatability(cfg):
    m = cases.build(cfg, _state(cfg, 1), DEV)
    img, tok = torch.from_numpy(cases.images(cfg, 33)).to(DEV), torch.from_numpy(cases.tokens(cfg, 33)).to(DEV)
    with torch.no_grad():
        fi, ft = m.encode_image(img), m.encode_text(tok)
        assert torch.equal(fi, m.encode_image(img)) and torch.equal(ft, m.encode_text(tok))
        for i in (0, 1, 16, 32):
            assert torch.equal(m.encode_image(img[i:i + 1])[0], fi[i]), i
            assert torch.equal(m.encode_text(tok[i:i + 1])[0], ft[i]), i
        assert torch.equal(m.encode_image(img[5:12]), fi[5:12])


def test_default_impl_launch_count_and_reprepare(monkeypatch):
    abi, ct = _abi(), _ct()
    m = cases.build('small', _state('small', 1), DEV)
    img = torch.from_numpy(cases.images('small', 3)).to(DEV)
    with torch.no_grad():
        before = abi.launch_count
        a = m.encode_image(img)                                   # default impl: CUDA input, gradients off -> the kernels
        assert abi.launch_count - before == ct.launches(2) == 18
        prep = m.__dict__['_sg3_prepared_visual']
        m.encode_image(img)
        assert m.__dict__['_sg3_prepared_visual'] is prep          # unchanged weights: no new copy
        before = abi.launch_count
        t = m.encode_image(img, impl='torch')
        assert abi.launch_count == before
        assert float((a - t).abs().max()) < 1e-2 * float(t.abs().max())
        # an in-place edit re-prepares and changes the result
        m.visual.transformer.resblocks[1].mlp.c_fc.weight.mul_(0.5)
        b = m.encode_image(img)
        assert m.__dict__['_sg3_prepared_visual'] is not prep and not torch.equal(a, b)
        sd2 = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        ref = cases.encode_image64(sd2, 'small', img, device=DEV)
        assert float((b.double() - ref).abs().max()) < 1e-2 * float(ref.abs().max())
        # a stale copy during a capture raises instead of preparing inside the graph
        m.visual.ln_post.bias.add_(1.0)
        monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
        before = abi.launch_count
        with pytest.raises(RuntimeError, match='stale during a graph capture'):
            m.encode_image(img)
        assert abi.launch_count == before
        monkeypatch.undo()
        assert not torch.equal(m.encode_image(img), b)
    # with gradients on, the default is the composite
    m2 = cases.build('tiny96', device=DEV).requires_grad_(True)
    before = abi.launch_count
    y = m2.encode_image(torch.from_numpy(cases.images('tiny96', 1)).to(DEV))
    assert abi.launch_count == before and y.requires_grad


def test_graph_replay_equals_eager():
    m = cases.build('small', _state('small', 1), DEV)
    x = torch.from_numpy(cases.images('small', 4)).to(DEV)
    other = torch.from_numpy(cases.images('small', 4, seed=2)).to(DEV)
    with torch.no_grad():
        eager = m.encode_image(x).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.encode_image(x)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = m.encode_image(x)
        x.copy_(other)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, m.encode_image(other))
        x.copy_(torch.from_numpy(cases.images('small', 4)).to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---- 5. a shape the kernels refuse ------------------------------------------------------------------------------------------------

def test_unsupported_shape_runs_the_composite():
    """197 tokens (ViT-B/16's sequence) on a 2-layer model: not an error, the composite answers."""
    abi, ct = _abi(), _ct()
    m = cases.build('b16x2', device=DEV)
    assert not ct.image_supported(m) and ct.text_supported(m)
    img = torch.from_numpy(cases.images('b16x2', 2)).to(DEV)
    with torch.no_grad():
        before = abi.launch_count
        f = m.encode_image(img)
        assert abi.launch_count == before
        assert tuple(f.shape) == (2, 64) and torch.isfinite(f).all()
        ref = cases.encode_image64(cases.state_dict('b16x2'), 'b16x2', img, device=DEV)
        assert float((f.double() - ref).abs().max()) < 1e-4 * float(ref.abs().max())
        with pytest.raises(RuntimeError, match="impl='hip' needs"):
            m.encode_image(img, impl='hip')


# ---- 6. the sweep ---------------------------------------------------------------------------------------------------------------

def test_sweep_on_the_native_encoder_is_batch_invariant():
    """compute_clip_features packs items of several channels into batches of 32; with the native encoder every item's features are
    bit-identical to encoding that item's image alone (the images are rendered in the same batches both times)."""
    import delta_i_c_cases as dcases
    from editing.styleclip_global_directions.preprocess import create_delta_i_c as cd
    from helpers import build_product_generator, golden
    G = build_product_generator('Ttiny', device=DEV)
    latents, mean, std = dcases.load_case(golden('delta_i_c'), 'Ttiny')
    latents = {k: torch.from_numpy(v).to(DEV) for k, v in latents.items()}
    m = cases.build('small', _state('small', 1), DEV)
    abi = _abi()
    channels = (0, 20)                                           # 20 channels x 2 samples x 2 directions = 80 items: 32 + 32 + 16
    sizes = []

    def one_by_one(images):
        sizes.append(int(images.shape[0]))
        return torch.cat([m.encode_image(images[i:i + 1]) for i in range(images.shape[0])])

    before = abi.launch_count
    packed = cd.compute_clip_features(G, latents, mean, std, m.encode_image, max_batch=32, channel_range=channels, force_fp32=True)
    assert abi.launch_count - before >= 3 * 18
    single = cd.compute_clip_features(G, latents, mean, std, one_by_one, max_batch=32, channel_range=channels, force_fp32=True)
    assert sizes == [32, 32, 16]
    assert packed.dtype == torch.float32 and tuple(packed.shape) == (20, dcases.NUM_SAMPLES, 2, 64)
    assert torch.equal(packed, single)
    assert float((packed[:, :, 1] - packed[:, :, 0]).abs().max()) > 0
