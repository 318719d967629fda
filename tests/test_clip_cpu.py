"""CLIP encoders without a GPU: the 'torch' composite against the reference's own outputs (tests/golden/clip.npz, made by
tests/golden/make_golden_clip.py), the state-dict contract, encode_text's edge cases, the C ABI of the transformer kernels
(struct layout and the host-side argument checks, no launch) and the delta_i_c sweep wiring."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch

import clip_cases as cases
from helpers import HERE, golden, maxabs

ROOT = os.path.dirname(HERE)
_models = {}


def model(cfg):
    if cfg not in _models:
        _models[cfg] = cases.build(cfg)
    return _models[cfg]


# ---- 1. composite versus the reference --------------------------------------------------------------------------------------

@pytest.mark.parametrize('cfg', cases.GOLDEN_CONFIGS)
@pytest.mark.parametrize('tower', ['image', 'text'])
def test_composite_matches_reference(cfg, tower):
    """float32 composite vs the reference's float64 outputs: at most 4 x the reference's own float32 error (an equivalent,
    differently ordered composite makes independent roundings of the same size; the error is a max over many elements)."""
    g = golden('clip')
    ref, ref_err = g[f'{cfg}/{tower}64'], float(g[f'{cfg}/{tower}_err'][0])
    m = model(cfg)
    with torch.no_grad():
        if tower == 'image':
            ours = m.encode_image(torch.from_numpy(cases.images(cfg, cases.GOLDEN_BATCH)), impl='torch')
        else:
            ours = m.encode_text(torch.from_numpy(cases.tokens(cfg, cases.GOLDEN_BATCH)), impl='torch')
    assert ours.dtype == torch.float32 and tuple(ours.shape) == ref.shape
    err = maxabs(ours.numpy(), ref)
    print(f'{cfg} {tower}: composite {err:.3e}, reference float32 {ref_err:.3e}, max|ref| {np.abs(ref).max():.3f}')
    assert 0 < ref_err < 1e-5
    assert err <= 4 * ref_err + 1e-7 * np.abs(ref).max()


def test_composite_half_weights_follow_the_reference_conversion():
    """convert_weights: matrices and their biases float16, LayerNorm parameters and embeddings float32; the converted composite's
    error is of the size of the reference's converted model's (within 2 x either way)."""
    from models.clip import convert_weights
    m = convert_weights(cases.build('small'))
    halves = {k for k, v in m.state_dict().items() if v.dtype == torch.float16}
    assert all(('.ln_' in k or k.startswith('ln_final')) == False for k in halves)           # noqa: E712
    assert {'visual.conv1.weight', 'visual.proj', 'text_projection', 'transformer.resblocks.0.attn.in_proj_bias',
            'visual.transformer.resblocks.1.mlp.c_proj.bias', 'visual.transformer.resblocks.0.attn.out_proj.weight'} <= halves
    assert not {'token_embedding.weight', 'positional_embedding', 'visual.class_embedding', 'logit_scale'} & halves
    g = golden('clip')
    with torch.no_grad():
        out = m.encode_image(torch.from_numpy(cases.images('small', cases.GOLDEN_BATCH)))
    assert out.dtype == torch.float16
    err, ref_err = maxabs(out.float().numpy(), g['small/image64']), float(g['small/image_err'][1])
    assert 0.5 * ref_err <= err <= 2 * ref_err, (err, ref_err)


# ---- 2. state dict ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('cfg', cases.GOLDEN_CONFIGS)
def test_state_dict_is_the_references(cfg):
    from models.clip import build_model
    m = model(cfg)
    assert [f'{k}:{list(v.shape)}' for k, v in m.state_dict().items()] == [str(k) for k in golden('clip')[f'{cfg}/keys']]
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == cases.shapes(cfg)
    # every size is rebuilt from the tensors alone, and the round trip is strict
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    sd.update(input_resolution=torch.tensor(224), context_length=torch.tensor(77), vocab_size=torch.tensor(64))   # extras of OpenAI's archives
    m2 = build_model(sd)
    c = cases.CONFIGS[cfg]
    assert (m2.visual.input_resolution, m2.visual.patch_size, m2.visual.width, m2.visual.heads, m2.visual.output_dim, len(m2.visual.transformer.resblocks)) == \
        (c['image_resolution'], c['vision_patch_size'], c['vision_width'], c['vision_width'] // 64, c['embed_dim'], c['vision_layers'])
    assert (m2.context_length, m2.vocab_size, m2.transformer.width, m2.transformer.heads, m2.transformer.layers) == \
        (c['context_length'], c['vocab_size'], c['transformer_width'], c['transformer_heads'], c['transformer_layers'])
    assert not m2.training
    m2.load_state_dict(m.state_dict(), strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k


def test_resnet_towers_are_refused():
    from models.clip import CLIP, build_model
    sd = {k: v for k, v in model('small').state_dict().items() if k != 'visual.proj'}
    with pytest.raises(NotImplementedError, match='not supported'):
        build_model(sd)
    with pytest.raises(NotImplementedError, match='not supported'):
        CLIP(**dict(cases.CONFIGS['small'], vision_layers=(3, 4, 6, 3)))


def test_load_reads_a_state_dict_file(tmp_path):
    from models.clip import load
    m = model('tiny96')
    torch.save(m.state_dict(), tmp_path / 'clip.pt')
    m2 = load(tmp_path / 'clip.pt', 'cpu')
    assert not m2.training and not any(p.requires_grad for p in m2.parameters())
    x = torch.from_numpy(cases.images('tiny96', 1))
    assert torch.equal(m2.encode_image(x), m.encode_image(x))
    (tmp_path / 'junk.pt').write_bytes(b'not a checkpoint')
    with pytest.raises(RuntimeError, match='neither a state-dict file nor a TorchScript archive'):
        load(tmp_path / 'junk.pt')


# ---- 3. encode_text edge cases ------------------------------------------------------------------------------------------------

def test_encode_text_reads_the_argmax_row_and_is_causal():
    cfg = 'small'
    m = model(cfg)
    t = cases.tokens(cfg, 4)
    eot = t.argmax(axis=1)
    assert eot[0] == 76 and (eot[1:] < 76).any()
    with torch.no_grad():
        base = m.encode_text(torch.from_numpy(t))
        # what follows the end-of-text position cannot reach it
        t2 = t.copy()
        for i in range(1, 4):
            t2[i, eot[i] + 1:] = np.arange(1, 77 - eot[i]) % 60 + 1
        assert (t2 != t).any() and (t2.argmax(axis=1) == eot).all()
        assert torch.equal(m.encode_text(torch.from_numpy(t2)), base)
        # a token before it does
        t3 = t.copy(); t3[:, 0] = (t3[:, 0] % 60) + 1
        assert (m.encode_text(torch.from_numpy(t3)) - base).abs().max() > 1e-3
        # the row taken is the argmax row: moving the largest id moves the feature to that row
        x = m.token_embedding(torch.from_numpy(t)) + m.positional_embedding
        rows = m.ln_final(m.transformer(x))
        assert torch.allclose(base, rows[torch.arange(4), torch.from_numpy(eot)] @ m.text_projection, atol=1e-6)
        assert torch.equal(m.encode_text(torch.from_numpy(t).int()), base)


@pytest.mark.parametrize('cfg', cases.GOLDEN_CONFIGS)
def test_restatement_matches_reference_fp64(cfg):
    g = golden('clip')
    sd = cases.state_dict(cfg)
    for tower, ours in (('image', cases.encode_image64(sd, cfg, cases.images(cfg, cases.GOLDEN_BATCH))),
                        ('text', cases.encode_text64(sd, cfg, cases.tokens(cfg, cases.GOLDEN_BATCH)))):
        ref = g[f'{cfg}/{tower}64']
        assert maxabs(ours.numpy(), ref) <= 1e-12 * np.abs(ref).max(), tower


def test_forward_logits():
    m = model('small')
    with torch.no_grad():
        li, lt = m(torch.from_numpy(cases.images('small', 2)), torch.from_numpy(cases.tokens('small', 3)))
    assert tuple(li.shape) == (2, 3) and torch.equal(lt, li.t())
    assert li.abs().max() <= 1 / 0.07 * (1 + 1e-5)


# ---- 4. C ABI ---------------------------------------------------------------------------------------------------------------

def _header_fields(cname):
    src = open(os.path.join(ROOT, 'include', 'sg3_ops.h')).read()
    body = re.search(r'typedef struct ' + cname + r' \{(.*?)\} ' + cname + ';', src, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        parts = decl.split(',')
        for nm in [parts[0].split()[-1]] + [q.strip() for q in parts[1:]]:
            names.append(re.sub(r'\[\d+\]|\*', '', nm))
    return names


def test_clip_structs_match_header():
    from torch_utils import _sg3abi as abi
    for cname, cls, size in (('sg3_clip_layernorm_params', abi.ClipLayernormParams, 4 * 8 + 8 + 4 * 4),
                             ('sg3_clip_gemm_params', abi.ClipGemmParams, 6 * 8 + 6 * 4),
                             ('sg3_clip_attention_params', abi.ClipAttentionParams, 2 * 8 + 4 * 4),
                             ('sg3_clip_embed_params', abi.ClipEmbedParams, 4 * 8 + 4 * 4)):
        assert _header_fields(cname) == [n for n, _ in cls._fields_], cname
        assert ctypes.sizeof(cls) == size, cname
    src = open(os.path.join(ROOT, 'include', 'sg3_ops.h')).read()
    for i, name in enumerate(('F32', 'F16', 'QUICKGELU_F16', 'RESIDUAL', 'PATCH')):
        assert re.search(rf'#define SG3_CLIP_EPI_{name}\s+{i}\b', src) and getattr(abi, f'SG3_CLIP_EPI_{name}') == i


def _gemm_params(**kw):
    from torch_utils import _sg3abi as abi
    bufs = {k: (ctypes.c_char * 64).from_buffer(bytearray(64 + 16)) for k in ('a', 'w', 'out', 'bias', 'pos', 'cls')}
    p = abi.ClipGemmParams()
    for k, b in bufs.items():
        setattr(p, k, (ctypes.addressof(b) + 15) & ~15)
    p.M, p.K, p.N, p.epilogue = 4, 64, 64, abi.SG3_CLIP_EPI_F32
    for k, v in kw.items():
        setattr(p, k, v)
    return p, bufs


@pytest.mark.parametrize('kw,msg', [
    (dict(K=48), 'K 48 is not a multiple of 32'),
    (dict(K=8), 'K 8 is not a multiple of 32'),
    (dict(N=96), 'N 96 is not a multiple of 64'),
    (dict(N=32), 'N 32 is not a multiple of 64'),
    (dict(a=None), 'null tensor'),
    (dict(w=None), 'null tensor'),
    (dict(out=None), 'null tensor'),
    (dict(M=0), 'sizes must be positive'),
    (dict(epilogue=5), 'unknown epilogue'),
    (dict(epilogue=4, K=3 * 64, P=8, R=224, M=28 * 28, pos=None), 'needs pos and cls'),
    (dict(epilogue=4, K=3 * 64, P=8, R=222, M=27 * 27), 'resolution 222'),
    (dict(epilogue=4, K=64, P=8, R=224, M=28 * 28), 'not 3 * patch^2'),
    (dict(epilogue=4, K=3 * 64, P=8, R=224, M=28 * 28 + 1), 'whole number'),
])
def test_clip_gemm_rejects_bad_arguments_on_the_host(kw, msg):
    from torch_utils import _sg3abi as abi
    lib = abi.load()
    p, _keep = _gemm_params(**kw)
    before = abi.launch_count
    assert lib.sg3_clip_gemm(ctypes.byref(p), None) == abi.SG3_BAD_ARG
    assert msg in abi.last_error()
    assert abi.launch_count == before
    assert lib.sg3_clip_gemm(None, None) == abi.SG3_BAD_ARG


def test_clip_other_entry_points_reject_null_and_bad_sizes():
    from torch_utils import _sg3abi as abi
    lib = abi.load()
    buf = ctypes.create_string_buffer(256)
    a = ctypes.addressof(buf)
    assert lib.sg3_clip_layernorm(None, None) == abi.SG3_BAD_ARG
    p = abi.ClipLayernormParams(); p.x, p.gamma, p.beta, p.rows, p.D, p.xRowStride, p.outDtype = a, a, a, 1, 8, 8, abi.SG3_F16
    assert lib.sg3_clip_layernorm(ctypes.byref(p), None) == abi.SG3_BAD_ARG and 'null tensor' in abi.last_error()
    p.out, p.outDtype = a + 64, abi.SG3_F64
    assert lib.sg3_clip_layernorm(ctypes.byref(p), None) == abi.SG3_BAD_ARG and 'float32 or float16' in abi.last_error()
    p.out, p.outDtype = a, abi.SG3_F16
    assert lib.sg3_clip_layernorm(ctypes.byref(p), None) == abi.SG3_BAD_ARG and 'in place' in abi.last_error()
    q = abi.ClipAttentionParams(); q.qkv, q.out, q.B, q.L, q.heads = a, a + 64, 1, 197, 2
    assert lib.sg3_clip_attention(ctypes.byref(q), None) == abi.SG3_BAD_ARG and 'L 197' in abi.last_error()
    q.L, q.qkv = 50, None
    assert lib.sg3_clip_attention(ctypes.byref(q), None) == abi.SG3_BAD_ARG and 'null tensor' in abi.last_error()
    e = abi.ClipEmbedParams(); e.tokens, e.table, e.pos, e.B, e.L, e.D, e.vocab = a, a, a, 1, 1, 1, 1
    assert lib.sg3_clip_embed(ctypes.byref(e), None) == abi.SG3_BAD_ARG and 'null tensor' in abi.last_error()


def test_clip_supported_query():
    from torch_utils import _sg3abi as abi
    from torch_utils.ops import clip_transformer as ct
    lib = abi.load()
    assert lib.sg3_clip_supported(768, 12, 50) == 1 and lib.sg3_clip_supported(512, 8, 77) == 1
    assert lib.sg3_clip_supported(768, 12, 197) == 0 and lib.sg3_clip_supported(100, 2, 50) == 0
    assert lib.sg3_clip_supported(768, 8, 50) == 0 and lib.sg3_clip_supported(128, 2, 0) == 0
    assert ct.image_supported(model('small')) and ct.text_supported(model('small')) and ct.image_supported(model('b32x2'))
    assert not ct.image_supported(cases.build('b16x2'))
    assert ct.launches(12) == 88 and ct.launches(12, 'text') == 87


def test_hip_is_not_taken_on_the_cpu():
    m = model('small')
    x = torch.from_numpy(cases.images('small', 1))
    with pytest.raises(RuntimeError, match="impl='hip' needs a CUDA input"):
        m.encode_image(x, impl='hip')
    with pytest.raises(ValueError):
        m.encode_image(x, impl='triton')
    # gradients flow through the composite
    m2 = cases.build('tiny96').requires_grad_(True)
    y = m2.encode_image(torch.from_numpy(cases.images('tiny96', 1)).requires_grad_(True))
    y.square().sum().backward()
    assert m2.visual.conv1.weight.grad.abs().max() > 0


# ---- 5. sweep wiring --------------------------------------------------------------------------------------------------------

def test_main_loads_the_native_encoder_from_clip_checkpoint_path(tmp_path):
    import delta_i_c_cases as dcases
    from editing.styleclip_global_directions.preprocess import create_delta_i_c as cd
    from helpers import build_product_generator
    G = build_product_generator('Ttiny')
    latents, mean, std = dcases.load_case(golden('delta_i_c'), 'Ttiny')
    keep = 6                                                     # the first channels of the sweep are enough for the wiring
    with open(tmp_path / 'S', 'wb') as f:
        pickle.dump(latents, f)
    with open(tmp_path / 's_stats', 'wb') as f:
        pickle.dump([{'theta': 0.0, 'x': 0.0, 'y': 0.0}, mean, std], f)
    m = model('small')
    torch.save(m.state_dict(), tmp_path / 'clip_small.pt')
    assert cd.Options().clip_checkpoint_path is None
    common = dict(latents_s_path=tmp_path / 'S', latents_statistics_path=tmp_path / 's_stats', num_samples=1, stylegan_size=64)
    a = cd.main(cd.Options(results_path=tmp_path / 'a', clip_checkpoint_path=tmp_path / 'clip_small.pt', **common), generator=G, max_batch=8,
                channel_range=(0, keep), force_fp32=True)
    b = cd.main(cd.Options(results_path=tmp_path / 'b', **common), image_encoder=m.encode_image, generator=G, max_batch=8,
                channel_range=(0, keep), force_fp32=True)
    for name in ('clip_features.npy', 'delta_i_c.npy'):
        assert (tmp_path / 'a' / name).exists() and np.array_equal(np.load(tmp_path / 'a' / name), np.load(tmp_path / 'b' / name), equal_nan=True)
    assert a[0].shape == (keep, 1, 2, 64) and np.array_equal(a[0], b[0]) and np.isfinite(a[0]).all()
    assert np.abs(a[0][:, :, 1] - a[0][:, :, 0]).max() > 0
