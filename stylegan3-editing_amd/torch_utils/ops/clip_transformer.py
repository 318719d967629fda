"""CLIP's ViT encoders on the fused HIP transformer kernels (csrc/sg3_clip.hip, include/sg3_ops.h sg3_clip_*).

`layernorm`, `gemm`, `attention` and `embed` are the thin bindings: one launch each on the current stream, tensors checked here,
sizes checked by the library.  `encode_image` / `encode_text` run a whole tower of a `models.clip.CLIP` from them: two launches
for the stem, seven per block (LayerNorm, QKV GEMM, attention, projection GEMM + residual, LayerNorm, GEMM + QuickGELU, GEMM +
residual) and two for the head; between the input and the features there are only allocations and, for text, the gather of the
end-of-text rows.  No host synchronisation, so a call can be captured in a HIP graph.

`encode_image` records an autograd node when gradients are on and the image requires one (weights are frozen: the gradient is
with respect to the image only).  The recording forward has the same launches and the same arithmetic; it keeps, per block, the
float32 stream at the block's entry and after the attention branch, the float16 qkv and the float16 MLP pre-activation
(22 * rows * width bytes), plus the stream before ln_pre and after the last block.  The backward is `launches_backward(layers)`
= 7 per block + 5 launches: `layernorm_bwd`, `attention_bwd`, `grad_scale` and the data-gradient epilogues of `gemm` on
pre-transposed float16 copies of the matrices (`PreparedTower.grad_weights`, built on the first recording call).

`prepared(model, tower, device)` holds what the kernels read: the matrices in float16 in their stored [out][in] order (the two
output projections transposed to it), everything else in float32.  The copy is keyed by the `(data_ptr, _version)` of every
parameter of the tower and rebuilt when one changes (in-place edits bump `_version`); it is never rebuilt while a graph is being
captured, where a stale key raises.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from .. import _sg3abi as abi

EPS = 1e-5
GRAD_SCALE = True       # the per-sample power of two of the backward; False only shows what is lost without it (tests)


def supported(width, heads, L):
    """Host-only: whether the kernels run a transformer of this width, head count and sequence length."""
    return bool(abi.load().sg3_clip_supported(int(width), int(heads), int(L)))


def _need(t, dtype, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise RuntimeError(f'clip kernels: {what} must be a contiguous CUDA {dtype} tensor, got {getattr(t, "dtype", type(t))} '
                           f'{list(getattr(t, "shape", []))} on {getattr(t, "device", None)}')
    return t


def _call(fn, p, device, what):
    with torch.cuda.device(device):
        abi.check(fn(ctypes.byref(p), abi.stream_ptr(device)), what)


def layernorm(x, gamma, beta, out, rows, D, row_stride=None, eps=EPS):
    """out [rows, D] (float16 or float32) = LayerNorm of the rows x.view(-1)[r * row_stride : r * row_stride + D]; out may be x (float32)."""
    _need(x, torch.float32, 'x'); _need(gamma, torch.float32, 'gamma'); _need(beta, torch.float32, 'beta')
    _need(out, torch.float32 if out.dtype == torch.float32 else torch.float16, 'out')
    row_stride = D if row_stride is None else int(row_stride)
    if gamma.numel() != D or beta.numel() != D or out.numel() != rows * D or x.numel() < (rows - 1) * row_stride + D:
        raise RuntimeError(f'clip layernorm: sizes do not match (rows {rows}, D {D}, stride {row_stride}, x {x.numel()}, out {out.numel()})')
    p = abi.ClipLayernormParams()
    p.x, p.gamma, p.beta, p.out = abi.ptr(x), abi.ptr(gamma), abi.ptr(beta), abi.ptr(out)
    p.xRowStride, p.rows, p.D, p.outDtype, p.eps = row_stride, int(rows), int(D), abi.dtype_code(out.dtype), float(eps)
    _call(abi.load().sg3_clip_layernorm, p, x.device, 'sg3_clip_layernorm')
    return out


_OUT_DTYPE = {abi.SG3_CLIP_EPI_F32: torch.float32, abi.SG3_CLIP_EPI_F16: torch.float16, abi.SG3_CLIP_EPI_QUICKGELU_F16: torch.float16,
              abi.SG3_CLIP_EPI_RESIDUAL: torch.float32, abi.SG3_CLIP_EPI_PATCH: torch.float32, abi.SG3_CLIP_EPI_QUICKGELU_SAVE_F16: torch.float16,
              abi.SG3_CLIP_EPI_DQUICKGELU_F16: torch.float16, abi.SG3_CLIP_EPI_PATCH_ADJOINT: torch.float32}
_A32_OK = (abi.SG3_CLIP_EPI_F16, abi.SG3_CLIP_EPI_DQUICKGELU_F16, abi.SG3_CLIP_EPI_PATCH_ADJOINT)


def gemm(a, w, bias, out, epilogue, M, pos=None, cls=None, patch=0, resolution=0, aux=None, scale=None):
    """out = a [M, K] . w [N, K]^T (+ bias) through `epilogue` (abi.SG3_CLIP_EPI_*); for SG3_CLIP_EPI_PATCH a is the float32 image
    [B, 3, R, R], out the float32 token stream [B, g*g + 1, N] and M = B * g * g.  `aux`: the residual to read
    (SG3_CLIP_EPI_RESIDUAL, float32 [M, N], optional), the pre-activation to write (SG3_CLIP_EPI_QUICKGELU_SAVE_F16) or to read
    (SG3_CLIP_EPI_DQUICKGELU_F16), float16 [M, N].  A float32 `a` is rounded to float16 by the kernel for the epilogues of
    `_A32_OK`.  SG3_CLIP_EPI_PATCH_ADJOINT: a is the token gradient [B, g*g + 1, K], w conv1.weight transposed [3*P*P, K], out the
    float32 image gradient [B, 3, R, R], times scale[b] when `scale` (float32 [B]) is given."""
    patchy = epilogue == abi.SG3_CLIP_EPI_PATCH
    a32 = a.dtype == torch.float32 and epilogue in _A32_OK
    _need(a, torch.float32 if patchy or a32 else torch.float16, 'a'); _need(w, torch.float16, 'w'); _need(out, _OUT_DTYPE[epilogue], 'out')
    N, K = int(w.shape[0]), int(w.shape[1])
    if bias is not None and _need(bias, torch.float32, 'bias').numel() != N:
        raise RuntimeError(f'clip gemm: bias has {bias.numel()} entries, N is {N}')
    if aux is not None:
        if epilogue not in (abi.SG3_CLIP_EPI_RESIDUAL, abi.SG3_CLIP_EPI_QUICKGELU_SAVE_F16, abi.SG3_CLIP_EPI_DQUICKGELU_F16):
            raise RuntimeError(f'clip gemm: epilogue {epilogue} takes no aux')
        if _need(aux, torch.float32 if epilogue == abi.SG3_CLIP_EPI_RESIDUAL else torch.float16, 'aux').numel() != M * N:
            raise RuntimeError(f'clip gemm: aux has {aux.numel()} entries, M * N is {M * N}')
    elif epilogue in (abi.SG3_CLIP_EPI_QUICKGELU_SAVE_F16, abi.SG3_CLIP_EPI_DQUICKGELU_F16):
        raise RuntimeError(f'clip gemm: epilogue {epilogue} needs aux')
    if epilogue == abi.SG3_CLIP_EPI_PATCH_ADJOINT:
        g = resolution // max(patch, 1)
        B = M // max(g * g, 1)
        if patch <= 0 or g <= 0 or M % (g * g) or a.numel() != B * (g * g + 1) * K or out.numel() != B * 3 * resolution * resolution or N != 3 * patch * patch \
                or (scale is not None and _need(scale, torch.float32, 'scale').numel() != B):
            raise RuntimeError(f'clip gemm: patch adjoint sizes do not match (M {M}, patch {patch}, resolution {resolution}, N {N}, K {K})')
    elif scale is not None:
        raise RuntimeError(f'clip gemm: epilogue {epilogue} takes no scale')
    elif patchy:
        g = resolution // max(patch, 1)
        _need(pos, torch.float32, 'pos'); _need(cls, torch.float32, 'cls')
        if M % max(g * g, 1) or a.numel() != (M // max(g * g, 1)) * 3 * resolution * resolution or out.numel() != (M // max(g * g, 1)) * (g * g + 1) * N \
                or pos.numel() != (g * g + 1) * N or cls.numel() != N:
            raise RuntimeError(f'clip gemm: patch embedding sizes do not match (M {M}, patch {patch}, resolution {resolution}, N {N})')
    elif a.numel() != M * K or out.numel() != M * N:
        raise RuntimeError(f'clip gemm: sizes do not match (M {M}, K {K}, N {N}, a {a.numel()}, out {out.numel()})')
    if aux is not None or a32 or epilogue > abi.SG3_CLIP_EPI_PATCH:          # the recording forward and the backward: sg3_clip_gemm_grad
        p = abi.ClipGemmGradParams()
        p.a, p.w, p.bias, p.out, p.aux, p.scale = abi.ptr(a), abi.ptr(w), abi.ptr(bias), abi.ptr(out), abi.ptr(aux), abi.ptr(scale)
        p.M, p.K, p.N, p.epilogue, p.P, p.R, p.aF32 = int(M), K, N, int(epilogue), int(patch), int(resolution), int(a32)
        _call(abi.load().sg3_clip_gemm_grad, p, w.device, 'sg3_clip_gemm_grad')
        return out
    p = abi.ClipGemmParams()
    p.a, p.w, p.bias, p.out, p.pos, p.cls = abi.ptr(a), abi.ptr(w), abi.ptr(bias), abi.ptr(out), abi.ptr(pos), abi.ptr(cls)
    p.M, p.K, p.N, p.epilogue, p.P, p.R = int(M), K, N, int(epilogue), int(patch), int(resolution)
    _call(abi.load().sg3_clip_gemm, p, w.device, 'sg3_clip_gemm')
    return out


def attention(qkv, out, B, L, heads, causal):
    """qkv float16 [B, L, 3 * 64 * heads] -> out float16 [B, L, 64 * heads]."""
    _need(qkv, torch.float16, 'qkv'); _need(out, torch.float16, 'out')
    if qkv.numel() != B * L * 192 * heads or out.numel() != B * L * 64 * heads:
        raise RuntimeError(f'clip attention: sizes do not match (B {B}, L {L}, heads {heads}, qkv {qkv.numel()}, out {out.numel()})')
    p = abi.ClipAttentionParams()
    p.qkv, p.out, p.B, p.L, p.heads, p.causal = abi.ptr(qkv), abi.ptr(out), int(B), int(L), int(heads), int(bool(causal))
    _call(abi.load().sg3_clip_attention, p, qkv.device, 'sg3_clip_attention')
    return out


def layernorm_bwd(dy, x, gamma, dx, rows, D, dy_stride=None, x_stride=None, dx_stride=None, accumulate=False, eps=EPS):
    """The input gradient of LayerNorm for float32 rows (strides in elements, D by default): dx (+)= rstd (g - mean g - xhat mean(g xhat)),
    g = gamma dy; the statistics of x are taken as `layernorm` takes them.  dx may be dy."""
    _need(dy, torch.float32, 'dy'); _need(x, torch.float32, 'x'); _need(gamma, torch.float32, 'gamma'); _need(dx, torch.float32, 'dx')
    sd, sx, so = (D if v is None else int(v) for v in (dy_stride, x_stride, dx_stride))
    if gamma.numel() != D or min(sd, sx, so) < D or any(t.numel() < (rows - 1) * st + D for t, st in ((dy, sd), (x, sx), (dx, so))):
        raise RuntimeError(f'clip layernorm_bwd: sizes do not match (rows {rows}, D {D}, strides {sd}, {sx}, {so}; dy {dy.numel()}, x {x.numel()}, dx {dx.numel()})')
    p = abi.ClipLayernormBwdParams()
    p.dy, p.x, p.gamma, p.dx = abi.ptr(dy), abi.ptr(x), abi.ptr(gamma), abi.ptr(dx)
    p.dyRowStride, p.xRowStride, p.dxRowStride, p.rows, p.D, p.accumulate, p.eps = sd, sx, so, int(rows), int(D), int(bool(accumulate)), float(eps)
    _call(abi.load().sg3_clip_layernorm_bwd, p, x.device, 'sg3_clip_layernorm_bwd')
    return dx


def attention_bwd(qkv, dout, dqkv, B, L, heads, causal=False):
    """qkv float16 [B, L, 3 * 64 * heads] (as saved), dout float16 [B, L, 64 * heads] -> dqkv float16 like qkv.  Non-causal only."""
    _need(qkv, torch.float16, 'qkv'); _need(dout, torch.float16, 'dout'); _need(dqkv, torch.float16, 'dqkv')
    if qkv.numel() != B * L * 192 * heads or dout.numel() != B * L * 64 * heads or dqkv.numel() != qkv.numel():
        raise RuntimeError(f'clip attention_bwd: sizes do not match (B {B}, L {L}, heads {heads}, qkv {qkv.numel()}, dout {dout.numel()}, dqkv {dqkv.numel()})')
    p = abi.ClipAttentionBwdParams()
    p.qkv, p.dout, p.dqkv, p.B, p.L, p.heads, p.causal = abi.ptr(qkv), abi.ptr(dout), abi.ptr(dqkv), int(B), int(L), int(heads), int(bool(causal))
    _call(abi.load().sg3_clip_attention_bwd, p, qkv.device, 'sg3_clip_attention_bwd')
    return dqkv


def grad_scale(g):
    """g float32 [B, E] -> (float16 [B, E] = g * 2^s_b, float32 [B] = 2^-s_b): per row, the power of two that puts max|g[b]| into
    [8, 16).  Taken on the device."""
    _need(g, torch.float32, 'g')
    B, E = (int(v) for v in g.shape)
    out, inv = torch.empty([B, E], dtype=torch.float16, device=g.device), torch.empty([B], dtype=torch.float32, device=g.device)
    p = abi.ClipGradScaleParams()
    p.g, p.out16, p.inv, p.B, p.E = abi.ptr(g), abi.ptr(out), abi.ptr(inv), B, E
    _call(abi.load().sg3_clip_grad_scale, p, g.device, 'sg3_clip_grad_scale')
    return out, inv


def embed(tokens, table, pos, out):
    """out float32 [B, L, D] = table[tokens] + pos."""
    _need(tokens, torch.int64, 'tokens'); _need(table, torch.float32, 'table'); _need(pos, torch.float32, 'pos'); _need(out, torch.float32, 'out')
    B, L = (int(v) for v in tokens.shape)
    vocab, D = (int(v) for v in table.shape)
    if pos.numel() != L * D or out.numel() != B * L * D:
        raise RuntimeError(f'clip embed: sizes do not match (B {B}, L {L}, D {D}, pos {pos.numel()}, out {out.numel()})')
    p = abi.ClipEmbedParams()
    p.tokens, p.table, p.pos, p.out, p.B, p.L, p.D, p.vocab = abi.ptr(tokens), abi.ptr(table), abi.ptr(pos), abi.ptr(out), B, L, D, vocab
    _call(abi.load().sg3_clip_embed, p, tokens.device, 'sg3_clip_embed')
    return out


# ---- prepared weights -------------------------------------------------------------------------------------------------------

def _tower_params(model, tower):
    if tower == 'visual':
        v = model.visual
        return [v.conv1.weight, v.class_embedding, v.positional_embedding, v.proj] + list(v.ln_pre.parameters()) + list(v.ln_post.parameters()) \
            + list(v.transformer.parameters())
    return [model.token_embedding.weight, model.positional_embedding, model.text_projection] + list(model.ln_final.parameters()) \
        + list(model.transformer.parameters())


def _key(model, tower, device):
    return (str(device),) + tuple((q.data_ptr(), q._version) for q in _tower_params(model, tower))


class PreparedTower:
    def __init__(self, model, tower, device):
        def f16(t):
            return t.detach().to(device=device, dtype=torch.float16).contiguous()

        def f32(t):
            return t.detach().to(device=device, dtype=torch.float32).contiguous()

        with torch.no_grad():
            if tower == 'visual':
                v = model.visual
                self.conv = f16(v.conv1.weight.detach().reshape(v.conv1.weight.shape[0], -1))
                self.cls, self.pos = f32(v.class_embedding), f32(v.positional_embedding)
                self.ln_pre = (f32(v.ln_pre.weight), f32(v.ln_pre.bias))
                self.ln_out = (f32(v.ln_post.weight), f32(v.ln_post.bias))
                self.proj = f16(v.proj.detach().t())
                transformer = v.transformer
            else:
                self.table, self.pos = f32(model.token_embedding.weight), f32(model.positional_embedding)
                self.ln_out = (f32(model.ln_final.weight), f32(model.ln_final.bias))
                self.proj = f16(model.text_projection.detach().t())
                transformer = model.transformer
            self.blocks = [dict(ln1=(f32(b.ln_1.weight), f32(b.ln_1.bias)), qkv=(f16(b.attn.in_proj_weight), f32(b.attn.in_proj_bias)),
                                out=(f16(b.attn.out_proj.weight), f32(b.attn.out_proj.bias)), ln2=(f32(b.ln_2.weight), f32(b.ln_2.bias)),
                                fc=(f16(b.mlp.c_fc.weight), f32(b.mlp.c_fc.bias)), proj=(f16(b.mlp.c_proj.weight), f32(b.mlp.c_proj.bias)))
                           for b in transformer.resblocks]
        self.key = _key(model, tower, device)
        self._grad = None

    def grad_weights(self):
        """The matrices of the image tower transposed to [in][out] float16, which makes dX = dY . W the K-contiguous GEMM: built on
        the first recording call, kept with (and dropped with) this copy.  Never built during a graph capture."""
        if self._grad is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('clip encoder: the transposed weights of the backward are not prepared; run one eager forward with gradients first')
            t = lambda w: w.t().contiguous()                    # noqa: E731
            self._grad = dict(conv=t(self.conv), proj=t(self.proj),
                              blocks=[{k: t(blk[k][0]) for k in ('qkv', 'out', 'fc', 'proj')} for blk in self.blocks])
        return self._grad


def prepared(model, tower, device):
    """The prepared weights of `tower` ('visual' or 'text') of `model`, cached on the module."""
    name = '_sg3_prepared_' + tower
    cache = model.__dict__.get(name)
    key = _key(model, tower, device)
    if cache is not None and cache.key == key:
        return cache
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('clip encoder: the prepared weights are stale during a graph capture; run one eager forward first')
    cache = PreparedTower(model, tower, device)
    model.__dict__[name] = cache
    return cache


# ---- towers -----------------------------------------------------------------------------------------------------------------

def _blocks(x, prep, B, L, D, heads, causal):
    """The residual blocks in place on the float32 stream x [B, L, D]: seven launches each."""
    M, dev = B * L, x.device
    h = torch.empty([M, D], dtype=torch.float16, device=dev)
    qkv = torch.empty([M, 3 * D], dtype=torch.float16, device=dev)
    att = torch.empty([M, D], dtype=torch.float16, device=dev)
    mlp = torch.empty([M, 4 * D], dtype=torch.float16, device=dev)
    for blk in prep.blocks:
        layernorm(x, *blk['ln1'], h, M, D)
        gemm(h, *blk['qkv'], qkv, abi.SG3_CLIP_EPI_F16, M)
        attention(qkv, att, B, L, heads, causal)
        gemm(att, *blk['out'], x, abi.SG3_CLIP_EPI_RESIDUAL, M)
        layernorm(x, *blk['ln2'], h, M, D)
        gemm(h, *blk['fc'], mlp, abi.SG3_CLIP_EPI_QUICKGELU_F16, M)
        gemm(mlp, *blk['proj'], x, abi.SG3_CLIP_EPI_RESIDUAL, M)
    return x


def launches(layers, tower='visual'):
    """Kernel launches of one tower forward: stem (two for the image, one for text), seven per block, LayerNorm and projection."""
    return 7 * int(layers) + (4 if tower == 'visual' else 3)


def launches_backward(layers):
    """Kernel launches of the image tower's backward: scale, head GEMM and ln_post, seven per block, ln_pre and the patch adjoint."""
    return 7 * int(layers) + 5


def image_supported(model):
    v = model.visual
    L = (v.input_resolution // v.patch_size) ** 2 + 1
    return supported(v.width, v.heads, L) and v.patch_size % 8 == 0 and v.input_resolution % 4 == 0 and v.output_dim % 64 == 0


def text_supported(model):
    return supported(model.transformer.width, model.transformer.heads, model.context_length) and int(model.text_projection.shape[1]) % 64 == 0


def encode_image(model, image):
    """image CUDA float32 [B, 3, R, R] -> float32 [B, E]."""
    v = model.visual
    image = _need(image.contiguous(), torch.float32, 'image')
    B, R, P, D = int(image.shape[0]), v.input_resolution, v.patch_size, v.width
    if image.ndim != 4 or tuple(image.shape[1:]) != (3, R, R) or B == 0:
        raise RuntimeError(f'clip encode_image: image must be [n, 3, {R}, {R}] with n > 0, got {list(image.shape)}')
    if torch.is_grad_enabled() and image.requires_grad:
        return _EncodeImage.apply(image, model)
    prep = prepared(model, 'visual', image.device)
    g = R // P
    L = g * g + 1
    x = torch.empty([B, L, D], dtype=torch.float32, device=image.device)
    gemm(image, prep.conv, None, x, abi.SG3_CLIP_EPI_PATCH, B * g * g, pos=prep.pos, cls=prep.cls, patch=P, resolution=R)
    layernorm(x, *prep.ln_pre, x, B * L, D)
    _blocks(x, prep, B, L, D, v.heads, False)
    h = torch.empty([B, D], dtype=torch.float16, device=image.device)
    layernorm(x, *prep.ln_out, h, B, D, row_stride=L * D)
    return gemm(h, prep.proj, None, torch.empty([B, v.output_dim], dtype=torch.float32, device=image.device), abi.SG3_CLIP_EPI_F32, B)


def _encode_image_recording(model, image):
    """The forward of `encode_image` with the same launches and arithmetic, keeping what the backward reads."""
    v = model.visual
    B, R, P, D, heads, dev = int(image.shape[0]), v.input_resolution, v.patch_size, v.width, v.heads, image.device
    prep = prepared(model, 'visual', dev)
    prep.grad_weights()
    g = R // P
    L = g * g + 1
    M = B * L
    f16 = lambda *shape: torch.empty(shape, dtype=torch.float16, device=dev)          # noqa: E731
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
    x0 = f32(B, L, D)
    gemm(image, prep.conv, None, x0, abi.SG3_CLIP_EPI_PATCH, B * g * g, pos=prep.pos, cls=prep.cls, patch=P, resolution=R)
    x = layernorm(x0, *prep.ln_pre, f32(B, L, D), M, D)
    h, att, mlp = f16(M, D), f16(M, D), f16(M, 4 * D)
    saved = []
    for blk in prep.blocks:
        qkv, u, x_mid, x_out = f16(M, 3 * D), f16(M, 4 * D), f32(B, L, D), f32(B, L, D)
        layernorm(x, *blk['ln1'], h, M, D)
        gemm(h, *blk['qkv'], qkv, abi.SG3_CLIP_EPI_F16, M)
        attention(qkv, att, B, L, heads, False)
        gemm(att, *blk['out'], x_mid, abi.SG3_CLIP_EPI_RESIDUAL, M, aux=x)
        layernorm(x_mid, *blk['ln2'], h, M, D)
        gemm(h, *blk['fc'], mlp, abi.SG3_CLIP_EPI_QUICKGELU_SAVE_F16, M, aux=u)
        gemm(mlp, *blk['proj'], x_out, abi.SG3_CLIP_EPI_RESIDUAL, M, aux=x_mid)
        saved.append((x, qkv, x_mid, u))
        x = x_out
    hb = f16(B, D)
    layernorm(x, *prep.ln_out, hb, B, D, row_stride=L * D)
    feats = gemm(hb, prep.proj, None, f32(B, v.output_dim), abi.SG3_CLIP_EPI_F32, B)
    return feats, prep, x0, saved, x


def _encode_image_backward(prep, geom, x0, saved, x_last, dfeat):
    """d image of sum(features * dfeat): `launches_backward` launches.  The gradient stream `gs` [B, L, D] is float32 and carries
    the per-sample power of two of `grad_scale`, which the patch adjoint divides out."""
    B, L, D, heads, P, R = geom
    M, dev, gw = B * L, dfeat.device, prep.grad_weights()
    f16 = lambda *shape: torch.empty(shape, dtype=torch.float16, device=dev)          # noqa: E731
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
    g16, inv = grad_scale(dfeat) if GRAD_SCALE else (dfeat.half(), None)
    dh = gemm(g16, gw['proj'], None, f32(B, D), abi.SG3_CLIP_EPI_F32, B)
    gs = torch.zeros([B, L, D], dtype=torch.float32, device=dev)
    layernorm_bwd(dh, x_last, prep.ln_out[0], gs, B, D, x_stride=L * D, dx_stride=L * D)
    du, dn, datt, dqkv = f16(M, 4 * D), f32(M, D), f16(M, D), f16(M, 3 * D)
    for blk, wt, (x_in, qkv, x_mid, u) in zip(reversed(prep.blocks), reversed(gw['blocks']), reversed(saved)):
        gemm(gs, wt['proj'], None, du, abi.SG3_CLIP_EPI_DQUICKGELU_F16, M, aux=u)
        gemm(du, wt['fc'], None, dn, abi.SG3_CLIP_EPI_F32, M)
        layernorm_bwd(dn, x_mid, blk['ln2'][0], gs, M, D, accumulate=True)
        gemm(gs, wt['out'], None, datt, abi.SG3_CLIP_EPI_F16, M)
        attention_bwd(qkv, datt, dqkv, B, L, heads)
        gemm(dqkv, wt['qkv'], None, dn, abi.SG3_CLIP_EPI_F32, M)
        layernorm_bwd(dn, x_in, blk['ln1'][0], gs, M, D, accumulate=True)
    layernorm_bwd(gs, x0, prep.ln_pre[0], gs, M, D)
    g = R // P
    dimage = (torch.zeros if R % P else torch.empty)([B, 3, R, R], dtype=torch.float32, device=dev)      # pixels past the patch grid feed nothing
    return gemm(gs, gw['conv'], None, dimage, abi.SG3_CLIP_EPI_PATCH_ADJOINT, B * g * g, patch=P, resolution=R, scale=inv)


class _EncodeImage(torch.autograd.Function):
    """encode_image with the gradient with respect to the image (weights frozen)."""

    @staticmethod
    def forward(ctx, image, model):
        v = model.visual
        feats, prep, x0, saved, x_last = _encode_image_recording(model, image)
        ctx.prep, ctx.x0, ctx.saved, ctx.x_last = prep, x0, saved, x_last
        ctx.geom = (int(image.shape[0]), int(x0.shape[1]), v.width, v.heads, v.patch_size, v.input_resolution)
        return feats

    @staticmethod
    @once_differentiable                # double backward raises ("differentiate twice"): impl='torch' is the differentiable composite
    def backward(ctx, dfeat):
        return _encode_image_backward(ctx.prep, ctx.geom, ctx.x0, ctx.saved, ctx.x_last, dfeat.float().contiguous()), None


def encode_text(model, tokens):
    """tokens CUDA integer [B, context] -> float32 [B, E]."""
    tokens = _need(tokens.long().contiguous(), torch.int64, 'tokens')
    L, D = model.context_length, model.transformer.width
    if tokens.ndim != 2 or int(tokens.shape[1]) != L or int(tokens.shape[0]) == 0:
        raise RuntimeError(f'clip encode_text: tokens must be [n, {L}] with n > 0, got {list(tokens.shape)}')
    B = int(tokens.shape[0])
    prep = prepared(model, 'text', tokens.device)
    x = torch.empty([B, L, D], dtype=torch.float32, device=tokens.device)
    embed(tokens, prep.table, prep.pos, x)
    _blocks(x, prep, B, L, D, model.transformer.heads, True)
    eot = x[torch.arange(B, device=x.device), tokens.argmax(dim=-1)].contiguous()     # the one gather: LayerNorm is per row, so it runs on these rows only
    h = torch.empty([B, D], dtype=torch.float16, device=x.device)
    layernorm(eot, *prep.ln_out, h, B, D)
    E = int(model.text_projection.shape[1])
    return gemm(h, prep.proj, None, torch.empty([B, E], dtype=torch.float32, device=x.device), abi.SG3_CLIP_EPI_F32, B)
