"""The CLIP loss without a GPU: the package's CLIPLoss in float64 against the reference's own results (tests/golden/clip_loss.npz,
made by tests/golden/make_golden_clip_loss.py), the composite definition of nearest_up_avg_pool against the two torch modules it
fuses, the float64 gradient yardstick of the GPU tests, and the C ABI of the backward kernels (struct layout and host-side
argument checks, no launch)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import clip_cases as cases
import clip_loss_cases as lcases
from helpers import HERE, golden

ROOT = os.path.dirname(HERE)
RESAMPLE_SHAPES = [(7, 1, 32, 32), (7, 2, 64, 64), (7, 3, 96, 96), (7, 8, 256, 256), (3, 2, 5, 9), (2, 5, 7, 6)]


@pytest.mark.parametrize('w_scale', lcases.W_SCALES)
def test_clip_loss_float64_matches_reference(w_scale):
    """Loss and d mean(loss) / d image equal the reference's float64 run to 1e-10 relative (of the largest entry)."""
    from criteria.clip_loss import CLIPLoss
    g = golden('clip_loss')
    m = cases.build(lcases.CFG, w_scale=w_scale).double()
    text = torch.from_numpy(lcases.tokens())
    for size, n in lcases.GOLDEN_IMAGES.items():
        loss_fn = CLIPLoss(lcases.opts(size), model=m)
        image = torch.from_numpy(lcases.images(size, n)).double().requires_grad_(True)
        loss = loss_fn(image, text)
        assert loss.dtype == torch.float64 and tuple(loss.shape) == (n, lcases.N_TEXT)
        loss.mean().backward()
        ref_loss, ref_grad = g[f'w{w_scale}/loss{size}'], g[f'w{w_scale}/grad{size}']
        assert np.abs(loss.detach().numpy() - ref_loss).max() <= 1e-10 * np.abs(ref_loss).max()
        assert np.abs(ref_grad).max() > 0
        assert np.abs(image.grad.numpy() - ref_grad).max() <= 1e-10 * np.abs(ref_grad).max()


def test_clip_loss_text_features_are_constants_and_model_comes_from_opts(tmp_path):
    """Text features are computed under no_grad (no gradient reaches the text tower's parameters even when they require one); a model
    is loaded from opts.clip_checkpoint_path when none is given."""
    from criteria.clip_loss import CLIPLoss
    sd = cases.state_dict(lcases.CFG)
    path = tmp_path / 'clip_small.pt'
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, str(path))
    opts = lcases.opts(64)
    opts.clip_checkpoint_path = str(path)
    loss_fn = CLIPLoss(opts)
    loss_fn.model.to('cpu')
    given = CLIPLoss(lcases.opts(64), model=cases.build(lcases.CFG, sd))
    image, text = torch.from_numpy(lcases.images(64, 2)), torch.from_numpy(lcases.tokens())
    with torch.no_grad():
        assert torch.equal(loss_fn(image, text), given(image, text))
    given.model.token_embedding.weight.requires_grad_(True)
    given.model.text_projection.requires_grad_(True)
    given(image.clone().requires_grad_(True), text).mean().backward()
    assert given.model.token_embedding.weight.grad is None and given.model.text_projection.grad is None
    with pytest.raises(ValueError, match='stylegan_size'):
        CLIPLoss(lcases.opts(16), model=given.model)


@pytest.mark.parametrize('up,k,H,W', RESAMPLE_SHAPES)
def test_nearest_up_avg_pool_equals_the_torch_modules(up, k, H, W):
    """On the CPU the op is its definition: equal to AvgPool2d(k)(Upsample(scale_factor=up)(x)) and to its autograd, bit for bit, on
    strided views, in float32 and float64; the output size floors."""
    from torch_utils.ops.clip_resample import nearest_up_avg_pool, out_size
    r = np.random.RandomState(up * 100 + k)
    for dtype in (torch.float32, torch.float64):
        base = torch.from_numpy(r.randn(2, 3, H + 3, 2 * W + 1)).to(dtype)
        ba, bb = base.clone().requires_grad_(True), base.clone().requires_grad_(True)
        view = lambda t: t[:, :, 2:2 + H, 1:1 + 2 * W:2]          # noqa: E731
        assert not view(ba).is_contiguous() and tuple(view(ba).shape) == (2, 3, H, W)
        ya = nearest_up_avg_pool(view(ba), up, k)
        yb = torch.nn.AvgPool2d(kernel_size=k)(torch.nn.Upsample(scale_factor=up)(view(bb)))
        assert tuple(ya.shape) == (2, 3, (up * H) // k, (up * W) // k) == (2, 3, out_size(H, up, k), out_size(W, up, k))
        assert torch.equal(ya, yb)
        dy = torch.from_numpy(r.randn(*ya.shape)).to(dtype)
        ya.backward(dy); yb.backward(dy)
        assert torch.equal(ba.grad, bb.grad) and float(ba.grad.abs().max()) > 0
    if up == 7 and H % 32 == 0:
        assert (up * H) // k == 224                       # the sizes the loss uses all give CLIP's 224


def test_nearest_up_avg_pool_argument_errors():
    from torch_utils.ops.clip_resample import nearest_up_avg_pool
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError, match='positive integers'):
        nearest_up_avg_pool(x, 0, 2)
    with pytest.raises(RuntimeError, match='positive integers'):
        nearest_up_avg_pool(x, 2.5, 2)
    with pytest.raises(RuntimeError, match='smaller than the pooling window'):
        nearest_up_avg_pool(x, 2, 9)
    with pytest.raises(RuntimeError, match=r'\[B,C,H,W\]'):
        nearest_up_avg_pool(x[0], 2, 2)


def test_encode_image64_is_a_gradient_yardstick():
    """tests/clip_cases.encode_image64 is differentiable, and its gradient of the loss equals the reference's (the fixture) when the
    loss is rebuilt on it: the GPU tests use it as the float64 yardstick.  1e-7 relative: two float64 evaluations that order their
    sums differently, through two blocks at w_scale 3; the float16 errors the GPU tests measure against it are 1e-4 and larger."""
    g = golden('clip_loss')
    sd = cases.state_dict(lcases.CFG, w_scale=3)
    text = torch.from_numpy(lcases.tokens())
    image = torch.from_numpy(lcases.images(64, 2)).double().requires_grad_(True)
    x = torch.nn.functional.avg_pool2d(torch.nn.functional.interpolate(image, scale_factor=7, mode='nearest'), 2)
    fi = cases.encode_image64(sd, lcases.CFG, x)
    ft = cases.encode_text64(sd, lcases.CFG, text)
    fi, ft = fi / fi.norm(dim=-1, keepdim=True), ft / ft.norm(dim=-1, keepdim=True)
    loss = 1 - (1 / 0.07) * fi @ ft.t() / 100
    loss.mean().backward()
    assert np.abs(loss.detach().numpy() - g['w3/loss64']).max() <= 1e-7 * np.abs(g['w3/loss64']).max()
    assert np.abs(image.grad.numpy() - g['w3/grad64']).max() <= 1e-7 * np.abs(g['w3/grad64']).max()


def test_impl_hip_wording_is_kept_on_the_cpu():
    """impl='hip' by name on a CPU image that requires a gradient is still refused with the present wording."""
    m = cases.build('tiny96')
    x = torch.from_numpy(cases.images('tiny96', 1)).requires_grad_(True)
    with pytest.raises(RuntimeError, match="impl='hip' needs"):
        m.encode_image(x, impl='hip')
    assert m.encode_image(x).requires_grad                  # the default: the composite


# ---- the C ABI of the backward kernels: layout and host-side checks (no launch, no GPU) ------------------------------------------

def test_backward_struct_layouts_match_header():
    from torch_utils import _sg3abi
    with open(os.path.join(ROOT, 'include', 'sg3_ops.h')) as f:
        src = f.read()
    for cname, cls in (('sg3_clip_gemm_grad_params', _sg3abi.ClipGemmGradParams), ('sg3_clip_layernorm_bwd_params', _sg3abi.ClipLayernormBwdParams),
                       ('sg3_clip_attention_bwd_params', _sg3abi.ClipAttentionBwdParams), ('sg3_clip_grad_scale_params', _sg3abi.ClipGradScaleParams),
                       ('sg3_clip_resample_params', _sg3abi.ClipResampleParams)):
        body = re.search(r'typedef struct ' + cname + r' \{(.*?)\} ' + cname + ';', src, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        names = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                parts = decl.split(',')
                names += [re.sub(r'\[\d+\]|\*', '', nm) for nm in [parts[0].split()[-1]] + [q.strip() for q in parts[1:]]]
        assert names == [n for n, _ in cls._fields_], cname
    for name, value in re.findall(r'#define (SG3_CLIP_EPI_\w+)\s+(\d+)', src):
        assert getattr(_sg3abi, name) == int(value), name


def test_backward_argument_checks_refuse_before_any_launch():
    """Every refusal below is made on the host before a launch (the pointers are placeholders that are never followed)."""
    import torch  # noqa: F401
    from torch_utils import _sg3abi as abi
    lib = abi.load()
    fake = 4096
    a = abi.ClipAttentionBwdParams()
    a.qkv, a.dout, a.dqkv, a.B, a.L, a.heads, a.causal = fake, 2 * fake, 3 * fake, 1, 10, 2, 1
    assert lib.sg3_clip_attention_bwd(ctypes.byref(a), None) == abi.SG3_BAD_ARG and b'causal' in lib.sg3_last_error()
    a.causal, a.L = 0, 129
    assert lib.sg3_clip_attention_bwd(ctypes.byref(a), None) == abi.SG3_BAD_ARG
    ln = abi.ClipLayernormBwdParams()
    ln.dy, ln.x, ln.gamma, ln.dx, ln.rows, ln.D, ln.dyRowStride, ln.xRowStride, ln.dxRowStride = fake, 2 * fake, 3 * fake, 4 * fake, 2, 128, 128, 128, 64
    assert lib.sg3_clip_layernorm_bwd(ctypes.byref(ln), None) == abi.SG3_BAD_ARG and b'row strides' in lib.sg3_last_error()
    g = abi.ClipGemmGradParams()
    g.a, g.w, g.out, g.M, g.K, g.N = fake, 2 * fake, 3 * fake, 4, 64, 64
    for epi, aux, msg in ((abi.SG3_CLIP_EPI_DQUICKGELU_F16, 0, b'needs aux'), (abi.SG3_CLIP_EPI_QUICKGELU_SAVE_F16, 0, b'needs aux'),
                          (abi.SG3_CLIP_EPI_RESIDUAL, 0, b'needs aux'), (abi.SG3_CLIP_EPI_F32, 4 * fake, b'takes no aux'),
                          (abi.SG3_CLIP_EPI_QUICKGELU_SAVE_F16, 3 * fake, b'must not be out'),
                          (abi.SG3_CLIP_EPI_QUICKGELU_F16, 0, b'unknown epilogue'), (abi.SG3_CLIP_EPI_PATCH, 0, b'unknown epilogue'), (8, 0, b'unknown epilogue')):
        g.epilogue, g.aux = epi, aux
        assert lib.sg3_clip_gemm_grad(ctypes.byref(g), None) == abi.SG3_BAD_ARG and msg in lib.sg3_last_error(), (epi, lib.sg3_last_error())
    g.epilogue, g.aux, g.aF32 = abi.SG3_CLIP_EPI_F32, 0, 1
    assert lib.sg3_clip_gemm_grad(ctypes.byref(g), None) == abi.SG3_BAD_ARG and b'float32 operand' in lib.sg3_last_error()
    g.epilogue, g.P, g.R = abi.SG3_CLIP_EPI_PATCH_ADJOINT, 32, 96
    assert lib.sg3_clip_gemm_grad(ctypes.byref(g), None) == abi.SG3_BAD_ARG and b'3 * patch^2' in lib.sg3_last_error()
    g.epilogue, g.aF32, g.K = abi.SG3_CLIP_EPI_F16, 0, 48
    assert lib.sg3_clip_gemm_grad(ctypes.byref(g), None) == abi.SG3_BAD_ARG and b'multiple of 32' in lib.sg3_last_error()
    r = abi.ClipResampleParams()
    r.x, r.y, r.B, r.C, r.H, r.W, r.oh, r.ow, r.up, r.k = fake, 2 * fake, 1, 3, 64, 64, 225, 224, 7, 2
    assert lib.sg3_clip_resample(ctypes.byref(r), None) == abi.SG3_BAD_ARG and b'floor' in lib.sg3_last_error()
    s = abi.ClipGradScaleParams()
    s.g, s.out16, s.inv, s.B, s.E = fake, 2 * fake, 0, 1, 64
    assert lib.sg3_clip_grad_scale(ctypes.byref(s), None) == abi.SG3_BAD_ARG
