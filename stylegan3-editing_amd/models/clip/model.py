"""CLIP with a ViT image tower (reference models/styleganxl/feature_networks/clip/model.py:153-236, :239-352, :392-432).

The constructor arguments, attribute names and state-dict keys are the reference's, so OpenAI's ViT state dicts load with
strict=True.  ResNet image towers are not supported.  Tokenising strings is not part of this module: `encode_text` takes token
ids [n, context_length].

Two implementations sit behind `impl`:
  'torch'  the composite below.  It runs on CPU and GPU, in float32, float64 or with float16 weights (`convert_weights`: the
           matrices and their biases in float16, LayerNorm parameters float32 and LayerNorm computed in float32, as the
           reference converts a model), and records gradients.  It is the definition.
  'hip'    torch_utils/ops/clip_transformer.py: fused HIP kernels, float16 GEMM operands with float32 accumulation, float32
           residual stream, float32 features.  CUDA input; gradients off, or, for encode_image with impl='hip' given by name,
           an image that requires a gradient while no parameter of the image tower does (the backward is HIP as well and gives
           the gradient of the image only; it cannot be differentiated again).
impl=None (default) takes 'hip' when the input is a CUDA tensor, gradients are off (torch.no_grad(), or no parameter and no input
requires one) and the kernels support the tower's shape (`sg3_clip_supported`), else 'torch'.  A shape the kernels refuse is not
an error; impl='hip' given explicitly for one is.
"""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn


class LayerNorm(nn.LayerNorm):
    """LayerNorm computed in at least float32 whatever the stream's dtype."""

    def forward(self, x):
        if x.dtype in (torch.float16, torch.bfloat16):
            return super().forward(x.float()).to(x.dtype)
        return super().forward(x)


class QuickGELU(nn.Module):
    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class ResidualAttentionBlock(nn.Module):
    def __init__(self, d_model, n_head, causal=False):
        super().__init__()
        self.attn = nn.MultiheadAttention(d_model, n_head)       # holds in_proj_weight / in_proj_bias / out_proj; forward is written out below
        self.ln_1 = LayerNorm(d_model)
        self.mlp = nn.Sequential(OrderedDict([('c_fc', nn.Linear(d_model, d_model * 4)), ('gelu', QuickGELU()),
                                              ('c_proj', nn.Linear(d_model * 4, d_model))]))
        self.ln_2 = LayerNorm(d_model)
        self.n_head = n_head
        self.causal = causal

    def attention(self, x):
        """x [n, L, D] -> [n, L, D]: softmax(q k^T / sqrt(64) + mask) v per head, then the output projection."""
        n, L, D = x.shape
        q, k, v = F.linear(x, self.attn.in_proj_weight, self.attn.in_proj_bias).view(n, L, 3, self.n_head, D // self.n_head).permute(2, 0, 3, 1, 4)
        scores = (q * (1.0 / math.sqrt(D // self.n_head))) @ k.transpose(-1, -2)
        if self.causal:
            scores = scores + torch.full([L, L], float('-inf'), dtype=x.dtype, device=x.device).triu_(1)
        out = torch.softmax(scores, dim=-1) @ v
        return F.linear(out.permute(0, 2, 1, 3).reshape(n, L, D), self.attn.out_proj.weight, self.attn.out_proj.bias)

    def forward(self, x):
        x = x + self.attention(self.ln_1(x))
        return x + self.mlp(self.ln_2(x))


class Transformer(nn.Module):
    def __init__(self, width, layers, heads, causal=False):
        super().__init__()
        self.width, self.layers, self.heads = width, layers, heads
        self.resblocks = nn.Sequential(*[ResidualAttentionBlock(width, heads, causal) for _ in range(layers)])

    def forward(self, x):
        """x [n, L, width], batch first."""
        return self.resblocks(x)


class VisualTransformer(nn.Module):
    def __init__(self, input_resolution, patch_size, width, layers, heads, output_dim):
        super().__init__()
        self.input_resolution, self.patch_size, self.width, self.heads, self.output_dim = input_resolution, patch_size, width, heads, output_dim
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = LayerNorm(width)
        self.transformer = Transformer(width, layers, heads)
        self.ln_post = LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))

    def forward(self, x):
        x = self.conv1(x).flatten(2).transpose(1, 2)                                    # [n, grid^2, width]
        cls = self.class_embedding.to(x.dtype).expand(x.shape[0], 1, -1)
        x = torch.cat([cls, x], dim=1) + self.positional_embedding.to(x.dtype)
        x = self.transformer(self.ln_pre(x))
        return self.ln_post(x[:, 0, :]) @ self.proj


class CLIP(nn.Module):
    def __init__(self, embed_dim, image_resolution, vision_layers, vision_width, vision_patch_size, context_length, vocab_size,
                 transformer_width, transformer_heads, transformer_layers, impl=None):
        super().__init__()
        if isinstance(vision_layers, (tuple, list)):
            raise NotImplementedError('CLIP: ResNet image towers are not supported, only the ViT models (a state dict with visual.proj)')
        if impl not in (None, 'hip', 'torch'):
            raise ValueError(f"CLIP: impl must be None, 'hip' or 'torch', got {impl!r}")
        self.impl = impl
        self.context_length = context_length
        self.visual = VisualTransformer(image_resolution, vision_patch_size, vision_width, vision_layers, vision_width // 64, embed_dim)
        self.transformer = Transformer(transformer_width, transformer_layers, transformer_heads, causal=True)
        self.vocab_size = vocab_size
        self.token_embedding = nn.Embedding(vocab_size, transformer_width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, transformer_width))
        self.ln_final = LayerNorm(transformer_width)
        self.text_projection = nn.Parameter(torch.empty(transformer_width, embed_dim))
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self.initialize_parameters()

    def initialize_parameters(self):
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        for tr in (self.transformer, self.visual.transformer):
            proj_std, attn_std, fc_std = (tr.width ** -0.5) * ((2 * tr.layers) ** -0.5), tr.width ** -0.5, (2 * tr.width) ** -0.5
            for block in tr.resblocks:
                nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
                nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
                nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
                nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=self.transformer.width ** -0.5)

    @property
    def dtype(self):
        return self.visual.conv1.weight.dtype

    def _pick(self, impl, x, tower):
        from torch_utils.ops import clip_transformer as ct
        impl = self.impl if impl is None else impl
        if impl == 'torch':
            return 'torch'
        if impl not in (None, 'hip'):
            raise ValueError(f"CLIP: impl must be None, 'hip' or 'torch', got {impl!r}")
        grads = torch.is_grad_enabled() and (x.requires_grad or any(q.requires_grad for q in self.parameters()))
        ok = x.is_cuda and not grads and (ct.image_supported(self) if tower == 'visual' else ct.text_supported(self))
        if impl == 'hip' and grads and tower == 'visual' and x.is_cuda and x.requires_grad and ct.image_supported(self) \
                and not any(q.requires_grad for q in self.visual.parameters()):
            return 'hip'                                         # asked for by name: the kernels' backward, gradient of the image only
        if impl == 'hip' and not ok:
            raise RuntimeError(f"CLIP: impl='hip' needs a CUDA input, gradients off and a tower shape the kernels support "
                               f"(input on {x.device}, gradients {'on' if grads else 'off'})")
        return 'hip' if ok else 'torch'

    def encode_image(self, image, impl=None):
        """image [n, 3, R, R] -> features [n, embed_dim] (float32 from 'hip', the model's dtype from 'torch')."""
        if self._pick(impl, image, 'visual') == 'hip':
            from torch_utils.ops import clip_transformer as ct
            return ct.encode_image(self, image.float())
        return self.visual(image.to(self.dtype))

    def encode_text(self, text, impl=None):
        """text: token ids [n, context_length]; the feature is read at the position of the largest id (the end-of-text token)."""
        if self._pick(impl, text, 'text') == 'hip':
            from torch_utils.ops import clip_transformer as ct
            return ct.encode_text(self, text)
        x = self.token_embedding(text).to(self.dtype) + self.positional_embedding.to(self.dtype)
        x = self.ln_final(self.transformer(x)).to(self.dtype)
        return x[torch.arange(x.shape[0], device=x.device), text.argmax(dim=-1)] @ self.text_projection

    def forward(self, image, text):
        image_features, text_features = self.encode_image(image), self.encode_text(text)
        image_features = image_features / image_features.norm(dim=-1, keepdim=True)
        text_features = text_features / text_features.norm(dim=-1, keepdim=True)
        logits_per_image = self.logit_scale.exp().to(image_features.dtype) * image_features @ text_features.to(image_features.dtype).t()
        return logits_per_image, logits_per_image.t()


def convert_weights(model):
    """Float16 weights as the reference converts a model: convolution, linear and attention matrices with their biases and the two
    output projections; LayerNorm parameters, embeddings and logit_scale keep their dtype."""
    for m in model.modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            m.weight.data = m.weight.data.half()
            if m.bias is not None:
                m.bias.data = m.bias.data.half()
        elif isinstance(m, nn.MultiheadAttention):
            m.in_proj_weight.data = m.in_proj_weight.data.half()
            m.in_proj_bias.data = m.in_proj_bias.data.half()
    model.visual.proj.data = model.visual.proj.data.half()
    model.text_projection.data = model.text_projection.data.half()
    return model


def build_model(state_dict, impl=None):
    """A CLIP whose every size is read off the tensors of `state_dict`, with the weights loaded (strict) and in eval mode."""
    if 'visual.proj' not in state_dict:
        raise NotImplementedError('CLIP: this state dict has no visual.proj: ResNet image towers are not supported, only the ViT models')
    state_dict = {k: v for k, v in state_dict.items() if k not in ('input_resolution', 'context_length', 'vocab_size')}
    width, _, patch, _ = state_dict['visual.conv1.weight'].shape
    grid = round((state_dict['visual.positional_embedding'].shape[0] - 1) ** 0.5)
    text_width = state_dict['ln_final.weight'].shape[0]
    model = CLIP(embed_dim=state_dict['text_projection'].shape[1], image_resolution=patch * grid,
                 vision_layers=sum(k.startswith('visual.') and k.endswith('.attn.in_proj_weight') for k in state_dict), vision_width=width,
                 vision_patch_size=patch, context_length=state_dict['positional_embedding'].shape[0],
                 vocab_size=state_dict['token_embedding.weight'].shape[0], transformer_width=text_width, transformer_heads=text_width // 64,
                 transformer_layers=len({k.split('.')[2] for k in state_dict if k.startswith('transformer.resblocks.')}), impl=impl)
    model.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in state_dict.items()}, strict=True)
    return model.eval()


def load(path, device='cpu', impl=None):
    """The model of a state-dict file (torch.save of the state dict, or of a dict holding it under 'state_dict'); OpenAI's
    TorchScript archives are tried through torch.jit.load.  Returns the model on `device`, float32, eval mode, requires_grad off."""
    try:
        obj = torch.load(str(path), map_location='cpu', weights_only=True)
    except Exception as first:
        try:
            obj = torch.jit.load(str(path), map_location='cpu').state_dict()
        except Exception:
            raise RuntimeError(f'models.clip.load: {path} is neither a state-dict file nor a TorchScript archive ({first})') from first
    if isinstance(obj, dict) and 'state_dict' in obj and 'visual.proj' not in obj:
        obj = obj['state_dict']
    return build_model(obj, impl=impl).requires_grad_(False).to(device)
