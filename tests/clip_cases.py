"""Cases shared by the CLIP encoder tests and tests/golden/make_golden_clip.py: configurations, seeded weights (one RandomState
per tensor; biases ~ N(0, 0.1), LayerNorm gains ~ N(1, 0.2), block matrices at init-like scale times `w_scale`, so every term of
the network shows in the result), seeded inputs, and an fp64 restatement of both encoders in torch (runs on any device; reference
models/styleganxl/feature_networks/clip/model.py:153-236, :324-352)."""
import zlib

import numpy as np

_TEXT_SMALL = dict(context_length=77, vocab_size=64, transformer_width=128, transformer_heads=2, transformer_layers=2)
_TEXT_B32 = dict(context_length=77, vocab_size=64, transformer_width=512, transformer_heads=8)
CONFIGS = {
    'small': dict(embed_dim=64, image_resolution=224, vision_layers=2, vision_width=128, vision_patch_size=32, **_TEXT_SMALL),
    'tiny96': dict(embed_dim=64, image_resolution=96, vision_layers=2, vision_width=128, vision_patch_size=32, **_TEXT_SMALL),
    'b32x2': dict(embed_dim=512, image_resolution=224, vision_layers=2, vision_width=768, vision_patch_size=32, transformer_layers=2, **_TEXT_B32),
    'b32': dict(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32, transformer_layers=12, **_TEXT_B32),
    # ViT-B/16's 197 tokens on a 2-layer model: a shape the kernels refuse
    'b16x2': dict(embed_dim=64, image_resolution=224, vision_layers=2, vision_width=128, vision_patch_size=16, **_TEXT_SMALL),
}
GOLDEN_CONFIGS = ('small', 'tiny96', 'b32x2')
GOLDEN_BATCH = 2


def _rs(key, seed):
    return np.random.RandomState((zlib.crc32(key.encode()) + 7919 * int(seed)) % (2 ** 32))


def shapes(cfg):
    """{state-dict key: shape} of configuration `cfg`."""
    c = CONFIGS[cfg]
    w, p, e, tw = c['vision_width'], c['vision_patch_size'], c['embed_dim'], c['transformer_width']
    out = {'positional_embedding': (c['context_length'], tw), 'text_projection': (tw, e), 'logit_scale': (),
           'visual.class_embedding': (w,), 'visual.positional_embedding': ((c['image_resolution'] // p) ** 2 + 1, w), 'visual.proj': (w, e),
           'visual.conv1.weight': (w, 3, p, p), 'visual.ln_pre.weight': (w,), 'visual.ln_pre.bias': (w,)}

    def blocks(prefix, d, layers):
        for i in range(layers):
            b = f'{prefix}resblocks.{i}.'
            out.update({b + 'attn.in_proj_weight': (3 * d, d), b + 'attn.in_proj_bias': (3 * d,), b + 'attn.out_proj.weight': (d, d),
                        b + 'attn.out_proj.bias': (d,), b + 'ln_1.weight': (d,), b + 'ln_1.bias': (d,), b + 'mlp.c_fc.weight': (4 * d, d),
                        b + 'mlp.c_fc.bias': (4 * d,), b + 'mlp.c_proj.weight': (d, 4 * d), b + 'mlp.c_proj.bias': (d,),
                        b + 'ln_2.weight': (d,), b + 'ln_2.bias': (d,)})

    blocks('visual.transformer.', w, c['vision_layers'])
    out.update({'visual.ln_post.weight': (w,), 'visual.ln_post.bias': (w,)})
    blocks('transformer.', tw, c['transformer_layers'])
    out.update({'token_embedding.weight': (c['vocab_size'], tw), 'ln_final.weight': (tw,), 'ln_final.bias': (tw,)})
    return out


def state_dict(cfg, seed=0, w_scale=1.0):
    """Seeded float32 numpy state dict of configuration `cfg`."""
    sd = {}
    for k, shp in shapes(cfg).items():
        r = _rs(k, seed).randn(*shp) if shp else None
        if k == 'logit_scale':
            v = np.log(1 / 0.07)
        elif k.endswith('.bias') or k.endswith('in_proj_bias'):
            v = 0.1 * r
        elif '.ln_' in k or k.startswith('ln_final'):
            v = 1 + 0.2 * r                                         # LayerNorm gains (their biases matched above)
        elif k == 'visual.conv1.weight':
            v = r / np.sqrt(np.prod(shp[1:]))
        elif k.endswith('embedding') or k == 'token_embedding.weight':
            v = 0.5 * r
        elif k in ('visual.proj', 'text_projection'):
            v = r / np.sqrt(shp[0])
        else:                                                       # the four matrices of a block, [out][in]
            v = w_scale * r / np.sqrt(shp[1])
        sd[k] = np.asarray(v, dtype=np.float32)
    return sd


def images(cfg, n, seed=1):
    r = CONFIGS[cfg]['image_resolution']
    return _rs(f'images{r}', seed).randn(n, 3, r, r).astype(np.float32)


def tokens(cfg, n, seed=1):
    """int64 [n, context]: a start id, random ids, the end-of-text id (the largest of the vocabulary) at a seeded position, zeros after."""
    c = CONFIGS[cfg]
    r = _rs('tokens', seed)
    t = r.randint(1, c['vocab_size'] - 1, size=(n, c['context_length'])).astype(np.int64)
    eot = r.randint(1, c['context_length'], size=n)
    eot[0] = c['context_length'] - 1                                 # one row that uses the whole context
    for i in range(n):
        t[i, eot[i]] = c['vocab_size'] - 1
        t[i, eot[i] + 1:] = 0
    return t


def build(cfg, sd=None, device='cpu', half=False, impl=None, **kw):
    """The package's CLIP for `cfg` with the seeded weights, eval mode, requires_grad off."""
    import torch
    from models.clip import build_model, convert_weights
    sd = state_dict(cfg, **kw) if sd is None else sd
    m = build_model({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, impl=impl).requires_grad_(False)
    return (convert_weights(m) if half else m).to(device)


# ---- fp64 restatement ---------------------------------------------------------------------------------------------------------

def _t64(v, device):
    import torch
    if isinstance(v, torch.Tensor):
        return v.to(device).double()
    return torch.as_tensor(np.asarray(v), device=device).double()


def _ln64(x, w, b):
    m = x.mean(-1, keepdim=True)
    d = x - m
    return d / (d.pow(2).mean(-1, keepdim=True) + 1e-5).sqrt() * w + b


def _blocks64(sd, prefix, x, heads, layers, causal, dev):
    import torch
    n, L, D = x.shape
    for i in range(layers):
        g = lambda k: _t64(sd[f'{prefix}resblocks.{i}.{k}'], dev)        # noqa: E731
        q, k, v = (_ln64(x, g('ln_1.weight'), g('ln_1.bias')) @ g('attn.in_proj_weight').T + g('attn.in_proj_bias')).view(n, L, 3, heads, 64).unbind(2)
        s = torch.einsum('nihd,njhd->nhij', q, k) / 8.0
        if causal:
            s = s.masked_fill(torch.ones(L, L, dtype=torch.bool, device=dev).triu(1), float('-inf'))
        o = torch.einsum('nhij,njhd->nihd', torch.softmax(s, dim=-1), v).reshape(n, L, D)
        x = x + o @ g('attn.out_proj.weight').T + g('attn.out_proj.bias')
        u = _ln64(x, g('ln_2.weight'), g('ln_2.bias')) @ g('mlp.c_fc.weight').T + g('mlp.c_fc.bias')
        x = x + (u * torch.sigmoid(1.702 * u)) @ g('mlp.c_proj.weight').T + g('mlp.c_proj.bias')
    return x


def encode_image64(sd, cfg, image, device='cpu'):
    """float64 torch tensor [n, embed_dim]."""
    import torch
    c = CONFIGS[cfg]
    p, w = c['vision_patch_size'], c['vision_width']
    g = c['image_resolution'] // p
    x = _t64(image, device)
    n = x.shape[0]
    patches = x.view(n, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(n, g * g, 3 * p * p)
    x = patches @ _t64(sd['visual.conv1.weight'], device).view(w, -1).T
    x = torch.cat([_t64(sd['visual.class_embedding'], device).expand(n, 1, w), x], dim=1) + _t64(sd['visual.positional_embedding'], device)
    x = _ln64(x, _t64(sd['visual.ln_pre.weight'], device), _t64(sd['visual.ln_pre.bias'], device))
    x = _blocks64(sd, 'visual.transformer.', x, w // 64, c['vision_layers'], False, device)
    return _ln64(x[:, 0], _t64(sd['visual.ln_post.weight'], device), _t64(sd['visual.ln_post.bias'], device)) @ _t64(sd['visual.proj'], device)


def encode_text64(sd, cfg, toks, device='cpu'):
    import torch
    c = CONFIGS[cfg]
    t = (toks if isinstance(toks, torch.Tensor) else torch.as_tensor(np.asarray(toks))).to(device).long()
    x = _t64(sd['token_embedding.weight'], device)[t] + _t64(sd['positional_embedding'], device)
    x = _blocks64(sd, 'transformer.', x, c['transformer_heads'], c['transformer_layers'], True, device)
    x = _ln64(x, _t64(sd['ln_final.weight'], device), _t64(sd['ln_final.bias'], device))
    return x[torch.arange(x.shape[0], device=device), t.argmax(dim=-1)] @ _t64(sd['text_projection'], device)
