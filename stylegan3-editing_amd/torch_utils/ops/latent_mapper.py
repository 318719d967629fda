"""StyleCLIP latent mapper forward on the fused HIP kernel (csrc/sg3_latent_mapper.hip, include/sg3_ops.h sg3_latent_mapper).

`prepared(groups, device)` holds the per-checkpoint weights the kernel reads: every EqualLinear's `weight * scale` (computed in
fp32 on the device as reference editing/styleclip_mapper/latent_mappers.py:119 computes it on every call), in the stored [out][in]
order, and `bias * lr_mul`.  The copy is keyed by the `(data_ptr, _version)` of every parameter it comes from and rebuilt when one
changes (in-place edits bump `_version`); it is never rebuilt while a graph is being captured.  `launch` runs one forward of all
groups: five kernel launches on the current stream.

`train_forward` is the differentiable form (sg3_latent_mapper_train_forward / sg3_latent_mapper_backward): the same forward kernels
with h0..h4 kept, and a backward of at most ten launches that returns dx and the gradients of the STORED weights and biases.  The
prepared copy is rebuilt after every optimizer step (one stack and one multiply per tensor kind).  A backward entered with gradients
enabled (create_graph) differentiates the torch composite instead.
"""
import math

import torch
import torch.nn.functional as F

from torch_utils import _sg3abi

D = 512


def _linears(mapper):
    """The four EqualLinear layers of a Mapper (index 0 of `mapping` is the parameter-free PixelNorm)."""
    return [mapper.mapping[i] for i in range(1, 5)]


def _key(mappers, device):
    return (str(device),) + tuple((p.data_ptr(), p._version) for m in mappers for lin in _linears(m) for p in (lin.weight, lin.bias))


class PreparedMapper:
    """(W * scale) [G,4,512,512] and (b * lr_mul) [G,4,512] of G Mapper modules, on one device."""

    def __init__(self, mappers, device):
        with torch.no_grad():
            self.weight = torch.stack([torch.stack([(lin.weight.to(device) * lin.scale) for lin in _linears(m)]) for m in mappers]).contiguous()
            self.bias = torch.stack([torch.stack([(lin.bias.to(device) * lin.lr_mul) for lin in _linears(m)]) for m in mappers]).contiguous()
        self.key = _key(mappers, device)


def prepared(owner, mappers, device):
    """The prepared weights of `mappers`, cached on `owner` (the SingleMapper / LevelsMapper module)."""
    cache = owner.__dict__.get('_sg3_prepared')
    if not mappers:
        return None
    key = _key(mappers, device)
    if cache is not None and cache.key == key:
        return cache
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError('latent mapper: the prepared weights are stale during a graph capture; run one eager forward first')
    cache = PreparedMapper(mappers, device)
    owner.__dict__['_sg3_prepared'] = cache
    return cache


def launch(x, prep, ranges, alpha=0.1, want_out=True, want_delta=False):
    """x: CUDA float32 [N, L, 512].  ranges: [(level_begin, level_end)] of the enabled groups, in the order of `prep`'s weights.
    Returns (out, delta): out = x + alpha * mapper(x), delta = mapper(x) (None when not asked for)."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == D):
        raise RuntimeError(f'latent mapper kernel: needs a CUDA float32 [N, L, 512] tensor, got {x.dtype} {tuple(x.shape)} on {x.device}')
    if len(ranges) > 4 or (len(ranges) > 0) != (prep is not None):
        raise RuntimeError('latent mapper kernel: groups and prepared weights do not match')
    x = x.contiguous()
    n, L, _ = x.shape
    out = torch.empty_like(x) if want_out else None
    delta = torch.empty_like(x) if want_delta else None
    scratch = torch.empty([2, n, L, D], dtype=torch.float32, device=x.device) if ranges else None
    p = _sg3abi.LatentMapperParams()
    p.x = _sg3abi.ptr(x)
    p.weight = _sg3abi.ptr(prep.weight) if prep is not None else None
    p.bias = _sg3abi.ptr(prep.bias) if prep is not None else None
    p.out = _sg3abi.ptr(out)
    p.delta = _sg3abi.ptr(delta)
    p.scratch = _sg3abi.ptr(scratch)
    p.N, p.L, p.D, p.groups = n, L, D, len(ranges)
    for g, (b, e) in enumerate(ranges):
        p.levelBegin[g], p.levelEnd[g] = b, e
    p.alpha = float(alpha)
    lib = _sg3abi.load()
    with torch.cuda.device(x.device):
        _sg3abi.check(lib.sg3_latent_mapper(p, _sg3abi.stream_ptr(x.device)), 'sg3_latent_mapper')
    return out, delta


def composite(x, weights, biases, ranges, scales, lr_muls, alpha):
    """(out, delta) of the torch composite over explicit parameter lists (4 weights and 4 biases per group, group-major): what
    the modules in editing/styleclip_mapper/latent_mappers.py compute, restated for the double backward."""
    parts = {}
    for g, (b, e) in enumerate(ranges):
        h = x[:, b:e, :]
        h = h * torch.rsqrt(torch.mean(h ** 2, dim=1, keepdim=True) + 1e-8)
        for i in range(4):
            j = 4 * g + i
            h = F.linear(h, weights[j] * scales[j])
            h = F.leaky_relu(h + (biases[j] * lr_muls[j]).view(1, -1), negative_slope=0.2) * math.sqrt(2)
        parts[(b, e)] = h
    delta = torch.cat([parts[r] if r in parts else torch.zeros_like(x[:, r[0]:r[1], :]) for r in _cover(ranges, x.shape[1])], dim=1)
    return x + alpha * delta, delta


def _cover(ranges, L):
    """The level ranges of `ranges` plus the gaps between them, in level order, covering [0, L)."""
    out, at = [], 0
    for b, e in sorted(ranges):
        if b > at:
            out.append((at, b))
        out.append((b, e))
        at = e
    if at < L:
        out.append((at, L))
    return out


def _fill_groups(p, ranges, n, L, alpha):
    p.N, p.L, p.D, p.groups = n, L, D, len(ranges)
    for g, (b, e) in enumerate(ranges):
        p.levelBegin[g], p.levelEnd[g] = b, e
    p.alpha = float(alpha)


class _MapperTrain(torch.autograd.Function):
    """(out, delta) = f(x, *weights, *biases); out is None unless asked for."""

    @staticmethod
    def forward(ctx, meta, x, *params):
        prep, ranges, scales, lr_muls, alpha, want_out = meta
        x = x.contiguous()
        n, L, _ = x.shape
        out = torch.empty_like(x) if want_out else None
        delta = torch.empty_like(x)
        acts = torch.empty([4, n, L, D], dtype=torch.float32, device=x.device) if ranges else None
        p = _sg3abi.LatentMapperTrainParams()
        p.x = _sg3abi.ptr(x)
        p.weight = _sg3abi.ptr(prep.weight) if prep is not None else None
        p.bias = _sg3abi.ptr(prep.bias) if prep is not None else None
        p.out, p.delta, p.acts = _sg3abi.ptr(out), _sg3abi.ptr(delta), _sg3abi.ptr(acts)
        _fill_groups(p, ranges, n, L, alpha)
        with torch.cuda.device(x.device):
            _sg3abi.check(_sg3abi.load().sg3_latent_mapper_train_forward(p, _sg3abi.stream_ptr(x.device)), 'sg3_latent_mapper_train_forward')
        ctx.meta = meta
        ctx.prep_weight = prep.weight if prep is not None else None     # the prepared copy this forward read (kept alive for the backward)
        ctx.acts = acts
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, delta, *params)
        return out, delta

    @staticmethod
    def backward(ctx, d_out, d_delta):
        prep, ranges, scales, lr_muls, alpha, _ = ctx.meta
        x, delta, *params = ctx.saved_tensors
        k = len(params) // 2
        need_x, need_p = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
        none = (None,) * (2 + len(params))
        if d_out is None and d_delta is None:
            return none
        if torch.is_grad_enabled():
            # double backward: differentiate the composite (the kernels have no second derivative)
            with torch.enable_grad():
                o, d = composite(x, params[:k], params[k:], ranges, scales, lr_muls, alpha)
                outs, gouts = [], []
                if d_out is not None:
                    outs.append(o); gouts.append(d_out)
                if d_delta is not None:
                    outs.append(d); gouts.append(d_delta)
                wanted = [t for t, need in zip([x] + list(params), ctx.needs_input_grad[1:]) if need]
                grads = iter(torch.autograd.grad(outs, wanted, gouts, create_graph=True, allow_unused=True))
            return (None,) + tuple(next(grads) if need else None for need in ctx.needs_input_grad[1:])
        n, L, _ = x.shape
        dev = x.device
        d_out = d_out.contiguous() if d_out is not None else None
        d_delta = d_delta.contiguous() if d_delta is not None else None
        if not ranges:
            # no group: delta is constant, out = x
            return (None, d_out if need_x else None) + (None,) * len(params)
        if not (need_x or need_p):
            return none
        G = len(ranges)
        dx = torch.empty_like(x) if need_x else None
        dW = torch.empty([G, 4, D, D], dtype=torch.float32, device=dev) if need_p else None
        dB = torch.empty([G, 4, D], dtype=torch.float32, device=dev) if need_p else None
        scratch = torch.empty([2, n, L, D], dtype=torch.float32, device=dev)
        p = _sg3abi.LatentMapperBackwardParams()
        p.x, p.weight, p.acts, p.delta = _sg3abi.ptr(x), _sg3abi.ptr(ctx.prep_weight), _sg3abi.ptr(ctx.acts), _sg3abi.ptr(delta)
        p.dDelta, p.dOut = _sg3abi.ptr(d_delta), _sg3abi.ptr(d_out)
        p.dx, p.dW, p.dB, p.scratch = _sg3abi.ptr(dx), _sg3abi.ptr(dW), _sg3abi.ptr(dB), _sg3abi.ptr(scratch)
        _fill_groups(p, ranges, n, L, alpha)
        for j in range(4 * G):
            p.wScale[j], p.bScale[j] = scales[j], lr_muls[j]
        with torch.cuda.device(dev):
            _sg3abi.check(_sg3abi.load().sg3_latent_mapper_backward(p, _sg3abi.stream_ptr(dev)), 'sg3_latent_mapper_backward')
        gw = [dW[j // 4, j % 4] if need_p and ctx.needs_input_grad[2 + j] else None for j in range(k)]
        gb = [dB[j // 4, j % 4] if need_p and ctx.needs_input_grad[2 + k + j] else None for j in range(k)]
        return (None, dx) + tuple(gw) + tuple(gb)


def train_forward(x, owner, mappers, ranges, alpha=0.1, want_out=True):
    """Differentiable (out, delta) of the enabled groups `mappers` over level `ranges` on the HIP kernels; out is None unless
    want_out.  Gradients flow to x and to every weight and bias of `mappers`."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[2] == D):
        raise RuntimeError(f'latent mapper kernel: needs a CUDA float32 [N, L, 512] tensor, got {x.dtype} {tuple(x.shape)} on {x.device}')
    if len(ranges) > 4 or len(ranges) != len(mappers):
        raise RuntimeError('latent mapper kernel: groups and mappers do not match')
    prep = prepared(owner, mappers, x.device)
    lins = [lin for m in mappers for lin in _linears(m)]
    meta = (prep, list(ranges), [float(lin.scale) for lin in lins], [float(lin.lr_mul) for lin in lins], float(alpha), bool(want_out))
    return _MapperTrain.apply(meta, x, *[lin.weight for lin in lins], *[lin.bias for lin in lins])
