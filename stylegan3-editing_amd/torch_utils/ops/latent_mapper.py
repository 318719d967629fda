"""StyleCLIP latent mapper forward on the fused HIP kernel (csrc/sg3_latent_mapper.hip, include/sg3_ops.h sg3_latent_mapper).

`prepared(groups, device)` holds the per-checkpoint weights the kernel reads: every EqualLinear's `weight * scale` (computed in
fp32 on the device as reference editing/styleclip_mapper/latent_mappers.py:119 computes it on every call), in the stored [out][in]
order, and `bias * lr_mul`.  The copy is keyed by the `(data_ptr, _version)` of every parameter it comes from and rebuilt when one
changes (in-place edits bump `_version`); it is never rebuilt while a graph is being captured.  `launch` runs one forward of all
groups: five kernel launches on the current stream.
"""
import torch

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
