"""StyleCLIP latent mappers (reference editing/styleclip_mapper/latent_mappers.py).

The torch composite below is the definition: `Mapper` is PixelNorm then four EqualLinear(512, 512, lr_mul=0.01,
activation='fused_lrelu') (reference :9-25); `SingleMapper` runs one Mapper over all levels (:28-38); `LevelsMapper` runs one per
level group -- coarse 0-4 (`course_mapping`, the reference's spelling), medium 5-7, fine 8-15 -- and a disabled group gives zeros
(:41-78).  `PixelNorm` normalises over dim 1, which for the mapper's [N, L, 512] input is the LEVEL axis (:131-137); that is kept.

In eval mode, with no gradient recorded, on a CUDA float32 [N, 16, 512] input and 512 x 512 weights, `SingleMapper.forward` and
`LevelsMapper.forward` run every group in one fused HIP forward (torch_utils/ops/latent_mapper.py, csrc/sg3_latent_mapper.hip);
`edit(w, alpha)` returns `w + alpha * mapper(w)` from the same launches.  In TRAINING mode with gradients enabled, on the same
inputs, both run the differentiable HIP form (`latent_mapper.train_forward`: the same forward kernels with the activations kept,
and a HIP backward to the input and to every weight and bias).  Anywhere else -- eval mode with gradients enabled included, which
the tests use as their fp32 yardstick -- the composite runs.
"""
import torch
from torch import nn
from torch.nn import Module
from torch.nn import functional as F

from models.stylegan2.model import EqualLinear  # noqa: F401  (re-exported: the reference defines it in this module, :108-128)

_COARSE, _MEDIUM, _FINE = (0, 5), (5, 8), (8, 16)


class PixelNorm(nn.Module):
    """x * rsqrt(mean(x^2 over dim 1) + 1e-8) (reference :131-137)."""

    def forward(self, input):  # pylint: disable=redefined-builtin
        return input * torch.rsqrt(torch.mean(input ** 2, dim=1, keepdim=True) + 1e-8)


def fused_leaky_relu(input, bias, negative_slope=0.2, scale=2 ** 0.5):  # pylint: disable=redefined-builtin
    """leaky_relu(input + bias, negative_slope) * scale; the bias runs along the last dim of a 3-D input and along dim 1
    otherwise (reference :92-106, without its `.cuda()` move, so it also runs on the CPU)."""
    rest = [1] * (input.ndim - bias.ndim - 1)
    shape = (1, *rest, bias.shape[0]) if input.ndim == 3 else (1, bias.shape[0], *rest)
    return F.leaky_relu(input + bias.view(*shape), negative_slope=negative_slope) * scale


class FusedLeakyReLU(nn.Module):
    """Module form of `fused_leaky_relu` with a learned bias (reference :80-90)."""

    def __init__(self, channel, negative_slope=0.2, scale=2 ** 0.5):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(channel))
        self.negative_slope = negative_slope
        self.scale = scale

    def forward(self, input):  # pylint: disable=redefined-builtin
        return fused_leaky_relu(input, self.bias, self.negative_slope, self.scale)


class Mapper(Module):
    def __init__(self, opts, latent_dim=512):
        super().__init__()
        self.opts = opts
        self.mapping = nn.Sequential(PixelNorm(), *[EqualLinear(latent_dim, latent_dim, lr_mul=0.01, activation='fused_lrelu')
                                                    for _ in range(4)])

    def forward(self, x):
        return self.mapping(x)


class _FusedMapperMixin:
    """The HIP path shared by SingleMapper and LevelsMapper.  `_groups()` lists ((level_begin, level_end), Mapper or None)."""

    def _fused_ok(self, x):
        if self.training or torch.is_grad_enabled():
            return False
        return self._fused_shapes_ok(x)

    def _fused_train_ok(self, x):
        return self.training and torch.is_grad_enabled() and self._fused_shapes_ok(x)

    def _fused_shapes_ok(self, x):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[1] == 16 and x.shape[2] == 512):
            return False
        for _, m in self._groups():
            if m is None:
                continue
            for lin in m.mapping[1:]:
                if lin.weight.shape != (512, 512) or lin.bias is None or lin.weight.dtype != torch.float32 or lin.weight.device != x.device:
                    return False
        return True

    def _fused(self, x, alpha, want_out, want_delta):
        from torch_utils.ops import latent_mapper
        on = [(r, m) for r, m in self._groups() if m is not None]
        prep = latent_mapper.prepared(self, [m for _, m in on], x.device)
        return latent_mapper.launch(x, prep, [r for r, _ in on], alpha=alpha, want_out=want_out, want_delta=want_delta)

    def _fused_train(self, x, alpha, want_out):
        """(out, delta) with gradients to x and the parameters; out is None unless want_out."""
        from torch_utils.ops import latent_mapper
        on = [(r, m) for r, m in self._groups() if m is not None]
        return latent_mapper.train_forward(x, self, [m for _, m in on], [r for r, _ in on], alpha=alpha, want_out=want_out)

    def edit(self, w, alpha=0.1):
        """w + alpha * self(w) (reference scripts/inference.py:98); on the HIP path straight from the kernel."""
        if self._fused_ok(w):
            return self._fused(w, alpha, True, False)[0]
        if self._fused_train_ok(w):
            return self._fused_train(w, alpha, True)[0]
        return w + alpha * self(w)


class SingleMapper(_FusedMapperMixin, Module):
    def __init__(self, opts):
        super().__init__()
        self.opts = opts
        self.mapping = Mapper(opts)

    def _groups(self):
        return [((0, 16), self.mapping)]

    def forward(self, x):
        if self._fused_ok(x):
            return self._fused(x, 0.1, False, True)[1]
        if self._fused_train_ok(x):
            return self._fused_train(x, 0.1, False)[1]
        return self.mapping(x)


class LevelsMapper(_FusedMapperMixin, Module):
    def __init__(self, opts):
        super().__init__()
        self.opts = opts
        if not opts.no_coarse_mapper:
            self.course_mapping = Mapper(opts)
        if not opts.no_medium_mapper:
            self.medium_mapping = Mapper(opts)
        if not opts.no_fine_mapper:
            self.fine_mapping = Mapper(opts)

    def _groups(self):
        return [(_COARSE, None if self.opts.no_coarse_mapper else self.course_mapping),
                (_MEDIUM, None if self.opts.no_medium_mapper else self.medium_mapping),
                (_FINE, None if self.opts.no_fine_mapper else self.fine_mapping)]

    def forward(self, x):
        if self._fused_ok(x):
            return self._fused(x, 0.1, False, True)[1]
        if self._fused_train_ok(x):
            return self._fused_train(x, 0.1, False)[1]
        parts = []
        for (b, e), m in self._groups():
            xs = x[:, b:e, :] if e < 16 else x[:, b:, :]
            parts.append(torch.zeros_like(xs) if m is None else m(xs))
        return torch.cat(parts, dim=1)
