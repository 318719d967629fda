"""`fma(a, b, c) = a * b + c` with broadcasting (operator API of reference torch_utils/ops/fma.py: `fma` :15).

Imported by name from the module source embedded in upstream training snapshots (the discriminator's modulated
convolution); the generator graph of this package does not use it.  The contract is the value, broadcasting, and
gradients that come back in each operand's own shape, to any order.  `torch.addcmul` is all of that in one fused
elementwise kernel: its autograd formula sums every operand's gradient over the axes that operand was broadcast along
and is itself differentiable, so no autograd node of this package's own is needed.
"""
import torch


def fma(a, b, c):
    return torch.addcmul(c, a, b)
