"""Ranger: RAdam with lookahead and gradient centralisation (reference utils/ranger.py, version 20.4.11), restated.

Constructor arguments, state keys ('step', 'exp_avg', 'exp_avg_sq', 'slow_buffer'), the ten-slot `radam_buffer` of
(step, N_sma, step_size), the `N_sma > N_sma_threshhold` choice between the adaptive and the plain step, centralisation of every
gradient with `grad.dim() > gc_gradient_threshold` (1, or 3 with gc_conv_only) and the lookahead blend every k-th step are the
reference's.  As there, the centralised gradient is left in `p.grad`.  Half and bfloat16 tensors are stepped in float32, as there;
a float64 parameter is stepped in float64 (the reference would round it to float32), so that the class can serve as its own
double-precision yardstick.

When every parameter that has a gradient is a contiguous CUDA float32 tensor of at most two dimensions, a step is one launch of
csrc/sg3_ranger.hip per 32 tensors (sg3_ranger_step): `step_size`, the branch and the lookahead flag are computed here from the
Python step count, so nothing is read back from the device.  Anything else, or everything after `optimizer.fused = False`, takes
the torch path below.
"""
import math

import torch
from torch.optim.optimizer import Optimizer

_FUSED_MAX = 32


def _compute_dtype(p):
    return torch.float64 if p.dtype == torch.float64 else torch.float32


class Ranger(Optimizer):

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999), eps=1e-5, weight_decay=0,
                 use_gc=True, gc_conv_only=False):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f'Invalid slow update rate: {alpha}')
        if not 1 <= k:
            raise ValueError(f'Invalid lookahead steps: {k}')
        if not lr > 0:
            raise ValueError(f'Invalid Learning Rate: {lr}')
        if not eps > 0:
            raise ValueError(f'Invalid eps: {eps}')
        defaults = dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps,
                        weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha = alpha
        self.k = k
        self.radam_buffer = [[None, None, None] for _ in range(10)]
        self.use_gc = use_gc
        self.gc_gradient_threshold = 3 if gc_conv_only else 1
        self.fused = True              # False: always the torch path

    def _init_state(self, p):
        state = self.state[p]
        if len(state) == 0:
            state['step'] = 0
            state['exp_avg'] = torch.zeros_like(p.data, dtype=_compute_dtype(p))
            state['exp_avg_sq'] = torch.zeros_like(p.data, dtype=_compute_dtype(p))
            state['slow_buffer'] = torch.empty_like(p.data)
            state['slow_buffer'].copy_(p.data)
        return state

    def _schedule(self, step, beta1, beta2):
        """(N_sma, step_size) of `step`, through the reference's ten-slot buffer."""
        slot = self.radam_buffer[int(step % 10)]
        if step == slot[0]:
            return slot[1], slot[2]
        slot[0] = step
        beta2_t = beta2 ** step
        n_max = 2 / (1 - beta2) - 1
        n_sma = n_max - 2 * step * beta2_t / (1 - beta2_t)
        slot[1] = n_sma
        if n_sma > self.N_sma_threshhold:
            step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2)) / (1 - beta1 ** step)
        else:
            step_size = 1.0 / (1 - beta1 ** step)
        slot[2] = step_size
        return n_sma, step_size

    def _centralise(self, grad):
        return self.use_gc and grad.dim() > self.gc_gradient_threshold

    @staticmethod
    def _fusable(p):
        return (p.is_cuda and p.dtype == torch.float32 and p.dim() <= 2 and p.numel() > 0 and p.is_contiguous()
                and p.grad.dtype == torch.float32 and p.grad.is_contiguous() and p.grad.device == p.device and not p.grad.is_sparse)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        with_grad = [p for group in self.param_groups for p in group['params'] if p.grad is not None]
        fused = self.fused and bool(with_grad) and all(self._fusable(p) for p in with_grad)
        for group in self.param_groups:
            params = [p for p in group['params'] if p.grad is not None]
            if fused:
                self._step_fused(group, params)
            else:
                for p in params:
                    self._step_torch(group, p)
        return loss

    def _step_torch(self, group, p):
        if p.grad.is_sparse:
            raise RuntimeError('Ranger optimizer does not support sparse gradients')
        grad = p.grad.data.to(_compute_dtype(p))      # the gradient itself when it is float32: centralised in place, as in the reference
        p32 = p.data.to(_compute_dtype(p))
        state = self._init_state(p)
        state['exp_avg'] = state['exp_avg'].type_as(p32)
        state['exp_avg_sq'] = state['exp_avg_sq'].type_as(p32)
        exp_avg, exp_avg_sq = state['exp_avg'], state['exp_avg_sq']
        beta1, beta2 = group['betas']
        if self._centralise(grad):
            grad.add_(-grad.mean(dim=tuple(range(1, grad.dim())), keepdim=True))
        state['step'] += 1
        exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
        n_sma, step_size = self._schedule(state['step'], beta1, beta2)
        if group['weight_decay'] != 0:
            p32.add_(p32, alpha=-group['weight_decay'] * group['lr'])
        if n_sma > self.N_sma_threshhold:
            denom = exp_avg_sq.sqrt().add_(group['eps'])
            p32.addcdiv_(exp_avg, denom, value=-step_size * group['lr'])
        else:
            p32.add_(exp_avg, alpha=-step_size * group['lr'])
        p.copy_(p32)                     # through p, not p.data: the version counter moves, and caches keyed by it (the mapper's prepared weights) follow
        if state['step'] % group['k'] == 0:
            slow = state['slow_buffer']
            slow.add_(p.data - slow, alpha=self.alpha)
            p.copy_(slow)

    def _step_fused(self, group, params):
        from torch_utils import _sg3abi
        beta1, beta2 = group['betas']
        # tensors of one launch share the step count (they do unless parameters were added or skipped along the way)
        by_step = {}
        for p in params:
            state = self._init_state(p)
            state['step'] += 1
            by_step.setdefault((state['step'], p.device), []).append(p)
        lib = _sg3abi.load()
        for (step, device), ps in by_step.items():
            n_sma, step_size = self._schedule(step, beta1, beta2)
            for at in range(0, len(ps), _FUSED_MAX):
                chunk = ps[at:at + _FUSED_MAX]
                a = _sg3abi.RangerParams()
                a.count = len(chunk)
                for i, p in enumerate(chunk):
                    state = self.state[p]
                    t = a.t[i]
                    t.p, t.grad = p.data_ptr(), p.grad.data_ptr()
                    t.expAvg, t.expAvgSq, t.slow = state['exp_avg'].data_ptr(), state['exp_avg_sq'].data_ptr(), state['slow_buffer'].data_ptr()
                    t.rows, t.cols = (p.shape[0], p.shape[1]) if p.dim() == 2 else (1, p.numel())
                    t.centralise = int(self._centralise(p.grad))
                a.beta1, a.beta2, a.oneMinusBeta1, a.oneMinusBeta2 = beta1, beta2, 1 - beta1, 1 - beta2
                a.eps, a.decay, a.stepLr, a.alpha = group['eps'], group['weight_decay'] * group['lr'], step_size * group['lr'], self.alpha
                a.adaptive, a.lookahead = int(n_sma > self.N_sma_threshhold), int(step % group['k'] == 0)
                with torch.cuda.device(device):
                    _sg3abi.check(lib.sg3_ranger_step(a, _sg3abi.stream_ptr(device)), 'sg3_ranger_step')
                for p in chunk:          # the kernel wrote through raw pointers: move the version counters as an in-place op would
                    torch.autograd.graph.increment_version(p)
                    if self._centralise(p.grad):
                        torch.autograd.graph.increment_version(p.grad)
