"""Training-mode BatchNorm2d of the encoder trunk on libsg3hip (csrc/sg3_bn_train.hip): batch statistics, the element-wise apply,
the backward's per-channel sums and its element-wise pass, and the running-statistic update.

A BatchNorm in FRONT of a convolution is never applied as a pass of its own: `stats` returns a = gamma * invstd and
b = beta - mean * a, which sg3_conv2d and sg3_conv2d_wgrad_sum take as their input affine.  A BatchNorm BEHIND a convolution is
`stats` + `apply`.  All sums are float64 in a fixed order (bit-identical on repeat); every call is one `abi.check`."""
import collections
import ctypes

import torch

from .. import _sg3abi as abi

# var is the biased batch variance; mean + mean_lo the float64 mean in two floats; count = N * H * W
Stats = collections.namedtuple('Stats', ['mean', 'var', 'invstd', 'a', 'b', 'mean_lo', 'count'])


def _check(x):
    assert x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.is_contiguous()
    return tuple(int(v) for v in x.shape)


def _vec(t, c, dev):
    if t is None:
        return None
    assert t.numel() == c
    return t.detach().to(device=dev, dtype=torch.float32).contiguous()


def _partial(x):
    n, c, h, w = x.shape
    return torch.empty([c, int(abi.load().sg3_bn_train_partials(n, h, w)), 2], dtype=torch.float64, device=x.device)


def stats(x, weight, bias, eps):
    """Batch mean / biased variance per channel of x [N,C,H,W], and the affine they make with weight, bias, eps -> Stats.  Two launches
    in one call."""
    n, c, h, w = _check(x)
    out = torch.empty([6, c], dtype=torch.float32, device=x.device)
    p = abi.BnTrainStatsParams()
    weight, bias, partial = _vec(weight, c, x.device), _vec(bias, c, x.device), _partial(x)
    p.x, p.gamma, p.beta, p.partial = abi.ptr(x), abi.ptr(weight), abi.ptr(bias), abi.ptr(partial)
    p.mean, p.var, p.invstd, p.a, p.b, p.meanLo = (abi.ptr(out[j]) for j in range(6))
    p.N, p.C, p.H, p.W, p.eps = n, c, h, w, float(eps)
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_bn_train_stats(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_bn_train_stats')
    return Stats(out[0], out[1], out[2], out[3], out[4], out[5], n * h * w)


def apply(x, scale, shift, centre=None, centre_lo=None, slope=None, want_pre=False):
    """y = PReLU(scale[c] * (x - centre[c] - centre_lo[c]) + shift[c]; slope[c]) (None: 0, slope None: no activation) -> y, or (y, pre)
    with the value in front of the activation.  For a BatchNorm behind a convolution pass scale = st.a, shift = beta, centre = st.mean,
    centre_lo = st.mean_lo: the difference is formed first, so a mean far above the spread costs nothing."""
    n, c, h, w = _check(x)
    y = torch.empty_like(x)
    pre = torch.empty_like(x) if want_pre else None
    p = abi.BnTrainApplyParams()
    scale, shift, centre, centre_lo, slope = (_vec(t, c, x.device) for t in (scale, shift, centre, centre_lo, slope))
    p.x, p.scale, p.shift, p.centre, p.centreLo, p.slope = (abi.ptr(t) for t in (x, scale, shift, centre, centre_lo, slope))
    p.y, p.pre = abi.ptr(y), abi.ptr(pre)
    p.N, p.C, p.H, p.W = n, c, h, w
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_bn_train_apply(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_bn_train_apply')
    return (y, pre) if want_pre else y


def _reduce(dy, x, mean, mean_lo, invstd, mode, slope=None, masked=None):
    n, c, h, w = _check(x)
    assert tuple(dy.shape) == tuple(x.shape) and dy.is_cuda and dy.dtype == torch.float32 and dy.is_contiguous()
    out = torch.empty([2, c], dtype=torch.float32, device=x.device)
    p = abi.BnTrainBwdReduceParams()
    partial = _partial(x)
    p.dy, p.x, p.mean, p.meanLo, p.invstd, p.partial = abi.ptr(dy), abi.ptr(x), abi.ptr(mean), abi.ptr(mean_lo), abi.ptr(invstd), abi.ptr(partial)
    p.sum1, p.sum2, p.slope, p.masked = abi.ptr(out[0]), abi.ptr(out[1]), abi.ptr(slope), abi.ptr(masked)
    p.N, p.C, p.H, p.W, p.mode = n, c, h, w, mode
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_bn_train_bwd_reduce(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_bn_train_bwd_reduce')
    return out[0], out[1]


def backward_reduce(dy, x, st):
    """(dbeta, dgamma) = (sum dy, sum dy * xhat) per channel, xhat = (x - st.mean) * st.invstd."""
    return _reduce(dy, x, st.mean, st.mean_lo, st.invstd, 0)


def slope_grad(dh, pre, slope=None):
    """Gradient of a per-channel PReLU slope: sum dh * min(pre, 0), with `pre` the activation's input.  With `slope` the same launch
    also writes the gradient in front of the activation -> (dslope, dh * (pre > 0 ? 1 : slope))."""
    if slope is None:
        return _reduce(dh, pre, None, None, None, 1)[1]
    slope, masked = _vec(slope, pre.shape[1], pre.device), torch.empty_like(pre)
    return _reduce(dh, pre, None, None, None, 1, slope, masked)[1], masked


def backward_apply(dy, x, st, dbeta, dgamma, addend=None, act=None, slope=None, want_raw=False):
    """dx = st.a * (dy - dbeta / M - xhat * dgamma / M) (+ addend, any strides), then times the derivative of the PReLU with per-channel
    `slope` whose pre-activation is `act` -> dx, or (dx, raw) with the value in front of that mask."""
    n, c, h, w = _check(x)
    assert tuple(dy.shape) == tuple(x.shape) and dy.is_cuda and dy.dtype == torch.float32 and dy.is_contiguous()
    dx = torch.empty_like(x)
    raw = torch.empty_like(x) if want_raw else None
    p = abi.BnTrainBwdApplyParams()
    p.dy, p.x, p.mean, p.meanLo, p.invstd, p.scale, p.sum1, p.sum2 = (abi.ptr(t) for t in (dy, x, st.mean, st.mean_lo, st.invstd, st.a, dbeta, dgamma))
    if addend is not None:
        assert tuple(addend.shape) == tuple(x.shape) and addend.dtype == torch.float32 and addend.device == x.device
        p.addend, p.addStride = abi.ptr(addend), abi.strides4(addend)
    if act is not None:
        assert tuple(act.shape) == tuple(x.shape) and act.is_contiguous() and act.dtype == torch.float32 and slope is not None
        slope = _vec(slope, c, x.device)
        p.act, p.slope = abi.ptr(act), abi.ptr(slope)
    p.dx, p.raw = abi.ptr(dx), abi.ptr(raw)
    p.N, p.C, p.H, p.W = n, c, h, w
    with torch.cuda.device(x.device):
        abi.check(abi.load().sg3_bn_train_bwd_apply(ctypes.byref(p), abi.stream_ptr(x.device)), 'sg3_bn_train_bwd_apply')
    return (dx, raw) if want_raw else dx


def update_running(bns, sts):
    """torch.nn.BatchNorm2d's running-statistic update for a list of modules and the Stats of their accepted forward: momentum (None:
    the cumulative average), the unbiased variance M / (M - 1), num_batches_tracked += 1.  A handful of `_foreach` operations over
    all modules at once (one per buffer kind and distinct momentum), nothing read back from the device."""
    items = [(bn, st) for bn, st in zip(bns, sts) if bn.track_running_stats and bn.running_mean is not None]
    if not items:
        return
    with torch.no_grad():
        torch._foreach_add_([bn.num_batches_tracked for bn, _ in items], 1)
        means, unbiased = [st.mean for _, st in items], torch._foreach_mul([st.var for _, st in items], [st.count / (st.count - 1.0) for _, st in items])
        fixed = [i for i, (bn, _) in enumerate(items) if bn.momentum is not None]
        cumul = [i for i, (bn, _) in enumerate(items) if bn.momentum is None]
        pick = lambda seq, idx: [seq[i] for i in idx]          # noqa: E731
        for f in sorted({float(items[i][0].momentum) for i in fixed}):
            idx = [i for i in fixed if float(items[i][0].momentum) == f]
            torch._foreach_lerp_([items[i][0].running_mean for i in idx], pick(means, idx), f)
            torch._foreach_lerp_([items[i][0].running_var for i in idx], pick(unbiased, idx), f)
        for i in cumul:         # momentum None: the cumulative average, factor 1 / num_batches_tracked formed on the device (no read-back);
            bn = items[i][0]    # a per-module loop: this is not the encoder's configuration
            f = 1.0 / bn.num_batches_tracked.to(torch.float32)
            bn.running_mean.add_((means[i] - bn.running_mean) * f)
            bn.running_var.add_((unbiased[i] - bn.running_var) * f)
