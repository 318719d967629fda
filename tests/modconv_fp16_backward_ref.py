"""float64 yardsticks of the modulated convolution's backward on fp16 tensors (the generator's `use_fp16` layers), next to
tests/modconv_backward_ref.py, whose references (`dgrad_ref`, `wgrad_ref`, `modgrad_ref`) and fp32 error model they build on.

Data gradient.  `modulated_conv._data_gradient` runs the forward's single-product fp16 kernels with the roles exchanged: dy * dcoef
(times the power of two that puts its peak just below 2^15) is rounded to fp16 once, the normalised transposed weights once, the
products are exact and accumulate in fp32, s_in rides in the epilogue coefficient, dx is stored as fp16.  The bound is the one the
project holds the same arithmetic to in the forward (tests/modconv_abi.py `bounds`: max 4e-3, mean 4e-4 of max(1, max |ref|)) plus the
store: half the fp16 spacing at the result, 2^-25 (half a step of the subnormal grid 2^-24) below 2^-14.  Both operand scalings are
powers of two taken from max |dy| on the device, so the arithmetic up to the store is the same at every magnitude of dy: for
dy = m * dy_1 (m a power of two) the bound is m times the bound at m = 1 plus the store at m * ref_1 (`fp16_dgrad_bound`'s `unit`),
and once m * ref_1 is below 2^-14 what is left of it is the fp16 grid itself.

Style gradient.  The weight-gradient kernel splits each operand (times its power-of-two scale) into hi + lo with hi = the top 11
significand bits: an fp16 operand HAS 11 bits, so hi is the operand, lo = 0, and every product is exact -- the fp32 model of
modconv_backward_ref (`wgrad_bound` -> `modgrad_bound`) applies unchanged, as an upper bound with its split term unused.

Whole network.  `synthesis_fp64` evaluates a SynthesisNetwork entirely in float64 from matrix products (the input's transform algebra
restated in float64 -- the module builds its matrices from float32 identities --, one GEMM per tap for the convolutions, the banded
filter matrices of tests/flrelu_ref.py): the reference of the end-to-end d image / d ws, on whichever device the latents live.
"""
import copy
import ctypes

import numpy as np
import torch

import modconv_backward_ref as R
import style_stage_ref as S

MAGNITUDES = (2.0 ** -20, 2.0 ** -10, 1.0, 2.0 ** 10)      # max |dy| of the sweep
F16_MAX_REL, F16_MEAN_REL = 4e-3, 4e-4                    # modconv_abi.bounds of the single-product forms
F16_MIN_NORMAL = 2.0 ** -14

# kernel families and precision codes (torch_utils/_sg3abi.py)
FP32_MFMA, TORGB, ROWS, FLAT, GEMM1, F23 = range(6)
CONV_F16, CONV_F16_F23 = 2, 4

# Forward calls (N, I, O, H, W, k, demodulate; padding k - 1) whose BACKWARD launch -- I and O exchanged, the (H + k - 1) x (W + k - 1)
# gradient as its input, padding 0 -- takes each fp16 form: (precision, family, (WM, WN, TM, TN, PACK), M16, K splits) of that launch
# on a 256-CU device.  tests/test_modconv_fp16_backward_ref_cpu.py holds this table to the host-only dispatch query, the GPU test to
# the plan the launch itself reports.
DGRAD_ROWS = {
    # direct 3x3, row tiles: 32 channels x 16 rows (203 rows of M: seven tiles, the last with 11), with the tap-packed K tail
    # (51 = 3 x 16 + 3), 64 channels x 8 rows with the packed tail (100 = 6 x 16 + 4), and the taller stacks of planes of 128 rows or more
    'rows32':       ((2, 203, 128, 37, 40, 3, True), (CONV_F16, ROWS, (1, 4, 1, 4, 0), 0, 1)),
    'rows32_pack':  ((1, 81, 51, 50, 53, 3, True), (CONV_F16, ROWS, (1, 4, 1, 4, 1), 0, 1)),
    'rows64_pack':  ((2, 64, 100, 21, 24, 3, True), (CONV_F16, ROWS, (2, 2, 1, 4, 1), 0, 1)),
    'rows32_tall':  ((1, 16, 32, 130, 37, 3, True), (CONV_F16, ROWS, (1, 4, 1, 5, 0), 0, 1)),
    'rows64_tall':  ((1, 64, 20, 130, 36, 3, True), (CONV_F16, ROWS, (2, 2, 1, 6, 1), 0, 1)),
    # direct 3x3, flat runs: a padded K chunk (70 = 4 x 16 + 6); 323 rows of M = five tiles + 3 rows (an M block of pure padding);
    # 128 input channels on a grid smaller than the chip: K split over workgroups, partial images reduced afterwards
    'flat':         ((2, 64, 70, 35, 38, 3, True), (CONV_F16, FLAT, (2, 2, 1, 2, 0), 0, 1)),
    'flat_pad_m':   ((1, 323, 70, 17, 20, 3, True), (CONV_F16, FLAT, (2, 2, 1, 2, 0), 0, 1)),
    'flat_ksplit':  ((1, 323, 128, 17, 20, 3, True), (CONV_F16, FLAT, (2, 2, 1, 2, 0), 0, 2)),
    # transform domain: the backward's plane is (H + 2) x (W + 2) at padding 0, its width must be even and at least 50; 51 = 3 x 16 + 3
    # input channels and 81 = 64 + 17 rows of M; 323 = 20 x 16 + 3 and 203 = 3 x 64 + 11 (padded K chunk, an M block of pure padding)
    'f23':          ((1, 81, 51, 50, 50, 3, True), (CONV_F16_F23, F23, (2, 4, 1, 4, 0), 0, 1)),
    'f23_pad':      ((1, 203, 323, 22, 48, 3, True), (CONV_F16_F23, F23, (2, 4, 1, 4, 0), 0, 1)),
    # 1x1 GEMM (config R): the 256-row tile in the 16x16x32 form, the 128-row tile, the thin 64-row tile with one LDS image
    'gemm256':      ((2, 645, 406, 20, 23, 1, True), (CONV_F16, GEMM1, (2, 4, 4, 2, 0), 1, 1)),
    'gemm256_pad':  ((1, 203, 323, 20, 23, 1, True), (CONV_F16, GEMM1, (2, 4, 4, 2, 0), 1, 1)),
    'gemm128':      ((1, 100, 300, 20, 23, 1, True), (CONV_F16, GEMM1, (2, 4, 2, 2, 0), 1, 1)),
    'gemm_thin':    ((1, 64, 64, 33, 36, 1, True), (CONV_F16, GEMM1, (1, 8, 2, 1, 0), 0, 1)),
    # ToRGB: not demodulated, three output channels -- its adjoint is a 1x1 GEMM with K = 3 (one stage of 32, 29 of them padding)
    'torgb':        ((2, 64, 3, 33, 36, 1, False), (CONV_F16, GEMM1, (1, 8, 2, 1, 0), 0, 1)),
    'torgb_odd':    ((1, 81, 3, 21, 24, 1, False), (CONV_F16, GEMM1, (1, 8, 2, 1, 0), 0, 1)),
}


def backward_call(row):
    """(N, I, O, H, W, k, pad) of the data-gradient launch of a forward call (N, I, O, H, W, k, ...) with padding k - 1."""
    n, ci, co, h, w, k = row[:6]
    return n, co, ci, h + k - 1, w + k - 1, k, 0


def plan_key(precision, plan):
    """A recorded plan (sg3_modconv_dispatch_info as a dict) in the form of DGRAD_ROWS' expectations."""
    return (precision, plan['family'], tuple(plan[c] for c in ('WM', 'WN', 'TM', 'TN', 'PACK')), plan['M16'], plan['kSplits'])


def host_plan(call, cus=256, dtype=torch.float16):
    """The plan of a bounded call (N, I, O, H, W, k, pad) on `dtype` tensors, without a GPU: the form `modulated_conv._choose_form`
    picks, then the host-only query on the parameter block `_launch` would fill (dcoef present, unlimited scratch on offer -- `_launch`
    sizes the scratch by the same plan)."""
    from torch_utils import _sg3abi as abi
    from torch_utils.ops import modulated_conv as mc
    n, ci, co, h, w, k, pad = call
    prec = mc._choose_form(dtype, k, pad, ci, co, h, w, True)
    p = abi.ModconvParams()
    p.dcoef, p.dtype, p.precision, p.outRowStride = 16, abi.dtype_code(dtype), prec, 0
    p.N, p.I, p.O, p.H, p.W, p.k, p.pad = n, ci, co, h, w, k, pad
    p.splitScratch, p.splitScratchFloats = 16, 2 ** 62
    info = abi.ModconvDispatchInfo()
    abi.check(abi.load().sg3_modconv_dispatch(ctypes.byref(p), cus, ctypes.byref(info)), 'sg3_modconv_dispatch')
    return plan_key(prec, {name: getattr(info, name) for name, _ in info._fields_})


def wgrad_splits(n, ci, co, h, w, k, pad):
    """(bands, segment groups) of the weight-gradient launch (host-only query)."""
    from torch_utils import _sg3abi as abi
    nb, ng = ctypes.c_int(), ctypes.c_int()
    abi.check(abi.load().sg3_conv2d_wgrad_splits(n, ci, co, h, w, k, pad, ctypes.byref(nb), ctypes.byref(ng)), 'sg3_conv2d_wgrad_splits')
    return nb.value, ng.value


# ---------------------------------------------------------------------------------------------------------------- fp16 grid

def f16_half_spacing(v):
    """Half the distance between neighbouring fp16 values at |v| (float64 tensor): 2^(floor(log2 |v|) - 11), and 2^-25 -- half a
    step of the subnormal grid -- below 2^-14.  What one round-to-nearest store of v to fp16 can move it by."""
    a = v.to(torch.float64).abs().clamp_min(F16_MIN_NORMAL)
    _, e = torch.frexp(a)                                       # a = m 2^e, m in [0.5, 1): floor(log2 a) = e - 1
    return torch.exp2((e - 12).to(torch.float64))


def lattice_dy(shape, seed, device='cpu'):
    """A gradient with max |dy| = 1 exactly whose entries are multiples of 2^-4 (float64): m * dy is an fp16 value for every m of
    MAGNITUDES (at m = 2^-20 the entries are multiples of the subnormal step 2^-24; at 2^10 they stay below 65504)."""
    g = torch.Generator().manual_seed(seed)
    d = (torch.randn(shape, generator=g, dtype=torch.float64) * 4.0).round().clamp(-15, 15) / 16
    d.view(-1)[d.numel() // 3] = -1.0
    return d.to(device)


def fp16_dgrad_bound(ref, unit=1.0):
    """(element-wise bound [as ref], bound on the mean) of |dx(kernel, fp16) - ref| for a gradient dy = unit * dy_1 with max |dy_1| in
    [1, 2): unit x the single-product bounds at unit 1, plus the fp16 store of a value within that of ref."""
    scale = unit * max(1.0, float(ref.abs().max()) / unit)
    store = f16_half_spacing(ref.abs() + F16_MAX_REL * scale)
    return F16_MAX_REL * scale + store, F16_MEAN_REL * scale + float(store.mean())


def unit_of(amax):
    """The power of two m with amax / m in [1, 2)."""
    return 2.0 ** int(np.floor(np.log2(float(amax))))


def style_grad_refs(x, dy, w, s, demodulate, input_gain, k, pad, x_amax, dy_amax):
    """((dw_ref, dw_bound), (ds_ref, ds_bound)) float64 of the weight-gradient kernel + sg3_modulation_backward on x and dy as the
    kernels read them (fp16 or fp32), with the maxima the backward scaled them by."""
    n, ci, h, wd = (int(v) for v in x.shape)
    co, oh, ow = int(dy.shape[1]), int(dy.shape[2]), int(dy.shape[3])
    ref = R.wgrad_ref(x, dy, k, pad)
    b_w = R.wgrad_bound(x, dy, k, pad, x_amax, dy_amax, R.wgrad_terms(oh, ow, k, *wgrad_splits(n, ci, co, h, wd, k, pad)))
    dw_ref, ds_ref = R.modgrad_ref(ref, w, s, demodulate, input_gain)
    b_dw, b_ds = R.modgrad_bound(b_w, ref, w, s, demodulate, input_gain)
    return (dw_ref, b_dw), (ds_ref, b_ds)


# ------------------------------------------------------------------------------------------------------- the network in float64

def _input_fp64(inp, t):
    """SynthesisInput.forward (reference networks_stylegan3.py:204-244) on float64 parameters and t [N,4] float64."""
    freqs, phases, amps = S.input_transform_chain(t, inp.transform, inp.freqs, inp.phases, inp.bandwidth, inp.sampling_rate, False)
    theta = torch.eye(3, dtype=torch.float64, device=t.device)[:2].clone()
    theta[0, 0] = 0.5 * inp.size[0] / inp.sampling_rate
    theta[1, 1] = 0.5 * inp.size[1] / inp.sampling_rate
    grid = torch.nn.functional.affine_grid(theta.unsqueeze(0), [1, 1, int(inp.size[1]), int(inp.size[0])], align_corners=False)
    x = S.fourier_chain(grid[0], freqs, phases, amps).permute(0, 2, 3, 1)
    return (x @ (inp.weight / np.sqrt(inp.channels)).t()).permute(0, 3, 1, 2)


def modconv_fp64(x, w_eff, pad):
    """out[n] = conv(x[n], w_eff[n], pad) in float64 as one [O,I] x [I,P] GEMM per sample and tap (differentiable, any device)."""
    n, ci, h, w = x.shape
    co, k = int(w_eff.shape[1]), int(w_eff.shape[3])
    oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    xp = torch.nn.functional.pad(x, (pad, pad, pad, pad))
    out = None
    for ky in range(k):
        for kx in range(k):
            t = torch.bmm(w_eff[:, :, :, ky, kx], xp[:, :, ky:ky + oh, kx:kx + ow].reshape(n, ci, -1))
            out = t if out is None else out + t
    return out.reshape(n, co, oh, ow)


def flrelu_fp64(x, b, fu, fd, up, down, padding, gain, slope, clamp):
    """filtered_lrelu in float64 with the banded matrices of tests/flrelu_ref.py (`forward_ref` without its detach: differentiable)."""
    import flrelu_ref as FR
    n, c, h, w = x.shape
    ops = FR._ops((h, w), fu, fd, up, down, padding, False, x.device)
    u = FR.Ops.apply(ops.A, (x + b[None, :, None, None]).reshape(n * c, h, w))
    a, _, _ = FR._act(u, gain, slope, clamp)
    return FR.Ops.apply(ops.B, a).reshape(n, c, *ops.y_hw)


def synthesis_fp64(synthesis, ws):
    """image [N,3,R,R] float64 of `synthesis(ws)` with every parameter, buffer and activation in float64, on the device of `ws`
    (float64), from matrix products alone; differentiable with respect to `ws`."""
    dev = ws.device
    net = copy.deepcopy(synthesis).to(dev)
    taps = [(layer.up_filter, layer.down_filter) for layer in net.layers()]          # the fp32 taps, as the ops take them
    net = net.double()
    assert ws.dtype == torch.float64
    per_layer = ws.unbind(dim=1)
    x = _input_fp64(net.input, net.input.transform_params(per_layer[0]))
    for layer, w, (fu, fd) in zip(net.layers(), per_layer[1:], taps):
        w_eff = R.effective_weights64(layer.weight, layer.styles_from_w(w), not layer.is_torgb, layer.magnitude_ema.rsqrt())
        x = modconv_fp64(x, w_eff, layer.conv_kernel - 1)
        x = flrelu_fp64(x, layer.bias, fu, fd, layer.up_factor, layer.down_factor, layer.padding, (1 if layer.is_torgb else np.sqrt(2)),
                        (1 if layer.is_torgb else 0.2), layer.conv_clamp)
    return x * net.output_scale
