"""GPU: the modulated convolution's backward at the full 1024^2 layer shapes against float64, element by element.

1. One real pivotal-tuning step (force_fp32 MSE, as test_gpu_pti.test_pti_step_at_full_size) with every convolution recorded:
   dx, dW_eff, dw and ds of all 15 layers against tests/modconv_backward_ref.py, under the error model stated there.
2. Boundary probes of the weight-gradient split: dy is zero except on rows / columns on both sides of every band, segment group
   and segment boundary, so each split's partial image and the reduced total are short sums a misplaced pixel cannot hide in.
"""
import ctypes
import functools
import time

import pytest
import torch

import modconv_backward_ref as R
from synth_weights import synth_ws

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _f23_data_gradient(co, ci, oh, ow, k, pad):
    """True when `_data_gradient` of a layer [co <- ci] runs on the transform-domain kernel (the selection of `_plan`)."""
    from torch_utils import _sg3abi as abi
    from torch_utils.ops import modulated_conv as mc
    p = k - 1 - pad
    return (k == 3 and mc.precision == 'f16x3' and mc.f23 != 'off' and mc._f23_wanted(co, ci, oh, ow, p)
            and bool(abi.load().sg3_modconv_f23_supported(abi.SG3_F32, co, ci, oh, ow, k, p, 0)))


def _splits(n, ci, co, h, w, k, pad):
    from torch_utils import _sg3abi as abi
    nb, ng = ctypes.c_int(), ctypes.c_int()
    abi.check(abi.load().sg3_conv2d_wgrad_splits(n, ci, co, h, w, k, pad, ctypes.byref(nb), ctypes.byref(ng)), 'sg3_conv2d_wgrad_splits')
    return nb.value, ng.value


def _record_step(cfg, n):
    """One force_fp32 MSE step of the product generator with every synthesis convolution recorded: per layer name a dict of the
    convolution's inputs (x, w, s, input_gain, padding, demodulate, x_bound), dy, and the dx / ds its HIP backward returned; and
    the weight gradients of the step."""
    from helpers import build_product_generator
    from torch_utils.ops import modulated_conv as mc
    G = build_product_generator(cfg, device=DEV)
    ws = torch.from_numpy(synth_ws(n, G.num_ws, G.w_dim, seed=3)).to(DEV)
    with torch.no_grad():
        ref_img = G.synthesis(ws, noise_mode='const', force_fp32=True)
    target = (0.5 * ref_img + 0.1).detach()
    G.requires_grad_(True)
    params = list(G.synthesis.parameters())
    names = {id(getattr(G.synthesis, nm).weight): nm for nm in G.synthesis.layer_names}
    rec = {}
    orig = mc.modulated_conv2d

    def recording(x, w, s, demodulate=True, padding=0, input_gain=None, impl='cuda', x_bound=None, prepared=None, epilogue=None,
                  align_rows=False):
        name = names.get(id(w))
        if name is None or not torch.is_grad_enabled():
            return orig(x, w, s, demodulate=demodulate, padding=padding, input_gain=input_gain, impl=impl, x_bound=x_bound,
                        prepared=prepared, epilogue=epilogue, align_rows=align_rows)
        e = rec[name] = dict(x=x.detach(), w=w.detach(), s=s.detach(), padding=int(padding), demodulate=bool(demodulate), x_bound=x_bound,
                             input_gain=None if input_gain is None else input_gain.detach())
        xv, sv = x.view_as(x), s.view_as(s)            # own autograd nodes: their gradients are exactly what this call's backward returned
        xv.register_hook(lambda g: e.__setitem__('dx', g))
        sv.register_hook(lambda g: e.__setitem__('ds', g))
        y = orig(xv, w, sv, demodulate=demodulate, padding=padding, input_gain=input_gain, impl=impl, x_bound=x_bound,
                 prepared=prepared, epilogue=epilogue, align_rows=align_rows)
        y.register_hook(lambda g: e.__setitem__('dy', g))
        return y

    mc.modulated_conv2d = recording
    try:
        out = G.synthesis(ws, noise_mode='const', force_fp32=True)
        loss = torch.nn.functional.mse_loss(out, target)
        grads = torch.autograd.grad(loss, params)
    finally:
        mc.modulated_conv2d = orig
    assert sorted(rec) == sorted(G.synthesis.layer_names)
    index = {id(p): j for j, p in enumerate(params)}
    for nm in G.synthesis.layer_names:
        assert all(key in rec[nm] for key in ('dx', 'dy', 'ds')), nm
        rec[nm]['dw'] = grads[index[id(getattr(G.synthesis, nm).weight)]]
    return G.synthesis.layer_names, rec


def _ratio(err, bound):
    """max err / bound (an element with bound 0 must be exact)."""
    bad = (bound <= 0) & (err > 0)
    assert not bool(bad.any()), 'nonzero error where the bound is zero'
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize('cfg,n', [('T1024', 1), ('R1024', 1), ('T1024', 4)])
def test_full_size_step_gradients_of_every_layer_match_fp64(cfg, n):
    """dx, dW_eff, dw and ds of every convolution of one real full-size PTI step (the batched prep, the max |dx| hand-off from
    the adjoint filtered_lrelu, the layers' input bounds, the closed-form modulation backward) against float64."""
    from torch_utils.ops import known_amax
    from torch_utils.ops import modulated_conv as mc
    t0 = time.time()
    layer_names, rec = _record_step(cfg, n)
    worst = {}
    for nm in layer_names:
        e = rec.pop(nm)
        x, dy, w, s, gain = e['x'], e['dy'], e['w'], e['s'], e['input_gain']
        co, ci, k, _ = (int(v) for v in w.shape)
        pad, demod = e['padding'], e['demodulate']
        oh, ow = int(dy.shape[2]), int(dy.shape[3])
        # the maxima the backward scaled its operands by: the adjoint's hand-off (a bound: it must not be below max |dy|)
        dy_max = float(mc._amax(dy))
        known = known_amax.lookup(dy)
        dy_amax = dy_max if known is None else float(known)
        assert dy_amax >= dy_max, (nm, dy_amax, dy_max)
        x_amax = float(e['x_bound']) if e['x_bound'] is not None and e['x_bound'] > 0 else float(mc._amax(x))
        assert x_amax >= float(mc._amax(x)), nm                                     # the layer's input bound holds
        # dx: element-wise; each element is a short sum, a wrong pixel is an O(1) error
        w_eff = R.effective_weights64(w, s, demod, gain)
        dx_ref = R.dgrad_ref(dy, w_eff, k, pad)
        f23 = _f23_data_gradient(co, ci, oh, ow, k, pad)
        b_dx, _ = R.dgrad_bound(dy, w, s, demod, gain, k, pad, dy_amax, f23)
        r_dx = _ratio((e['dx'].to(torch.float64) - dx_ref).abs(), b_dx)
        del dx_ref, b_dx, w_eff
        # dW_eff: the weight-gradient kernel with the tensors and bounds of this step's backward
        sx = None if e['x_bound'] is None or e['x_bound'] <= 0 else mc._bound_scalar(e['x_bound'], x.device)
        sd = torch.tensor([dy_amax], dtype=torch.float32, device=x.device)
        got = mc._weight_gradient(x, dy, k, pad, x_amax=sx, dy_amax=sd)
        ref = R.wgrad_ref(x, dy, k, pad)
        b_w = R.wgrad_bound(x, dy, k, pad, x_amax, dy_amax, R.wgrad_terms(oh, ow, k, *_splits(n, ci, co, int(x.shape[2]), int(x.shape[3]), k, pad)))
        r_weff = _ratio((got.to(torch.float64) - ref).abs(), b_w)
        # dw (weight.grad) and ds: the chain rule from the exact dW_eff, the dW_eff error pushed through the abs-Jacobian
        dw_ref, ds_ref = R.modgrad_ref(ref, w, s, demod, gain)
        b_dw, b_ds = R.modgrad_bound(b_w, ref, w, s, demod, gain)
        r_dw = _ratio((e['dw'].to(torch.float64) - dw_ref).abs(), b_dw)
        r_ds = _ratio((e['ds'].to(torch.float64) - ds_ref).abs(), b_ds)
        worst[nm] = (r_dx, r_weff, r_dw, r_ds)
        print(f'{cfg} N={n} {nm:14s} {ci:4d}->{co:4d} k{k} {"F23 " if f23 else "    "}err/bound  dx {r_dx:.3f}  dW_eff {r_weff:.3f}  '
              f'dw {r_dw:.3f}  ds {r_ds:.3f}')
        del e, x, dy, got, ref, b_w
    torch.cuda.synchronize()
    print(f'{cfg} N={n}: {time.time() - t0:.1f} s')
    failed = {nm: r for nm, r in worst.items() if max(r) > 1.0}
    assert not failed, f'err/bound (dx, dW_eff, dw, ds) above 1: {failed}'


# -------------------------------------------------------------------------------------------------- weight-gradient split probes

@functools.lru_cache(maxsize=None)
def _layer_shapes(cfg):
    """(I, O, H, W, k, pad) of the 15 synthesis convolutions of a configuration (a CPU generator: shapes only)."""
    from models.stylegan3.networks_stylegan3 import Generator
    from synth_weights import CONFIGS
    G = Generator(**CONFIGS[cfg])
    out = []
    for nm in G.synthesis.layer_names:
        L = getattr(G.synthesis, nm)
        out.append((int(L.in_channels), int(L.out_channels), int(L.in_size[1]), int(L.in_size[0]), int(L.conv_kernel), int(L.conv_kernel) - 1))
    return out


def _edges(c):
    """Channels at the 32- and 64-channel tile edges, and the first and last one."""
    return sorted({v for j in range(1, c // 32 + 1) for v in (32 * j - 1, 32 * j) if v < c} | {0, c - 1})


def _probe_lines(extent, cuts):
    return sorted({0, extent - 1} | {v for c in cuts if 0 < c < extent for v in (c - 1, c)})


def _check_split_probes(n, ci, co, h, w, k, pad, seed):
    from torch_utils.ops import modulated_conv as mc
    oh, ow = h + 2 * pad - k + 1, w + 2 * pad - k + 1
    nb, ng = _splits(n, ci, co, h, w, k, pad)
    band_rows = -(-oh // nb)                                  # as launch_wgrad computes them
    n_segs = -(-ow // 32)
    spg = -(-n_segs // ng)
    rows = _probe_lines(oh, [b * band_rows for b in range(1, nb)])
    cols = _probe_lines(ow, [g * spg * 32 for g in range(1, ng)] + [j * 32 for j in range(1, spg)]
                        + [((ng - 1) * spg + j) * 32 for j in range(1, spg)])
    oc, ic = _edges(co), _edges(ci)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    ri = torch.tensor(rows, device=DEV); cj = torch.tensor(cols, device=DEV)
    oi = torch.tensor(oc, device=DEV); ii = torch.tensor(ic, device=DEV)
    dy = torch.zeros([n, co, oh, ow], dtype=torch.float32, device=DEV)
    dy[:, oi[:, None, None], ri[None, :, None], cj[None, None, :]] = torch.randn([n, len(oc), len(rows), len(cols)], device=DEV, generator=gen) * 3e-6
    x = torch.zeros([n, ci, h, w], dtype=torch.float32, device=DEV)
    x[:, ii] = torch.randn([n, len(ic), h, w], device=DEV, generator=gen) * 60
    # fp64 per split: the probe grid's points inside its band x segment-group window
    xp = torch.nn.functional.pad(x.to(torch.float64), (pad, pad, pad, pad))
    taps = [(ky, kx) for ky in range(k) for kx in range(k)]
    ref = torch.zeros([nb * ng, n, k * k, co, ci], dtype=torch.float64, device=DEV)
    scale = torch.zeros_like(ref)
    sum_x = torch.zeros([nb * ng, n, k * k, 1, ci], dtype=torch.float64, device=DEV)
    sum_d = torch.zeros([nb * ng, n, 1, co, 1], dtype=torch.float64, device=DEV)
    for b in range(nb):
        rb = torch.tensor([r for r in rows if r // band_rows == b], device=DEV)
        for g in range(ng):
            cg = torch.tensor([c for c in cols if c // (spg * 32) == g], device=DEV)
            sp = b * ng + g
            D = dy[:, :, rb][:, :, :, cg].to(torch.float64)                                     # [N,O,r,c]
            X = torch.stack([xp[:, :, rb + ky][:, :, :, cg + kx] for ky, kx in taps], 2)       # [N,I,T,r,c]
            ref[sp] = torch.einsum('norc,nitrc->ntoi', D, X)
            scale[sp] = torch.einsum('norc,nitrc->ntoi', D.abs(), X.abs())
            sum_x[sp, :, :, 0] = X.abs().sum([3, 4]).transpose(1, 2)
            sum_d[sp, :, 0, :, 0] = D.abs().sum([2, 3])
    sx, sd = R.pow2_scale(float(x.abs().max())), R.pow2_scale(float(dy.abs().max()))
    c_rel = R.C_SPLIT + R._acc(R.wgrad_terms(oh, ow, k, nb, ng)) + 2 * R.U
    bound = c_rel * scale + R.FLOOR * (sum_d / sx + sum_x / sd) * (1 + 1e-3)
    # the partials, from a buffer in which every element the kernel fails to write stays NaN
    buf = torch.full([nb * ng, n, k * k, co, ci], float('nan'), dtype=torch.float32, device=DEV)
    partial = mc._weight_gradient_partials(x, dy, k, pad, partial=buf).to(torch.float64)
    assert tuple(partial.shape) == tuple(ref.shape)
    err = (partial - ref).abs()
    assert not bool(torch.isnan(partial).any()), 'unwritten partial elements'
    per_split = (err / bound.clamp_min(1e-300)).flatten(1).amax(1)                              # [S]
    per_split[((bound <= 0) & (err > 0)).flatten(1).any(1)] = float('inf')
    bad = [(int(sp) // ng, int(sp) % ng, float(per_split[sp])) for sp in torch.nonzero(per_split > 1).flatten()]
    tag = f'N={n} {ci}->{co} {h}x{w} k{k} pad{pad}: {nb} bands x {ng} segment groups, band {band_rows} rows, {spg} segments per group'
    assert not bad, f'{tag}: partials off in (band, group, err/bound) {bad[:8]}'
    # the total that `_weight_gradient` reduces, against the sum over all probe pixels
    total = mc._weight_gradient(x, dy, k, pad).to(torch.float64)                                # [N,O,I,k,k]
    as_taps = lambda t: t.permute(0, 2, 3, 1).reshape(n, co, ci, k, k)                        # noqa: E731  [N,T,O,I] -> [N,O,I,k,k]
    ref_t = as_taps(ref.sum(0))
    bound_t = as_taps(bound.sum(0)) + R._acc(nb * ng) * as_taps(scale.sum(0))
    r_tot = _ratio((total - ref_t).abs(), bound_t)
    if r_tot > 1:
        # name the split(s) whose window the total is missing (or has twice)
        named = []
        for sp in range(nb * ng):
            part = as_taps(ref[sp])
            for sign, what in ((-1, 'missing'), (1, 'counted twice')):
                if float(((total - (ref_t + sign * part)).abs() - bound_t).max()) <= 0:
                    named.append(f'split {sp} (band {sp // ng}, group {sp % ng}) {what}')
        raise AssertionError(f'{tag}: reduced total err/bound {r_tot:.3g}; {named or "no single split explains it"}')
    return max(float(per_split.max()), r_tot), (nb, ng)


@pytest.mark.parametrize('cfg', ['T1024', 'R1024'])
def test_wgrad_split_boundaries_at_full_size_layer_shapes(cfg):
    """Every distinct full-size layer shape of the configuration at N = 1 and 4: each split's partial == the fp64 sum over the
    probe pixels inside its own band x segment-group window, and the reduced total == the sum over all probe pixels."""
    t0 = time.time()
    shapes = sorted(set(_layer_shapes(cfg)), key=lambda t: (-t[2], t))
    if cfg == 'T1024':       # tiles whose waves share taps: one and two 32 x 32 blocks (wgrad tile = O x I)
        assert {(32, 32), (51, 32), (81, 51)} <= {(ci, co) for ci, co, *_ in shapes}
    else:
        assert (64, 64) in {(ci, co) for ci, co, *_ in shapes}
    for n in (1, 4):
        for j, (ci, co, h, w, k, pad) in enumerate(shapes):
            r, (nb, ng) = _check_split_probes(n, ci, co, h, w, k, pad, seed=1000 * n + j)
            print(f'{cfg} N={n} {ci:4d}->{co:4d} {h}x{w} k{k}: {nb:3d} x {ng:2d} splits, max err/bound {r:.3g}')
    print(f'{cfg}: {time.time() - t0:.1f} s')
