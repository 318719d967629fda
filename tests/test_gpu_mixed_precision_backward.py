"""GPU: the backward of the mixed-precision synthesis network -- what StyleCLIP mapper training differentiates -- against float64.

The decoder's parameters are frozen there and the latents need a gradient, so every `use_fp16` layer runs: the data gradient on the
single-product fp16 kernels with the roles exchanged, the weight-gradient kernel on fp16 tensors feeding `sg3_modulation_backward`
for ds alone, the fp16 adjoint of filtered_lrelu handing max |dx| on, and the casts at the fp32 -> fp16 boundary.  References,
bounds and the row table: tests/modconv_fp16_backward_ref.py (its own arithmetic: tests/test_modconv_fp16_backward_ref_cpu.py).

1. Data gradient, form by form (`test_data_gradient_on_fp16_tensors_form_by_form`).  Rows of `DGRAD_ROWS` and the plan their BACKWARD
   launch must report (family, (WM, WN, TM, TN, PACK), M16, K splits), each at max |dy| = 2^-20, 2^-10, 1, 2^10:
       rows32        2 x 203 -> 128 @ 37 x 40  k3   SG3_CONV_F16      ROWS  (1,4,1,4,0)       32-channel tile, M = 203 in seven tiles
       rows32_pack   1 x  81 ->  51 @ 50 x 53  k3   SG3_CONV_F16      ROWS  (1,4,1,4,1)       K = 51: tap-packed tail chunk
       rows64_pack   2 x  64 -> 100 @ 21 x 24  k3   SG3_CONV_F16      ROWS  (2,2,1,4,1)       64-channel tile, K = 100
       rows32_tall   1 x  16 ->  32 @ 130 x 37 k3   SG3_CONV_F16      ROWS  (1,4,1,5,0)       five rows per wave (planes of 128 rows and more)
       rows64_tall   1 x  64 ->  20 @ 130 x 36 k3   SG3_CONV_F16      ROWS  (2,2,1,6,1)       six rows per wave
       flat          2 x  64 ->  70 @ 35 x 38  k3   SG3_CONV_F16      FLAT  (2,2,1,2,0)       K = 70: padded chunk
       flat_pad_m    1 x 323 ->  70 @ 17 x 20  k3   SG3_CONV_F16      FLAT  (2,2,1,2,0)       M = 323: a block of pure padding
       flat_ksplit   1 x 323 -> 128 @ 17 x 20  k3   SG3_CONV_F16      FLAT  (2,2,1,2,0) x 2   K split over workgroups
       f23           1 x  81 ->  51 @ 50 x 50  k3   SG3_CONV_F16_F23  F23   (2,4,1,4,0)       plane 52 x 52, pad 0; K = 51, M = 81
       f23_pad       1 x 203 -> 323 @ 22 x 48  k3   SG3_CONV_F16_F23  F23   (2,4,1,4,0)       K = 323, M = 203 (as 323 -> 203 in fp32)
       gemm256       2 x 645 -> 406 @ 20 x 23  k1   SG3_CONV_F16      GEMM1 (2,4,4,2,0) M16   256-row tile
       gemm256_pad   1 x 203 -> 323 @ 20 x 23  k1   SG3_CONV_F16      GEMM1 (2,4,4,2,0) M16   K = 323 (eleven stages of 32), M = 203
       gemm128       1 x 100 -> 300 @ 20 x 23  k1   SG3_CONV_F16      GEMM1 (2,4,2,2,0) M16   128-row tile
       gemm_thin     1 x  64 ->  64 @ 33 x 36  k1   SG3_CONV_F16      GEMM1 (1,8,2,1,0)       64-row tile, one LDS image
       torgb         2 x  64 ->   3 @ 33 x 36  k1   SG3_CONV_F16      GEMM1 (1,8,2,1,0)       not demodulated; the adjoint's K = 3
       torgb_odd     1 x  81 ->   3 @ 21 x 24  k1   SG3_CONV_F16      GEMM1 (1,8,2,1,0)       K = 3, M = 81
2. Style gradient with a frozen weight (`test_style_gradient_*`): ds bit-identical with and without dw, None returned for w, both
   against `modgrad_ref(wgrad_ref(x16, dy16))` under `wgrad_bound` -> `modgrad_bound`; one case takes dy from a real fp16
   filtered_lrelu adjoint and its scale from `known_amax`.
3. One whole backward, layer by layer, and d image / d ws end to end against the composite execution as the yardstick.
4. One coach step on a mixed-precision decoder against the same step with a composite decoder and mapper.
"""
import contextlib
import functools
import math
import time
import zlib

import numpy as np
import pytest
import torch

import flrelu_ref as FR
import modconv_backward_ref as R
import modconv_fp16_backward_ref as H
from flrelu_record import setup_kwargs
from synth_weights import synth_state_dict, synth_ws

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
X_BOUND = 256.0 * 1.01          # a layer's input bound: the previous layer's clamp times its down filter's L1 norm (>= 1) and 1.01
FAMILY = ['FP32_MFMA', 'TORGB', 'ROWS', 'FLAT', 'GEMM1', 'F23']


class _plans:
    """Records the plan the library made (sg3_modconv_dispatch) for every modulated convolution launched inside the block."""

    def __enter__(self):
        from torch_utils.ops import modulated_conv as mc
        mc.dispatch_log = self.log = []
        return self.log

    def __exit__(self, *exc):
        from torch_utils.ops import modulated_conv as mc
        mc.dispatch_log = None


def _fp16_key(plan):
    """A recorded plan as a DGRAD_ROWS expectation.  The log carries no precision code; a single-product launch (SPLIT = 0) of the
    transform-domain family is SG3_CONV_F16_F23, of the direct families SG3_CONV_F16; anything else comes back as it is and mismatches."""
    if plan['SPLIT'] != 0 or plan['family'] not in (H.ROWS, H.FLAT, H.GEMM1, H.F23):
        return ('not a single-product fp16 form', FAMILY[plan['family']], plan['SPLIT'])
    return H.plan_key(H.CONV_F16_F23 if plan['family'] == H.F23 else H.CONV_F16, plan)


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


# ------------------------------------------------------------------------------------------------ 1. data gradient, form by form

@functools.lru_cache(maxsize=None)
def _row(name):
    """Inputs of a row and its float64 data gradient at max |dy| = 1, made once and shared by the row's four magnitudes."""
    (n, ci, co, h, w, k, demod), _ = H.DGRAD_ROWS[name]
    g = torch.Generator().manual_seed(_seed(name))
    x = (torch.randn([n, ci, h, w], generator=g) * 20).clamp(-256, 256).half().to(DEV)
    wt = torch.randn([co, ci, k, k], generator=g).to(DEV)
    s = torch.randn([n, ci], generator=g) + 1.0
    if not demod:
        s = s / math.sqrt(ci)                                   # ToRGB styles carry the 1 / sqrt(fan_in) weight gain
    s = s.to(DEV)
    gain = torch.tensor(0.8, device=DEV)
    dy1 = H.lattice_dy([n, co, h + k - 1, w + k - 1], _seed(name) + 1, DEV)
    ref1 = R.dgrad_ref(dy1, R.effective_weights64(wt, s, demod, gain), k, k - 1)
    return x, wt, s, gain, dy1, ref1


@pytest.mark.parametrize('m', H.MAGNITUDES, ids=['2^-20', '2^-10', '1', '2^10'])
@pytest.mark.parametrize('name', sorted(H.DGRAD_ROWS))
def test_data_gradient_on_fp16_tensors_form_by_form(name, m):
    """dx of `modulated_conv2d` on fp16 tensors through autograd, the backward launch's plan proven from `dispatch_log`, against
    `dgrad_ref` (float64, the fp16 dy and the float64 effective weights) under `fp16_dgrad_bound`: 4e-3 (max) and 4e-4 (mean) of
    m * max(1, max |ref at m = 1|) plus the fp16 store -- the same relative bound at every magnitude, and the fp16 grid where dx is
    subnormal (m = 2^-20: every element; the relative part is then below a quarter of a grid step)."""
    from torch_utils.ops import modulated_conv as mc
    (n, ci, co, h, w, k, demod), want = H.DGRAD_ROWS[name]
    x, wt, s, gain, dy1, ref1 = _row(name)
    dy = (dy1 * m).half()
    assert torch.equal(dy.double(), dy1 * m) and float(dy.abs().max()) == m
    xr = x.clone().requires_grad_(True)
    with _plans() as plans:
        y = mc.modulated_conv2d(xr, wt, s, demodulate=demod, padding=k - 1, input_gain=gain, x_bound=X_BOUND)
        forward = len(plans)
        (dx,) = torch.autograd.grad(y, xr, dy)
    assert forward == 1 and len(plans) == 2, [FAMILY[p['family']] for p in plans]
    ref = ref1 * m
    err = (dx.double() - ref).abs()
    bound, mean_bound = H.fp16_dgrad_bound(ref, m)
    r_max, r_mean = float((err / bound).max()), float(err.mean()) / mean_bound
    scale = m * max(1.0, float(ref1.abs().max()))
    print(f'{name:12s} m {m:9.3e} {n} x {ci:3d} -> {co:3d} @ {h} x {w} k{k}  backward {FAMILY[plans[1]["family"]]} {_fp16_key(plans[1])[2:]}  '
          f'max {float(err.max()) / scale:.3e} of scale, err/bound max {r_max:.3f} mean {r_mean:.3f}  '
          f'subnormal dx {float((ref.abs() < H.F16_MIN_NORMAL).double().mean()):.3f}  zero dx {float((dx == 0).double().mean()):.4f}')
    assert _fp16_key(plans[1]) == want, (name, _fp16_key(plans[1]), want)
    assert dx.dtype == torch.float16 and dx.shape == x.shape and bool(torch.isfinite(dx).all())
    assert r_max <= 1.0 and r_mean <= 1.0, (name, m, r_max, r_mean)


# ------------------------------------------------------------------------------------------- 2. style gradient, frozen weight

def _spy_backward():
    """Patches `_ModulatedConv2dHip.backward` to keep what it returns; -> (list of returned tuples, restore())."""
    from torch_utils.ops import modulated_conv as mc
    orig, seen = mc._ModulatedConv2dHip.backward, []

    def spy(ctx, dy):
        out = orig(ctx, dy)
        seen.append(out)
        return out

    def restore():
        mc._ModulatedConv2dHip.backward = staticmethod(orig)
    mc._ModulatedConv2dHip.backward = staticmethod(spy)
    return seen, restore


def _style_grads(x, w, s, gain, demod, k, dy, w_grad):
    """(dx, ds, dw or None) through autograd with x and s needing gradients and w only if `w_grad`; and what backward returned."""
    from torch_utils.ops import modulated_conv as mc
    seen, restore = _spy_backward()
    try:
        xr, sr, wr = x.clone().requires_grad_(True), s.clone().requires_grad_(True), w.clone().requires_grad_(w_grad)
        y = mc.modulated_conv2d(xr, wr, sr, demodulate=demod, padding=k - 1, input_gain=gain, x_bound=X_BOUND)
        grads = torch.autograd.grad(y, [xr, sr] + ([wr] if w_grad else []), dy)
    finally:
        restore()
    assert len(seen) == 1
    return grads[0], grads[1], (grads[2] if w_grad else None), seen[0]


def _gain(kind, n, ci, g):
    return {'scalar': torch.tensor(0.8), 'per_channel': torch.rand([ci], generator=g) + 0.5, 'per_sample': torch.rand([n, ci], generator=g) + 0.5}[kind].to(DEV)


STYLE_CASES = [(3, demod, gain, n) for demod in (True, False) for gain in ('scalar', 'per_channel', 'per_sample') for n in (1, 3)] \
    + [(1, True, 'scalar', 3), (1, False, 'per_sample', 1)]


@pytest.mark.parametrize('k,demod,gain_kind,n', STYLE_CASES)
def test_style_gradient_with_a_frozen_weight(k, demod, gain_kind, n):
    """need = (x, -, s), the combination of mapper training: ds equals, bit for bit, the ds of the run that also asks for dw; backward
    returns None for w.  Both against float64 under the fp32 chain `wgrad_bound` -> `modgrad_bound`: fp16 operands have 11 significand
    bits, the kernel's hi part keeps 11, so its split of them is exact and the fp32 model holds as it stands (51 -> 37 @ 20 x 23 for
    k = 3: a thin weight-gradient tile with channel tails; 64 -> 48 @ 20 x 22 for k = 1)."""
    ci, co, h, w = (51, 37, 20, 23) if k == 3 else (64, 48, 20, 22)
    g = torch.Generator().manual_seed(100 * k + 10 * n + int(demod))
    x = (torch.randn([n, ci, h, w], generator=g) * 20).clamp(-256, 256).half().to(DEV)
    wt = torch.randn([co, ci, k, k], generator=g).to(DEV)
    s = (torch.randn([n, ci], generator=g) + 1.0).to(DEV)
    gain = _gain(gain_kind, n, ci, g)
    dy = (H.lattice_dy([n, co, h + k - 1, w + k - 1], 7 + n, DEV) * 2.0 ** -10).half()
    dx_f, ds_f, _, ret_f = _style_grads(x, wt, s, gain, demod, k, dy, w_grad=False)
    dx_b, ds_b, dw_b, ret_b = _style_grads(x, wt, s, gain, demod, k, dy, w_grad=True)
    assert ret_f[1] is None and ret_f[2] is not None and ret_f[0] is not None and ret_b[1] is not None
    assert ds_f.dtype == torch.float32 and torch.equal(ds_f, ds_b) and torch.equal(dx_f, dx_b)
    (dw_ref, b_dw), (ds_ref, b_ds) = H.style_grad_refs(x, dy, wt, s, demod, gain, k, k - 1, X_BOUND, float(dy.abs().max()))
    r_ds = FR.ratio((ds_f.double() - ds_ref).abs(), b_ds)
    r_dw = FR.ratio((dw_b.double() - dw_ref).abs(), b_dw)
    print(f'k{k} demodulate {demod} gain {gain_kind} N={n}: err/bound ds {r_ds:.3f} dw {r_dw:.3f}  '
          f'(ds: max error {float((ds_f.double() - ds_ref).abs().max()):.3e} of max {float(ds_ref.abs().max()):.3e})')
    assert r_ds <= 1.0 and r_dw <= 1.0, (r_ds, r_dw)


MIXED = {       # 256 pixels, at most 32 channels: layers 0 - 2 (sampling rate 16) are fp32, layers 3 - 14 fp16 with the default num_fp16_res
    'T': dict(z_dim=512, c_dim=0, w_dim=512, img_resolution=256, img_channels=3, channel_base=2048, channel_max=32),
    'R': dict(z_dim=512, c_dim=0, w_dim=512, img_resolution=256, img_channels=3, channel_base=4096, channel_max=32, conv_kernel=1,
              use_radial_filters=True),
}


@functools.lru_cache(maxsize=None)
def _mixed(cfg):
    """The seeded generator of MIXED[cfg] on the GPU, frozen, with the default mixed precision."""
    from models.stylegan3.networks_stylegan3 import Generator
    G = Generator(**MIXED[cfg]).eval().requires_grad_(False)
    man = {k: list(v.shape) for k, v in G.state_dict().items()}
    sd = synth_state_dict(man, seed=0, input_bandwidth=float(G.synthesis.input.bandwidth))
    missing, unexpected = G.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k.endswith('_filter') for k in missing)
    return G.to(DEV)


def test_style_gradient_with_dy_from_a_real_fp16_adjoint():
    """modulated_conv2d -> filtered_lrelu on fp16 tensors with a frozen weight, as a layer runs them: dy is what the fp16 adjoint
    wrote, its max comes from `known_amax.lookup` (asserted: one hit, the value is max |dy| exactly), and dx, ds are bit-equal to the
    run with the hand-off disabled; ds against float64 with that scale."""
    from torch_utils.ops import filtered_lrelu as fl
    from torch_utils.ops import known_amax
    from torch_utils.ops import modulated_conv as mc
    syn = _mixed('T').synthesis
    L = next(layer for layer in syn.layers() if layer.use_fp16 and layer.up_factor == 2 and not layer.is_torgb)
    n, ci, k, side = 2, int(L.in_channels), int(L.conv_kernel), int(L.in_size[0])
    g = torch.Generator().manual_seed(41)
    x = (torch.randn([n, ci, side, side], generator=g) * 20).clamp(-256, 256).half().to(DEV)
    s = (torch.randn([n, ci], generator=g) + 1.0).to(DEV)
    gain = L.magnitude_ema.rsqrt()
    assert not L.weight.requires_grad

    def run():
        xr, sr = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
        kept = {}
        y = mc.modulated_conv2d(xr, L.weight, sr, demodulate=True, padding=k - 1, input_gain=gain, x_bound=X_BOUND)
        y.register_hook(lambda t: kept.__setitem__('dy', t))
        z = fl.filtered_lrelu(y, fu=L.up_filter, fd=L.down_filter, b=L.bias.half(), up=L.up_factor, down=L.down_factor, padding=L.padding,
                              gain=np.sqrt(2), slope=0.2, clamp=L.conv_clamp)
        up = (H.lattice_dy(list(z.shape), 43, DEV) * 2.0 ** -12).half()
        before = known_amax.hits
        dx, ds = torch.autograd.grad(z, [xr, sr], up)
        return dx, ds, kept['dy'], known_amax.hits - before

    dx, ds, dy, hits = run()
    assert dy.dtype == torch.float16 and hits == 1
    known = known_amax.lookup(dy)
    assert known is not None and float(known) == float(dy.abs().max()) > 0
    known_amax.enabled = False
    try:
        dx0, ds0, dy0, hits0 = run()
    finally:
        known_amax.enabled = True
    assert hits0 == 0 and torch.equal(dy, dy0) and torch.equal(ds, ds0) and torch.equal(dx, dx0)
    (_, _), (ds_ref, b_ds) = H.style_grad_refs(x, dy, L.weight, s, True, gain, k, k - 1, X_BOUND, float(known))
    r_ds = FR.ratio((ds.double() - ds_ref).abs(), b_ds)
    print(f'{ci} -> {int(L.out_channels)} @ {side}^2, dy from the fp16 adjoint (max {float(known):.3e}): ds err/bound {r_ds:.3f}')
    assert r_ds <= 1.0


# ------------------------------------------------------------------------------------------------ 3. one whole backward

def _record_backward(G, ws, g, which):
    """d sum(image * g) / d ws of `G.synthesis(ws)` with the default options, every layer's modulated_conv2d and filtered_lrelu call
    recorded (inputs, output, dy, and the dx / ds its backward returned).  `which` = 'cuda': the HIP ops; 'ref': the composite
    execution of both ops on the same fp16 layers (the convolution outside MIOpen, whose first call of every shape compiles)."""
    from torch_utils.ops import filtered_lrelu as fl
    from torch_utils.ops import modulated_conv as mc
    syn = G.synthesis
    names = list(syn.layer_names)
    by_weight = {id(getattr(syn, nm).weight): nm for nm in names}
    conv, act, order = {}, {}, []
    orig_mc, orig_fl = mc.modulated_conv2d, fl.filtered_lrelu

    def rec_conv(x, w, s, demodulate=True, padding=0, input_gain=None, impl='cuda', x_bound=None, prepared=None, epilogue=None, align_rows=False):
        nm = by_weight[id(w)]
        e = conv[nm] = dict(x=x.detach(), w=w.detach(), s=s.detach(), padding=int(padding), demodulate=bool(demodulate), x_bound=x_bound,
                            input_gain=None if input_gain is None else input_gain.detach())
        xv, sv = x.view_as(x), s.view_as(s)            # own autograd nodes: their gradients are exactly what this call's backward returned
        xv.register_hook(lambda t: e.__setitem__('dx', t))
        sv.register_hook(lambda t: e.__setitem__('ds', t))
        y = orig_mc(xv, w, sv, demodulate=demodulate, padding=padding, input_gain=input_gain, impl=which, x_bound=x_bound,
                    prepared=prepared if which == 'cuda' else None, epilogue=epilogue, align_rows=align_rows)
        y.register_hook(lambda t: e.__setitem__('dy', t))
        return y

    def rec_act(x, fu=None, fd=None, b=None, up=1, down=1, padding=0, gain=2 ** 0.5, slope=0.2, clamp=None, flip_filter=False, impl='cuda'):
        nm = names[len(order)]
        order.append(nm)
        e = act[nm] = dict(x=x.detach(), b=b.detach(), fu=fu, fd=fd, up=int(up), down=int(down), padding=list(padding), gain=float(gain),
                           slope=float(slope), clamp=clamp)
        xv = x.view_as(x)
        xv.register_hook(lambda t: e.__setitem__('dx', t))
        y = orig_fl(x=xv, fu=fu, fd=fd, b=b, up=up, down=down, padding=padding, gain=gain, slope=slope, clamp=clamp, flip_filter=flip_filter,
                    impl=which)
        e['y'] = y.detach()
        y.register_hook(lambda t: e.__setitem__('dy', t))
        return y

    mc.modulated_conv2d, fl.filtered_lrelu = rec_conv, rec_act
    try:
        wr = ws.detach().clone().requires_grad_(True)
        with torch.backends.cudnn.flags(enabled=(which == 'cuda')):
            img = syn(wr)
            (gw,) = torch.autograd.grad((img * g).sum(), wr)
    finally:
        mc.modulated_conv2d, fl.filtered_lrelu = orig_mc, orig_fl
    assert order == names and sorted(conv) == sorted(names)
    for nm in names:
        assert all(key in conv[nm] for key in ('dx', 'ds', 'dy')) and all(key in act[nm] for key in ('dx', 'dy')), nm
    return gw, img.detach(), conv, act


@functools.lru_cache(maxsize=None)
def _network_case(cfg):
    """(generator, ws [2, num_ws, 512], g [2, 3, 256, 256] ~ N(0, 1), float64 d sum(image * g) / d ws), the reference made once."""
    G = _mixed(cfg)
    ws = torch.from_numpy(synth_ws(2, G.num_ws, G.w_dim, seed=3)).to(DEV)
    g = torch.from_numpy(np.random.RandomState(11).randn(2, 3, 256, 256).astype(np.float32)).to(DEV)
    w64 = ws.double().requires_grad_(True)
    img64 = H.synthesis_fp64(G.synthesis, w64)
    (g64,) = torch.autograd.grad((img64 * g.double()).sum(), w64)
    FR._ops_cache.clear()
    return G, ws, g, g64.detach(), img64.detach()


def _check_conv(nm, e):
    """(err/bound of dx, of ds, fp16?) of one recorded convolution against float64."""
    from torch_utils.ops import known_amax
    from torch_utils.ops import modulated_conv as mc
    x, dy, w, s, gain = e['x'], e['dy'], e['w'], e['s'], e['input_gain']
    k, pad, demod = int(w.shape[2]), e['padding'], e['demodulate']
    fp16 = x.dtype == torch.float16
    assert dy.dtype == x.dtype and e['dx'].dtype == x.dtype and e['ds'].dtype == torch.float32, nm
    dy_max = float(mc._amax(dy))
    known = known_amax.lookup(dy)
    dy_amax = dy_max if known is None else float(known)
    assert dy_amax >= dy_max > 0, (nm, dy_amax, dy_max)
    assert e['x_bound'] is not None and e['x_bound'] >= float(mc._amax(x)), nm                  # the layer's input bound holds
    dx_ref = R.dgrad_ref(dy, R.effective_weights64(w, s, demod, gain), k, pad)
    err = (e['dx'].double() - dx_ref).abs()
    if fp16:
        bound, mean_bound = H.fp16_dgrad_bound(dx_ref, H.unit_of(dy_max))
        r_dx = max(float((err / bound).max()), float(err.mean()) / mean_bound)
    else:
        co, ci = int(w.shape[0]), int(w.shape[1])
        assert not (k == 3 and mc._f23_wanted(co, ci, int(dy.shape[2]), int(dy.shape[3]), k - 1 - pad))     # thin layers: the direct kernel
        bound, _ = R.dgrad_bound(dy, w, s, demod, gain, k, pad, dy_amax, False)
        r_dx = FR.ratio(err, bound)
    (_, _), (ds_ref, b_ds) = H.style_grad_refs(x, dy, w, s, demod, gain, k, pad, float(e['x_bound']), dy_amax)
    return r_dx, FR.ratio((e['ds'].double() - ds_ref).abs(), b_ds), fp16


def _check_act(e):
    """(err/bound of y, of dx, share of dx elements whose bound a sign decision widens) of one recorded filtered_lrelu call."""
    kw = setup_kwargs(e)
    x, b, fu, fd = e['x'], e['b'], e['fu'], e['fd']
    fp16 = x.dtype == torch.float16
    xhw = tuple(x.shape[2:])
    y64, u64 = FR.forward_ref(x, b, fu, fd, **kw)
    scales = FR.abs_scale_forward(x, b, fu, fd, **kw)
    by, bu = FR.forward_bounds(x, b, fu, fd, y_ref=y64, fp16=fp16, scales=scales, **kw)
    r_y = FR.ratio((e['y'].double() - y64).abs(), by)
    dx64, _ = FR.adjoint_ref(e['dy'], u64, xhw, fu, fd, **kw)
    b32, wid, _ = FR.adjoint_bounds(e['dy'], u64, bu, scales[0], xhw, fu, fd, **kw)
    bdx = b32 + FR._f16_store(dx64, b32) if fp16 else b32
    return r_y, FR.ratio((e['dx'].double() - dx64).abs(), bdx), FR.widened_share(wid)


@pytest.mark.parametrize('scale', [1.0, 2.0 ** -20], ids=['g~1', 'g~1e-6'])
@pytest.mark.parametrize('cfg', ['T', 'R'])
def test_whole_mixed_precision_backward_layer_by_layer_and_end_to_end(cfg, scale):
    """`synthesis(ws)` with the default options under autograd at batch 2, on sum(image * g): g ~ N(0, 1), and g * 2^-20 -- the size of
    a mean-reduced CLIP / ID gradient on a 1024^2 image.  The 64-pixel mini configurations have no fp32 layer with the default
    num_fp16_res (every sampling rate is above 64 / 16), so the network is MIXED: 256 pixels, 32 channels, layers 0 - 2 fp32, 3 - 14 fp16.

    Every layer's recorded calls against float64: the convolution's dx (fp16 layers: `fp16_dgrad_bound` with the unit of max |dy|;
    fp32 layers: `dgrad_bound`) and ds (`wgrad_bound` -> `modgrad_bound` with the layer's input bound and the adjoint's hand-off),
    filtered_lrelu's y and dx (tests/flrelu_ref.py, fp16 store included); the tensors between the calls are the same ones (the cast at
    the fp32 -> fp16 boundary and of the image included).
    End to end: e_hip <= 2 e_composite + 1e-6 max |g64| for d/dws, both against the float64 network (`synthesis_fp64`); the composite
    runs both ops with impl='ref' on the same fp16 layers, on the GPU (its convolutions on torch's own im2col + GEMM path).

    Measured on one MI355X (e relative to max |g64|; zero shares: fp16 dx entries of the convolutions, all fp16 layers together):
        T  g ~ 1     e_hip 8.58e-03  e_composite 9.68e-03   zero fp16 dx: hip 0.019 composite 0.019   zero d/dws: 0 | 0
        T  g ~ 1e-6  e_hip 3.00e-01  e_composite 7.63e-01   zero fp16 dx: hip 0.570 composite 0.747   zero d/dws: 0 | 0.56
        R  g ~ 1     e_hip 9.73e-03  e_composite 1.32e-02   zero fp16 dx: hip 0.038 composite 0.038   zero d/dws: 0 | 0
        R  g ~ 1e-6  e_hip 3.87e-01  e_composite 7.70e-01   zero fp16 dx: hip 0.671 composite 0.806   zero d/dws: 0 | 0.50
    Per layer, worst err / bound: convolution dx 0.19 (fp16) | 0.18 (fp32) at g ~ 1 and 0.94 at g ~ 1e-6, where every dx lies on the
    subnormal grid and the bound IS that grid; ds 0.007; filtered_lrelu y 0.999 and dx 1.000 (fp16: the store's own half step), 0.14 in fp32.
    At g ~ 1e-6 neither execution is close to float64: the image gradient 0.25 g (2.4e-7: four steps of fp16's subnormal grid) is cast
    to fp16 before the first adjoint, and every fp16 dx after it lives on that grid.  The HIP path loses less than the composite -- its
    convolutions scale dy up by a power of two before rounding it and keep fp32 sums up to the store, so the fp32 layers 0 - 2 still
    receive a gradient, where the composite hands them zeros (zero dx 1.000) -- but a third of the largest d/dws entry is error
    ("The mixed-precision backward against float64")."""
    t0 = time.time()
    G, ws, g1, g64_1, _ = _network_case(cfg)
    g, g64 = g1 * scale, g64_1 * scale
    names = list(G.synthesis.layer_names)
    layers = G.synthesis.layers()
    fp16_layers = [nm for nm, layer in zip(names, layers) if layer.use_fp16]
    assert len(fp16_layers) >= 4 and len(names) - len(fp16_layers) >= 1 and not layers[0].use_fp16 and layers[-1].use_fp16
    hip, img, conv, act = _record_backward(G, ws, g, 'cuda')
    comp, img_c, conv_c, _ = _record_backward(G, ws, g, 'ref')
    torch.cuda.synchronize()
    t1 = time.time()
    failed = {}
    for j, nm in enumerate(names):
        c, a = conv[nm], act[nm]
        want = torch.float16 if nm in fp16_layers else torch.float32
        assert c['x'].dtype == want and a['x'].dtype == want and a['y'].dtype == want, nm
        # the chain: what one call's backward returned is what the call before it received (through the casts at the boundaries)
        assert torch.equal(a['dx'], c['dy']), nm
        after = conv[names[j + 1]]['dx'] if j + 1 < len(names) else g.to(want) * G.synthesis.output_scale
        assert a['dy'].dtype == want and torch.equal(a['dy'], after.to(want)), nm
        r_dx, r_ds, _ = _check_conv(nm, c)
        r_y, r_adx, share = _check_act(a)
        zeros = float((c['dx'] == 0).double().mean())
        print(f'{cfg} g x {scale:.1e} {nm:14s} {"fp16" if want == torch.float16 else "fp32"} |dy| max {float(c["dy"].abs().max()):.2e}  err/bound  conv dx {r_dx:.3f} '
              f'ds {r_ds:.3f}  flrelu y {r_y:.3f} dx {r_adx:.3f} (widened {share:.1e})  zero dx {zeros:.4f} (composite {float((conv_c[nm]["dx"] == 0).double().mean()):.4f})')
        if max(r_dx, r_ds, r_y, r_adx) > 1.0 or share > 1e-3:
            failed[nm] = (r_dx, r_ds, r_y, r_adx, share)
    top = float(g64.abs().max())
    e_hip, e_comp = float((hip.double() - g64).abs().max()), float((comp.double() - g64).abs().max())

    def zero_share(rec):
        return sum(int((rec[nm]['dx'] == 0).sum()) for nm in fp16_layers) / sum(rec[nm]['dx'].numel() for nm in fp16_layers)
    print(f'{cfg} g x {scale:.1e}: d/dws  e_hip {e_hip / top:.3e}  e_composite {e_comp / top:.3e} of max |g64| {top:.3e}  ratio {e_hip / e_comp:.3f}  '
          f'zero entries of d/dws: hip {float((hip == 0).double().mean()):.4f} composite {float((comp == 0).double().mean()):.4f}; '
          f'of the fp16 dx: hip {zero_share(conv):.4f} composite {zero_share(conv_c):.4f}; image hip vs composite {float((img - img_c).abs().max()):.2e}  '
          f'[{t1 - t0:.1f} s runs, {time.time() - t1:.1f} s checks]')
    assert not failed, f'err/bound (conv dx, ds, flrelu y, dx, widened share) outside the model: {failed}'
    assert hip.dtype == torch.float32 and bool(torch.isfinite(hip).all()) and math.isfinite(e_comp) and e_comp > 0
    assert e_hip <= 2 * e_comp + 1e-6 * top, (e_hip, e_comp, top)


# ------------------------------------------------------------------------------------------------ 4. one coach step

class _composite_ops:
    """Inside the block `modulated_conv2d` and `filtered_lrelu` run their composite formulation (impl='ref')."""

    def __enter__(self):
        from torch_utils.ops import filtered_lrelu as fl
        from torch_utils.ops import modulated_conv as mc
        self.orig = orig_mc, orig_fl = mc.modulated_conv2d, fl.filtered_lrelu

        def conv(x, w, s, demodulate=True, padding=0, input_gain=None, impl='cuda', x_bound=None, prepared=None, epilogue=None, align_rows=False):
            return orig_mc(x, w, s, demodulate=demodulate, padding=padding, input_gain=input_gain, impl='ref')

        def act(x, fu=None, fd=None, b=None, up=1, down=1, padding=0, gain=2 ** 0.5, slope=0.2, clamp=None, flip_filter=False, impl='cuda'):
            return orig_fl(x=x, fu=fu, fd=fd, b=b, up=up, down=down, padding=padding, gain=gain, slope=slope, clamp=clamp, flip_filter=flip_filter,
                           impl='ref')
        mc.modulated_conv2d, fl.filtered_lrelu = conv, act

    def __exit__(self, *exc):
        from torch_utils.ops import filtered_lrelu as fl
        from torch_utils.ops import modulated_conv as mc
        mc.modulated_conv2d, fl.filtered_lrelu = self.orig


@pytest.mark.parametrize('cfg', ['Rmini', 'Tmini'])
def test_coach_one_step_on_a_mixed_precision_decoder(cfg, tmp_path):
    """`test_coach_one_step_gradients_equal_the_composite_mappers` with the decoder built with its default fp16 layers (all 15 at 64
    pixels), and a yardstick instead of a shared decoder: the step with HIP mapper and HIP decoder, and the step with the composite
    mapper AND the composite decoder (impl='ref' for both ops on the same fp16 layers), each against the mapper gradients of the
    least-rounded run there is -- composite mapper, all-fp32 decoder (num_fp16_res=0) on the HIP ops; float64 through the CLIP tower
    and the resampler is not built for this size.  Per tensor: e_hip <= 2 e_composite + 1e-6 max |g_ref|.
    Measured on one MI355X over the 24 mapper tensors (gradients of 1e-8 .. 6e-7): e_hip 0.2 - 4.7 % of the largest entry on Rmini,
    0.2 - 1.0 % on Tmini; e_composite 1.5 - 29 % and 0.6 - 5.9 %; e_hip / e_composite 0.14 - 0.39 and 0.09 - 0.31."""
    import mapper_cases as cases
    import test_gpu_styleclip_mapper_train as mt
    from helpers import build_product_generator
    coach, _ = mt._coach(cfg, tmp_path, 1)
    fp32_decoder = coach.net.decoder
    mixed_decoder = build_product_generator(cfg, device=DEV)
    assert sum(layer.use_fp16 for layer in mixed_decoder.synthesis.layers()) >= 4 and not any(layer.use_fp16 for layer in fp32_decoder.synthesis.layers())
    w = torch.from_numpy(cases.latents(2)).to(DEV)

    def step(decoder, train, composite):
        coach.net.decoder = decoder
        coach.net.mapper.train(train)
        coach.optimizer.zero_grad(set_to_none=True)
        with torch.no_grad():
            x = decoder.synthesis(w)
        with (_composite_ops() if composite else contextlib.nullcontext()), torch.backends.cudnn.flags(enabled=not composite):
            w_hat = coach.edit(w)
            loss, _ = coach.calc_loss(w, x, w_hat, decoder.synthesis(w_hat))
            loss.backward()
        assert all(p.grad is None for p in decoder.parameters())
        return {k: p.grad.detach().double().clone() for k, p in coach.net.mapper.named_parameters()}

    ref = step(fp32_decoder, False, False)
    hip = step(mixed_decoder, True, False)
    comp = step(mixed_decoder, False, True)
    worst = 0.0
    for k, g in ref.items():
        top = float(g.abs().max())
        e_hip, e_comp = float((hip[k] - g).abs().max()), float((comp[k] - g).abs().max())
        worst = max(worst, e_hip / (2 * e_comp + 1e-6 * top))
        print(f'{cfg} {k:28s} max |g_ref| {top:.3e}  e_hip {e_hip / top:.3e}  e_composite {e_comp / top:.3e}  ratio {e_hip / max(e_comp, 1e-300):.3f}')
        assert top > 0 and e_hip <= 2 * e_comp + 1e-6 * top, (k, e_hip, e_comp, top)
    print(f'{cfg}: largest e_hip / (2 e_composite + 1e-6 max |g_ref|) = {worst:.3f}')
