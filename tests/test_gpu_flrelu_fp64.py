"""GPU: filtered_lrelu forward and adjoint at the full 1024^2 layer shapes against float64, element by element, under the error
model of tests/flrelu_ref.py.

a. One real pivotal-tuning step (force_fp32, MSE) with every filtered_lrelu call recorded: y, sign codes, dx, db and the max |dx|
   hand-off of all 15 layers; the training forward against the plain forward of the same inputs.
b. Boundary probes of the work decomposition (sg3_filtered_lrelu_stream_grid) at the real plane counts of batch 1 and 4: inputs
   that are zero except around every chunk and strip boundary, the per-workgroup partial sums slot by slot.
c. Magnitudes (2^-20 .. 300 forward, 2^-24 .. 2^10 adjoint) in fp32 and fp16 I/O, with the kernel form proven per call.

The reference is computed a few planes at a time (`_plane_step`) to bound the float64 work.
"""
import ctypes
import functools
import math
import time

import numpy as np
import pytest
import torch

import flrelu_ref as R
from flrelu_record import record_step, setup_kwargs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _plane_step(n, u_hw, budget=3.0e7):
    """channels per reference pass: n * channels * upsampled plane <= budget elements (0.24 GB per float64 temporary)."""
    return max(1, int(budget // (n * u_hw[0] * u_hw[1])))


def _u_hw(kw, x_hw, fu):
    px0, px1, py0, py1 = R._four(kw['padding'])
    fuh = 1 if fu is None else int(fu.shape[0]); fuw = 1 if fu is None else int(fu.shape[-1])
    return (x_hw[0] * kw['up'] + py0 + py1 - (fuh - 1), x_hw[1] * kw['up'] + px0 + px1 - (fuw - 1))


def _active_hw(y_hw, fd, down):
    fdh = 1 if fd is None else int(fd.shape[0]); fdw = 1 if fd is None else int(fd.shape[-1])
    return (y_hw[0] * down - (down - 1) + fdh - 1, y_hw[1] * down - (down - 1) + fdw - 1)


class _Worst(dict):
    def up(self, key, v):
        self[key] = max(self.get(key, 0.0), v)


def _check_planes(x, b, fu, fd, kw, y=None, signs=None, dy=None, dx=None, db=None, acc_terms=None, fp16=False, worst=None, partial=None,
                  grid=None, sign_offsets=(0, 0)):
    """One group of channels against float64: every quantity given.  Returns the widening of this group (or None)."""
    xhw = tuple(x.shape[2:])
    y64, u64 = R.forward_ref(x, b, fu, fd, **kw)
    scales = R.abs_scale_forward(x, b, fu, fd, **kw)
    su = scales[0]
    by, bu = R.forward_bounds(x, b, fu, fd, y_ref=y64, fp16=fp16, scales=scales, **kw)
    if y is not None:
        worst.up('y', R.ratio((y.to(torch.float64) - y64).abs(), by))
    at0, atc = R.ambiguous(u64, bu, su, kw['gain'], kw['slope'], kw['clamp'])
    if signs is not None:
        bad = R.sign_mismatches(signs, sign_offsets[0], sign_offsets[1], u64, at0 | atc, kw['gain'], kw['slope'], kw['clamp'],
                                active_hw=_active_hw(tuple(y64.shape[2:]), fd, kw['down']))
        worst.up('sign mismatches', float(bad))
        worst.up('ambiguous share', float((at0 | atc).to(torch.float64).mean()))
    wid = None
    if dy is not None:
        dx64, db64 = R.adjoint_ref(dy, u64, xhw, fu, fd, **kw)
        b32, wid, _ = R.adjoint_bounds(dy, u64, bu, su, xhw, fu, fd, **kw)
        bdx = b32 + R._f16_store(dx64, b32) if fp16 else b32
        worst.up('dx', R.ratio((dx.to(torch.float64) - dx64).abs(), bdx))
        if db is not None:
            # the kernel sums its fp32 dx before the store: the element bounds without the fp16 store
            bdb = R.db_bound(b32, dx64, acc_terms)
            if fp16:
                bdb = bdb + R._f16_store(db64, bdb)
            worst.up('db', R.ratio((db.to(torch.float64) - db64).abs(), bdb))
        if partial is not None:
            # slot (chunk, strip) of the adjoint launch = the sum of dx over that window of the plane
            ns, tw, _, nc, ch = grid
            for k in range(nc):
                for s in range(ns):
                    win = (slice(None), slice(None), slice(k * ch, min((k + 1) * ch, xhw[0])), slice(s * tw, min((s + 1) * tw, xhw[1])))
                    ref = dx64[win].sum([2, 3])
                    bnd = b32[win].sum([2, 3])
                    bnd = bnd + (ch + 7) * R.U * R.SECOND * (dx64[win].abs().sum([2, 3]) + bnd)
                    worst.up('partial', R.ratio((partial[:, :, k * ns + s].to(torch.float64) - ref).abs(), bnd))
    return wid


# ---------------------------------------------------------------------------------------------------- a. one real PTI step

# batch 4 changes the chunk heights of L9 - L13 (T) and L5 - L13 (R: 69 .. 348 rows) and of their adjoints
STEP_CASES = [('T1024', 1), ('R1024', 1), ('T1024', 4), ('R1024', 4)]

def _record(cfg, n):
    from torch_utils import _hip_plugins as hp
    hp.stream_call_log = []
    try:
        names, rec = record_step(cfg, n, DEV)
        log = hp.stream_call_log
    finally:
        hp.stream_call_log = None
    return names, rec, log


@pytest.mark.parametrize('cfg,n', STEP_CASES)
def test_full_size_step_every_layer_matches_fp64(cfg, n):
    """y, sign codes, dx, db and max |dx| of every filtered_lrelu call of one real full-size PTI step against float64."""
    from torch_utils.ops import known_amax
    t0 = time.time()
    names, rec, log = _record(cfg, n)
    adj_grid = {}
    for entry in log:
        if entry['read'] and entry['grid'] is not None:
            adj_grid[(entry['shape'], entry['down'])] = entry['grid']       # the adjoint's down factor is the layer's up factor
    failed, shares = {}, {}
    for nm in names:
        e = rec.pop(nm)
        kw = setup_kwargs(e)
        x, b, fu, fd = e['x'], e['b'], e['fu'], e['fd']
        c = int(x.shape[1])
        u_hw = _u_hw(kw, tuple(x.shape[2:]), fu)
        # max |dx| handed to the convolution gradients: the maximum of what was stored, bit for bit
        known = known_amax.lookup(e['dx'])
        grid = adj_grid.get((tuple(e['dx'].shape), kw['up']))
        torgb = nm.startswith('L14')
        assert torgb or (grid is not None and known is not None and e['signs'] is not None), f'{nm}: the adjoint did not take the fused kernel'
        if known is not None:
            assert float(known) == float(e['dx'].abs().max()), (nm, float(known), float(e['dx'].abs().max()))
        acc = None if grid is None else grid[4] + 7 + grid[0] * grid[3] * n
        worst, wid_count, total = _Worst(), 0, 0
        step = _plane_step(n, u_hw)
        for c0 in range(0, c, step):
            sl = slice(c0, min(c0 + step, c))
            wid = _check_planes(x[:, sl], b[sl], fu, fd, kw, y=e['y'][:, sl], signs=None if e['signs'] is None else e['signs'][:, sl],
                                dy=e['dy'][:, sl], dx=e['dx'][:, sl], db=e['db'][sl], acc_terms=acc, worst=worst)
            wid_count += int((wid > 0).sum()); total += wid.numel()
        shares[nm] = wid_count / total
        print(f'{cfg} N={n} {nm:14s} C={c:4d} {x.shape[2]}->{e["y"].shape[2]} up{kw["up"]} adjoint grid {grid}  err/bound  y {worst["y"]:.3f}  '
              f'dx {worst["dx"]:.3f}  db {worst["db"]:.3f}  sign mismatches {int(worst.get("sign mismatches", -1))}  ambiguous {worst.get("ambiguous share", 0):.1e}  '
              f'widened dx share {shares[nm]:.1e}  |dy| max {float(e["dy"].abs().max()):.1e}')
        if max(worst['y'], worst['dx'], worst['db']) > 1.0 or worst.get('sign mismatches', 0) > 0 or shares[nm] > 1e-3:
            failed[nm] = dict(worst, share=shares[nm])
        del e, x, b
    torch.cuda.synchronize()
    print(f'{cfg} N={n}: {time.time() - t0:.1f} s')
    assert not failed, f'outside the model: {failed}'


@pytest.mark.parametrize('cfg,n', STEP_CASES)
def test_training_forward_is_bit_identical_to_the_plain_forward(cfg, n):
    """The sign-writing forward's y of every layer of the step equals the plain forward of the same inputs bit for bit: the
    sign codes are decided in the reference's order (gain, lrelu, clamp), the output values are formed as the plain forward forms
    them (gain once per output sample)."""
    from torch_utils.ops import filtered_lrelu as fl
    names, rec, _ = _record(cfg, n)
    differs = {}
    for nm in names:
        e = rec.pop(nm)
        kw = setup_kwargs(e)
        with torch.no_grad():
            y_plain = fl.filtered_lrelu(e['x'], fu=e['fu'], fd=e['fd'], b=e['b'], up=kw['up'], down=kw['down'], padding=kw['padding'],
                                        gain=kw['gain'], slope=kw['slope'], clamp=kw['clamp'])
        if not torch.equal(y_plain, e['y']):
            differs[nm] = float((y_plain - e['y']).abs().max())
        del e, y_plain
    print(f'{cfg} N={n}: training forward != plain forward, max |diff| per layer: {differs}')
    assert not differs, f'training forward != plain forward, max |diff| per layer: {differs}'


# ------------------------------------------------------------------------------------------- layers at their real geometry

@functools.lru_cache(maxsize=None)
def _layers(cfg):
    """{Lk: (channels, x side, call arguments, fu, fd)} of a full-size generator (filters as the product designs them)."""
    from helpers import build_product_generator
    G = build_product_generator(cfg)
    out = {}
    for name in G.synthesis.layer_names:
        L = getattr(G.synthesis, name)
        if not L.is_torgb:
            kw = dict(up=int(L.up_factor), down=int(L.down_factor), padding=[int(v) for v in L.padding], gain=float(np.sqrt(2)), slope=0.2,
                      clamp=L.conv_clamp, flip=False)                      # as SynthesisLayer.forward calls the op
            out[name.split('_')[0]] = (int(L.out_channels), int(L.in_size[0]) + L.conv_kernel - 1, kw, L.up_filter.to(DEV), L.down_filter.to(DEV))
    return out


def _grid(n, c, x_hw, fu, fd, up, down, pads, read=False, write=False):
    """(nStrips, stripW, nFullStrips, nChunks, chunkRows) of a call on dense fp32 planes, and its output size: the host-only query
    sg3_filtered_lrelu_stream_grid on a parameter block filled as the binding fills it (no data pointer is followed)."""
    from torch_utils import _sg3abi as abi
    lib = abi.load()
    fuw, fuh = int(fu.shape[-1]), (int(fu.shape[0]) if fu.ndim == 2 else 0)
    fdw, fdh = int(fd.shape[-1]), (int(fd.shape[0]) if fd.ndim == 2 else 0)
    out = [ctypes.c_int() for _ in range(5)]
    abi.check(lib.sg3_filtered_lrelu_shape(x_hw[0], x_hw[1], up, down, fuw, fuh, fdw, fdh, *pads, *[ctypes.byref(o) for o in out]), 'sg3_filtered_lrelu_shape')
    from torch_utils._hip_plugins import dense_strides, filtered_lrelu_params
    yh, yw = out[0].value, out[1].value
    p = filtered_lrelu_params(abi.SG3_F32, (n, c, x_hw[0], x_hw[1]), (yh, yw), dense_strides(n, c, x_hw[0], x_hw[1]), dense_strides(n, c, yh, yw), up, down,
                              (fuw, fuh), (fdw, fdh), pads[0], pads[2], 1.0, 0.2, 256.0, False, write_signs=write, read_signs=read, s_hw=(1, 1),
                              fu=abi.ptr(fu), fd=abi.ptr(fd), x=None, y=None, b=None)         # non-null placeholder for the signs
    g = [ctypes.c_int() for _ in range(5)]
    assert lib.sg3_filtered_lrelu_stream_grid(ctypes.byref(p), *[ctypes.byref(v) for v in g]) == 1
    return tuple(v.value for v in g), (p.yH, p.yW)


def _adjoint_setup(x_hw, y_hw, fu, fd, kw):
    from torch_utils.ops import filtered_lrelu as fl
    cfg = fl._setup(kw['up'], kw['down'], kw['padding'], kw['gain'], kw['slope'], kw['clamp'], kw['flip'])
    return fl._adjoint(cfg, fu, fd, x_hw, y_hw, 0, 0)


def _forward(x, b, fu, fd, kw, write_signs):
    """(y, signs, log entry) of one call of the binding."""
    from torch_utils import _hip_plugins as hp
    from torch_utils.ops import filtered_lrelu as fl
    fl._init()
    hp.stream_call_log = []
    try:
        y, so, rc = fl._plugin.filtered_lrelu(x, fu, fd, b, torch.empty(0), kw['up'], kw['down'], *R._four(kw['padding']), 0, 0, kw['gain'],
                                              kw['slope'], math.inf if kw['clamp'] is None else kw['clamp'], kw['flip'], write_signs)
        entry = hp.stream_call_log[0]
    finally:
        hp.stream_call_log = None
    assert rc == 0
    return y, so, entry


def _adjoint(dy, signs, x_hw, fu, fd, kw):
    """(dx, db, max |dx|, log entry) of the fused adjoint call as `_FusedFlrelu.backward` makes it."""
    from torch_utils import _hip_plugins as hp
    from torch_utils.ops import filtered_lrelu as fl
    adj, sx, sy = _adjoint_setup(x_hw, tuple(dy.shape[2:]), fu, fd, kw)
    zero_b = torch.zeros([dy.shape[1]], dtype=dy.dtype, device=dy.device)
    hp.stream_call_log = []
    try:
        res = fl._plugin.filtered_lrelu(dy, fd, fu, zero_b, signs, adj.up, adj.down, adj.px0, adj.px1, adj.py0, adj.py1, sx, sy, adj.gain, adj.slope,
                                        adj.clamp, adj.flip, False, return_sum=True, return_amax=True)
        entry = hp.stream_call_log[0]
    finally:
        hp.stream_call_log = None
    assert res[2] == 0 and res[4] is not None
    return res[0], res[3], res[4], entry


def _near(extent, cuts, width=2):
    """indices within `width` of every cut (on both sides) and of the middle, and the first and last `width`."""
    keep = set(range(min(width, extent))) | set(range(max(0, extent - width), extent))
    for c in list(cuts) + [extent // 2]:
        keep |= {v for v in range(c - width, c + width) if 0 <= v < extent}
    return torch.tensor(sorted(keep), device=DEV)


def _cuts(grid):
    ns, tw, nfull, nc, ch = grid
    return [k * ch for k in range(1, nc)], [s * tw for s in range(1, ns)]


def _probe(shape, rows, cols, gen, scale):
    """randn * scale on the given rows (all columns) and columns (all rows), zero elsewhere."""
    t = torch.zeros(shape, dtype=torch.float32, device=DEV)
    t[:, :, rows] = torch.randn([shape[0], shape[1], len(rows), shape[3]], device=DEV, generator=gen) * scale
    t[:, :, :, cols] = torch.randn([shape[0], shape[1], shape[2], len(cols)], device=DEV, generator=gen) * scale
    return t


def _channel_subset(c):
    return sorted({0, 1, c // 2, c - 2, c - 1} & set(range(c)))


PROBES = [('T1024', nm) for nm in ('L2', 'L5', 'L6', 'L9', 'L10', 'L13')] + [('R1024', nm) for nm in ('L5', 'L6', 'L10')]


@pytest.mark.parametrize('cfg,layer', PROBES)
def test_chunk_and_strip_boundaries_at_real_plane_counts(cfg, layer):
    """Forward (plain and sign-writing), adjoint, db, its partial sums slot by slot and max |dx| on inputs that are zero except
    around every chunk and strip boundary of the launch, at the layer's real N * C for batch 1 and 4."""
    c, side, kw, fu, fd = _layers(cfg)[layer]
    up, pads = kw['up'], R._four(kw['padding'])
    for n in (1, 4):
        t0 = time.time()
        gen = torch.Generator(device=DEV).manual_seed(100 * n + side)
        b0 = torch.zeros([c], device=DEV)
        worst, fwd = _Worst(), []
        sub = _channel_subset(c)
        for write in (False, True):
            # input rows / columns that feed the output rows / columns around the cuts of this launch
            grid, (yh, yw) = _grid(n, c, (side, side), fu, fd, up, kw['down'], pads, write=write)
            rc, cc = _cuts(grid)
            to_in = lambda v: int(round(v * 2 / up + (side * up - yh * 2) / (2 * up)))       # noqa: E731  (centre-aligned resampling)
            xs = _probe([n, c, side, side], _near(side, [to_in(v) for v in rc], 2), _near(side, [to_in(v) for v in cc], 2), gen, 3.0)
            y, so, ent = _forward(xs, b0, fu, fd, kw, write)
            assert ent['grid'] == grid                                  # the launch was cut as the query said
            for ch in sub:
                w2 = _Worst()
                _check_planes(xs[:, ch:ch + 1], b0[ch:ch + 1], fu, fd, kw, y=y[:, ch:ch + 1], signs=so[:, ch:ch + 1] if write else None, worst=w2)
                worst.up('y write' if write else 'y plain', w2['y'])
                if write:
                    worst.up('sign mismatches', w2['sign mismatches'])
            fwd.append((ent['grid'], ent['planes_per_wave']))
        # the adjoint: signs of a dense forward, dy around the cuts of the adjoint's own grid
        xd = torch.randn([n, c, side, side], device=DEV, generator=gen) * 2
        bd = torch.randn([c], device=DEV, generator=gen)
        _, signs, _ = _forward(xd, bd, fu, fd, kw, True)
        adj, _, _ = _adjoint_setup((side, side), (yh, yw), fu, fd, kw)
        grid_a, _ = _grid(n, c, (yh, yw), fd, fu, adj.up, adj.down, (adj.px0, adj.px1, adj.py0, adj.py1), read=True)
        rc, cc = _cuts(grid_a)
        to_out = lambda v: int(round((v - (side * up - yh * 2) / (2 * up)) * up / 2))      # noqa: E731
        dy = _probe([n, c, yh, yw], _near(yh, [to_out(v) for v in rc], 2), _near(yw, [to_out(v) for v in cc], 2), gen, 1e-6)
        dx, db, amax, ent_a = _adjoint(dy, signs, (side, side), fu, fd, kw)
        assert float(amax) == float(dx.abs().max())
        g = ent_a['grid']
        assert g == grid_a and ent_a['partial'].shape[2] == g[0] * g[3]
        for ch in sub:
            _check_planes(xd[:, ch:ch + 1], bd[ch:ch + 1], fu, fd, kw, dy=dy[:, ch:ch + 1], dx=dx[:, ch:ch + 1], db=db[ch:ch + 1],
                          acc_terms=g[4] + 7 + g[0] * g[3] * n, worst=worst, partial=ent_a['partial'][:, ch:ch + 1], grid=g)
        print(f'{cfg} {layer} N={n} C={c} {side}->{yh} up{up}: forward (grid, planes per wave) plain {fwd[0]} sign-writing {fwd[1]}, adjoint grid {g}; err/bound '
              + '  '.join(f'{k} {v:.3f}' for k, v in sorted(worst.items())) + f'  ({time.time() - t0:.1f} s)')
        assert worst.pop('sign mismatches') == 0
        assert max(worst.values()) <= 1.0, worst
        del xd, xs, y, signs, dy, dx


# ------------------------------------------------------------------------------------------------- c. magnitudes and fp16

# T up 2 and R up 2 (148 columns: a full strip + a two-plane remainder, form 3), T up 4 (52 columns: two planes per wave, form 2)
@pytest.mark.parametrize('cfg,layer,form', [('T1024', 'L6', 3), ('T1024', 'L2', 2), ('R1024', 'L6', 3)])
@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
def test_magnitudes_and_fp16_io(cfg, layer, form, dtype):
    """Forward with inputs scaled by 2^-20, 1, 40 (clamp active) and 300 on the left half of every plane (the redo pass on those
    strips only: inferred from the staged maxima on each half against the kernel's own threshold; the redo pass itself is observed in
    test_gpu_flrelu_fast_activation.py); adjoint with dy scaled by 2^-24, 1, 2^10.  fp16 keeps to the scales inside its normal range (forward 1 .. 300, adjoint 2^-6 .. 2^6)."""
    from torch_utils import _sg3abi as abi
    c, side, kw, fu, fd = _layers(cfg)[layer]
    up = kw['up']
    fp16 = dtype == torch.float16
    gen = torch.Generator(device=DEV).manual_seed(side + 7 * up)
    sub = _channel_subset(c)
    fu_host = fu.cpu().contiguous()
    thr = float(abi.load().sg3_filtered_lrelu_fast_threshold(fu_host.data_ptr(), int(fu_host.shape[0]), up, ctypes.c_float(kw['gain']),
                                                             ctypes.c_float(kw['slope']), ctypes.c_float(kw['clamp'])))
    assert thr > 0
    worst = _Worst()
    base = torch.randn([1, c, side, side], device=DEV, generator=gen)
    bias = torch.randn([c], device=DEV, generator=gen) * 0.5
    for scale in ((1.0, 40.0, 300.0) if fp16 else (2.0 ** -20, 1.0, 40.0, 300.0)):
        x = base * scale
        if scale == 300.0:
            x[..., side // 2:] = base[..., side // 2:]
        x = x.to(dtype); b = (bias * min(scale, 1.0)).to(dtype)
        staged = (x.float() + b.float()[None, :, None, None]).abs()
        if scale == 300.0:      # left strips run the redo pass, the strips on the right do not
            assert float(staged[..., :side // 2 - 8].amax()) > thr and float(staged[..., side // 2 + 8:].amax()) <= thr
        else:
            assert float(staged.amax()) <= thr
        y, _, ent = _forward(x, b, fu, fd, kw, False)
        assert ent['planes_per_wave'] == form, ent                    # which form of the plain forward ran
        for ch in sub:
            w2 = _Worst()
            _check_planes(x[:, ch:ch + 1], b[ch:ch + 1], fu, fd, kw, y=y[:, ch:ch + 1], fp16=fp16, worst=w2)
            worst.up(f'y x{scale:g}', w2['y'])
    # adjoint: the signs of the unit-scale forward
    x = base.to(dtype); b = bias.to(dtype)
    y, signs, _ = _forward(x, b, fu, fd, kw, True)
    gy = torch.randn(y.shape, device=DEV, generator=gen)
    for scale in ((2.0 ** -6, 1.0, 2.0 ** 6) if fp16 else (2.0 ** -24, 1.0, 2.0 ** 10)):      # fp16: db, a sum over the plane, stays finite
        dy = (gy * scale).to(dtype)
        dx, db, amax, ent = _adjoint(dy, signs, (side, side), fu, fd, kw)
        stored = float(dx.float().abs().max())                         # the kernel keeps the fp32 maximum before the store
        assert float(amax) == stored if not fp16 else abs(float(amax) - stored) <= 2.0 ** -11 * stored
        g = ent['grid']
        for ch in sub:
            w2 = _Worst()
            _check_planes(x[:, ch:ch + 1], b[ch:ch + 1], fu, fd, kw, dy=dy[:, ch:ch + 1], dx=dx[:, ch:ch + 1], db=db[ch:ch + 1],
                          acc_terms=g[4] + 7 + g[0] * g[3], fp16=fp16, worst=w2)
            worst.up(f'dx x{scale:g}', w2['dx']); worst.up(f'db x{scale:g}', w2['db'])
    print(f'{cfg} {layer} {str(dtype).split(".")[1]} C={c} {side} up{up} fast threshold {thr:.1f}: err/bound ' + '  '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
