"""CPU: the float64 references and the error model of tests/flrelu_ref.py.

The references against the vectors the real reference produced (golden ops / grads) and against the reference formulation run in
float64 with autograd; the fp32 `impl='ref'` result lies inside the bound; injected faults exceed it by a stated factor; and the
share of dx elements the adjoint's discontinuity widens stays below 1e-3 on the real inputs of a PTI step."""
import math
import warnings

import pytest
import torch

import flrelu_ref as R
from flrelu_record import record_step, setup_kwargs
from golden_cases import FLRELU_CASES, FLRELU_GRAD_CASES, make_filter, rand
from helpers import golden, product_design

# separable and 12x12 filters, flip, up 4, negative padding, no clamp, a tight clamp, the adjoint-like up 2 / down 4, 1x1
CASES = ['t_up2_dn2', 't_up4_dn2', 't_crit_l13', 'r_up2_dnrad2', 'r_up4_dnrad2', 'flip', 'asym_noflip', 'no_clamp', 'tight_clamp',
         'nonsquare_neg', 'bwd_like_dn4', 'full_up_2d', 't_torgb', 'no_bias']


def _case(name):
    c = FLRELU_CASES[name]
    x = torch.from_numpy(rand(11, *c['shape']))
    b = torch.from_numpy(rand(12, c['shape'][1])) if c['bias'] else None
    fu, fd = (None if f is None else torch.from_numpy(f) for f in (make_filter(c['fu'], product_design), make_filter(c['fd'], product_design)))
    kw = dict(up=c['up'], down=c['down'], padding=c['padding'], gain=c['gain'], slope=c['slope'], clamp=c['clamp'], flip=c['flip'])
    return x, b, fu, fd, kw


def _product(x, b, fu, fd, kw, dtype=None):
    from torch_utils.ops import filtered_lrelu as fl
    k = dict(kw)
    k['flip_filter'] = k.pop('flip')
    cast = (lambda t: t) if dtype is None else (lambda t: None if t is None else t.to(dtype))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return fl._filtered_lrelu_ref(cast(x), fu=fu, fd=fd, b=cast(b), **k)      # the taps stay fp32 values


@pytest.mark.parametrize('name', sorted(FLRELU_CASES))
def test_reference_matches_the_real_reference_forward(name):
    """forward_ref against the golden vector of every case, within the model's bound for an fp32 computation."""
    x, b, fu, fd, kw = _case(name)
    y, _ = R.forward_ref(x, b, fu, fd, **kw)
    by, _ = R.forward_bounds(x, b, fu, fd, **kw)
    gold = torch.from_numpy(golden('ops')['flrelu/' + name]).to(torch.float64)
    assert tuple(gold.shape) == tuple(y.shape)
    r = R.ratio((gold - y).abs(), by)
    print(f'{name}: golden y err/bound {r:.3f}')
    assert r <= 1.0


@pytest.mark.parametrize('name', FLRELU_GRAD_CASES)
def test_reference_matches_the_real_reference_gradients(name):
    x, b, fu, fd, kw = _case(name)
    y, u = R.forward_ref(x, b, fu, fd, **kw)
    dy = torch.from_numpy(rand(13, *y.shape))
    dx, db = R.adjoint_ref(dy, u, tuple(x.shape[2:]), fu, fd, **kw)
    _, bu = R.forward_bounds(x, b, fu, fd, **kw)
    su, _, _ = R.abs_scale_forward(x, b, fu, fd, **kw)
    bdx, wid, _ = R.adjoint_bounds(dy, u, bu, su, tuple(x.shape[2:]), fu, fd, **kw)
    g = golden('grads')
    r_dx = R.ratio((torch.from_numpy(g[name + '/dx']).to(torch.float64) - dx).abs(), bdx)
    r_db = R.ratio((torch.from_numpy(g[name + '/db']).to(torch.float64) - db).abs(), R.db_bound(bdx, dx))
    print(f'{name}: golden dx err/bound {r_dx:.3f}  db {r_db:.3f}  widened share {R.widened_share(wid):.2e}')
    assert r_dx <= 1.0 and r_db <= 1.0


@pytest.mark.parametrize('name', CASES)
def test_reference_equals_the_float64_formulation_and_bounds_the_fp32_one(name):
    x, b, fu, fd, kw = _case(name)
    x64 = x.to(torch.float64).requires_grad_(True)
    b64 = None if b is None else b.to(torch.float64).requires_grad_(True)
    # the formulation takes gain / slope / clamp as Python floats: hand it the fp32 values the kernels get
    kf = dict(kw, gain=R.f32(kw['gain']), slope=R.f32(kw['slope']), clamp=None if kw['clamp'] is None else R.f32(kw['clamp']))
    y_f = _product(x64, b64, fu, fd, kf, dtype=torch.float64)
    y, u = R.forward_ref(x, b, fu, fd, **kw)
    scale = float(y.abs().max())
    assert float((y - y_f.detach()).abs().max()) <= 1e-12 * scale
    dy = torch.from_numpy(rand(13, *y.shape))
    grads = torch.autograd.grad(y_f, [x64] + ([] if b64 is None else [b64]), dy.to(torch.float64))
    dx, db = R.adjoint_ref(dy, u, tuple(x.shape[2:]), fu, fd, **kw)
    assert float((dx - grads[0]).abs().max()) <= 1e-12 * float(dx.abs().max())
    if b64 is not None:
        assert float((db - grads[1]).abs().max()) <= 1e-11 * float(dx.abs().sum([0, 2, 3]).max())
    # abs scales: the same pipelines on |x + b|, |dy| with |taps|
    su, sy_pre, _ = R.abs_scale_forward(x, b, fu, fd, **kw)
    assert bool((su >= u.abs() * (1 - 1e-12)).all()) and bool((sy_pre >= y.abs() * (1 - 1e-12)).all())
    # fp32 result of the reference formulation inside the bound
    by, bu = R.forward_bounds(x, b, fu, fd, **kw)
    y32 = _product(x, b, fu, fd, kw)
    r = R.ratio((y32.to(torch.float64) - y).abs(), by)
    print(f'{name}: fp32 impl=ref y err/bound {r:.3f}')
    assert r <= 1.0


def test_rounding_counts():
    dev = torch.device('cpu')
    f12, f24 = torch.ones(12), torch.ones(24)
    rad = torch.ones(12, 12)
    sep = R.Ops(40, 40, f12, f12, 2, 2, [9, 8, 9, 8], False, dev)
    assert (sep.n_u(), sep.n_down()) == (13, 20)                       # 13 + 1 + 20 = 34
    up4 = R.Ops(40, 40, f24, f12, 4, 2, [-6, -9, -6, -9], False, dev)
    assert (up4.n_u(), up4.n_down()) == (13, 20)
    r = R.Ops(40, 40, f12, rad, 2, 2, [11, 10, 11, 10], False, dev)
    assert r.fd_mirror and (r.n_u(), r.n_down()) == (13, 39)           # folded: 13 + 1 + 39 = 53
    asym = rad.clone(); asym[0, 0] = 2.0
    assert R.Ops(40, 40, f12, asym, 2, 2, [11, 10, 11, 10], False, dev).n_down() == 74
    x = torch.zeros(1, 1, 40, 40); dy = torch.zeros(1, 1, 40, 40)
    for fu, fd, up, pad, want in ((f12, f12, 2, [9, 8, 9, 8], 33), (f24, f12, 4, [-6, -9, -6, -9], 51), (f12, rad, 2, [11, 10, 11, 10], 57),
                                  (f24, rad, 4, [-2, -5, -2, -5], 75)):
        kw = dict(up=up, down=2, padding=pad, gain=1.0, slope=0.2, clamp=None, flip=False)
        y, u = R.forward_ref(x, None, fu, fd, **kw)
        _, _, n_adj = R.adjoint_bounds(torch.zeros_like(y), u, torch.zeros_like(u), torch.zeros_like(u), (40, 40), fu, fd, **kw)
        assert n_adj == want


def test_sign_decoder_round_trip():
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 3, [2, 3, 21, 37], generator=g, dtype=torch.uint8)
    sx, sy, sh, swb = 5, 2, 26, 12
    full = torch.zeros([2, 3, sh, swb * 4], dtype=torch.uint8)
    full[:, :, sy:sy + 21, sx:sx + 37] = codes
    packed = sum(full[..., q::4] << (2 * q) for q in range(4)).to(torch.uint8)
    assert torch.equal(R.decode_signs(packed, sx, sy, (21, 37)), codes)
    # negative offsets: the part of the buffer outside the tensor decodes to 255
    d = R.decode_signs(packed, -3, -1, (21, 37))
    assert torch.equal(d[:, :, 1:, 3:], full[:, :, :20, :34]) and bool((d[:, :, 0] == 255).all()) and bool((d[..., :3] == 255).all())


# ------------------------------------------------------------------------------------------------------------ injected faults

def _fault_setup(name):
    x, b, fu, fd, kw = _case(name)
    y, u = R.forward_ref(x, b, fu, fd, **kw)
    by, bu = R.forward_bounds(x, b, fu, fd, **kw)
    su, _, _ = R.abs_scale_forward(x, b, fu, fd, **kw)
    dy = torch.from_numpy(rand(13, *y.shape)) * 1e-7             # the magnitude of an MSE gradient over 3 x 1024^2 pixels
    dx, db = R.adjoint_ref(dy, u, tuple(x.shape[2:]), fu, fd, **kw)
    bdx, wid, _ = R.adjoint_bounds(dy, u, bu, su, tuple(x.shape[2:]), fu, fd, **kw)
    return dict(x=x, b=b, fu=fu, fd=fd, kw=kw, y=y, u=u, by=by, bu=bu, su=su, dy=dy, dx=dx, db=db, bdx=bdx, wid=wid)


def _fault_ratio(err, bound):
    """max err / bound; an error where the bound is zero counts as infinite."""
    if bool(((bound <= 0) & (err > 0)).any()):
        return math.inf
    return float((err / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize('name', ['t_up2_dn2', 't_up4_dn2', 'r_up2_dnrad2'])
def test_injected_faults_exceed_the_bound(name):
    """Each fault against the bound, forward and adjoint: the factors asserted are the floor of what the fault must show."""
    s = _fault_setup(name)
    x, b, fu, fd, kw = s['x'], s['b'], s['fu'], s['fd'], s['kw']
    xhw = tuple(x.shape[2:])
    out = {}
    # 1. one outer tap zeroed (the first tap of the up filter; of the down filter for the adjoint's first pass)
    fu0 = fu.clone(); fu0[0] = 0
    fd0 = fd.clone(); fd0.view(-1)[0 if fd.ndim == 1 else fd.shape[1] // 2] = 0        # 12x12: the largest tap of the outer row
    y_f, _ = R.forward_ref(x, b, fu0, fd, **kw)
    out['tap/y'] = _fault_ratio((y_f - s['y']).abs(), s['by'])
    dx_f, _ = R.adjoint_ref(s['dy'], s['u'], xhw, fu, fd0, **kw)
    out['tap/dx'] = _fault_ratio((dx_f - s['dx']).abs(), s['bdx'])
    # 2. output shifted by one column
    out['shift/y'] = _fault_ratio((torch.roll(s['y'], 1, 3) - s['y']).abs(), s['by'])
    out['shift/dx'] = _fault_ratio((torch.roll(s['dx'], 1, 3) - s['dx']).abs(), s['bdx'])
    # 3. one strip boundary column taken from the neighbouring row
    for key, ref, bnd in (('y', s['y'], s['by']), ('dx', s['dx'], s['bdx'])):
        t = ref.clone()
        col = ref.shape[3] // 2
        t[:, :, 1:, col] = ref[:, :, :-1, col]
        out['column/' + key] = _fault_ratio((t - ref).abs(), bnd)
    # 4. one sign code flipped at a non-ambiguous sample: the multiplier 1 <-> slope there
    at0, atc = R.ambiguous(s['u'], s['bu'], s['su'], kw['gain'], kw['slope'], kw['clamp'])
    n, c = x.shape[:2]
    ops = R.Ops(xhw[0], xhw[1], fu, fd, kw['up'], kw['down'], kw['padding'], kw['flip'], x.device)
    g_up = R.Ops.apply(ops.B, s['dy'].to(torch.float64).reshape(n * c, *s['dy'].shape[2:]), transpose=True).reshape(s['u'].shape)
    cand = (~at0 & ~atc & (s['u'].abs() * R.f32(kw['gain']) < (math.inf if kw['clamp'] is None else kw['clamp'])))
    idx = torch.nonzero(cand & (g_up.abs() >= g_up.abs()[cand].median()))[7]
    delta = torch.zeros_like(s['u'])
    delta[tuple(idx)] = (1.0 - R.f32(kw['slope'])) * R.f32(kw['gain']) * g_up[tuple(idx)]
    d_dx = R.Ops.apply(ops.A, delta.reshape(n * c, *s['u'].shape[2:]), transpose=True).reshape(s['dx'].shape)
    out['sign/dx'] = _fault_ratio(d_dx.abs(), s['bdx'])
    codes = R.sign_codes_ref(s['u'], kw['gain'], kw['slope'], kw['clamp'])
    packed_w = -(-codes.shape[3] // 4) * 4
    full = torch.zeros([n, c, codes.shape[2], packed_w], dtype=torch.uint8)
    full[..., :codes.shape[3]] = codes
    packed = sum(full[..., q::4] << (2 * q) for q in range(4)).to(torch.uint8)
    assert R.sign_mismatches(packed, 0, 0, s['u'], at0 | atc, kw['gain'], kw['slope'], kw['clamp']) == 0
    i = tuple(int(v) for v in idx)
    packed[i[0], i[1], i[2], i[3] // 4] ^= 1 << (2 * (i[3] % 4))
    assert R.sign_mismatches(packed, 0, 0, s['u'], at0 | atc, kw['gain'], kw['slope'], kw['clamp']) == 1
    # 5. a db partial dropped: the sum over a 12-row x 29-column block of one plane, of 2 x 3 = 6 such blocks and more per plane
    part = s['dx'][0, :, :12, :29].sum([1, 2])
    bdb = R.db_bound(s['bdx'], s['dx'], acc_terms=12 + 7 + 9 * x.shape[0])
    out['partial/db'] = float((part.abs() / bdb).max())
    print(name, {k: f'{v:.3g}' for k, v in out.items()})
    floor = {'tap/y': 100, 'tap/dx': 100, 'shift/y': 1e4, 'shift/dx': 1e4, 'column/y': 1e4, 'column/dx': 1e4, 'sign/dx': 1e3, 'partial/db': 30}
    low = {k: v for k, v in out.items() if v < floor[k]}
    assert not low, f'faults too close to the bound (err/bound, floor): { {k: (v, floor[k]) for k, v in low.items()} }'


# ------------------------------------------------------------------------------------------------------- ambiguity share

@pytest.mark.parametrize('cfg', ['Ttiny', 'Rtiny'])
def test_widened_share_on_the_real_inputs_of_a_pti_step(cfg):
    """One force_fp32 MSE step on the CPU (impl='ref'), every layer: the reference formulation's y, dx, db inside the bound and
    the share of dx elements with a widened bound at most 1e-3."""
    names, rec = record_step(cfg, 2, 'cpu', impl='ref')
    worst = 0.0
    for nm in names:
        e = rec[nm]
        kw = setup_kwargs(e)
        x, b, fu, fd = e['x'], e['b'], e['fu'], e['fd']
        xhw = tuple(x.shape[2:])
        y, u = R.forward_ref(x, b, fu, fd, **kw)
        by, bu = R.forward_bounds(x, b, fu, fd, **kw)
        su, _, _ = R.abs_scale_forward(x, b, fu, fd, **kw)
        dx, db = R.adjoint_ref(e['dy'], u, xhw, fu, fd, **kw)
        bdx, wid, _ = R.adjoint_bounds(e['dy'], u, bu, su, xhw, fu, fd, **kw)
        share = R.widened_share(wid)
        worst = max(worst, share)
        r_y = R.ratio((e['y'].to(torch.float64) - y).abs(), by)
        r_dx = R.ratio((e['dx'].to(torch.float64) - dx).abs(), bdx)
        r_db = R.ratio((e['db'].to(torch.float64) - db).abs(), R.db_bound(bdx, dx))
        print(f'{cfg} {nm:12s} |dy| max {float(e["dy"].abs().max()):.2e}  y {r_y:.3f}  dx {r_dx:.3f}  db {r_db:.3f}  widened share {share:.2e}')
        assert share <= 1e-3, (nm, share)
        assert max(r_y, r_dx, r_db) <= 1.0, (nm, r_y, r_dx, r_db)
    print(f'{cfg}: worst widened share {worst:.2e}')
