"""Run one row of modconv_variant_cases through the C ABI: sg3_modulated_conv2d_prep + sg3_modulated_conv2d with the row's OWN
precision code and tensor type.  Nothing here goes through torch_utils.ops.modulated_conv._choose_form, which pairs fp32 tensors
with the split arithmetic and fp16 tensors with the single-product one and so never reaches the crossed kernels.

`measure(e)` is what tests/test_gpu_modconv_variants.py asserts on (check()); run as a program it measures the M16 = 0 rows, whose
knob is read once per process, and prints the figures as one JSON line:

    SG3_CONV1_MFMA32=1 python tests/modconv_abi.py m16
"""
import ctypes
import functools
import json
import os
import sys

import numpy as np

import modconv_variant_cases as mv

X_BOUND = 256.0
GAIN = 0.8
GUARD = 1024                      # sentinel elements on either side of the output buffer
DEV = 'cuda:0'


def _rand(seed, *shape):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


def _shape_key(e):
    return tuple(e[n] for n in ('N', 'I', 'O', 'H', 'W', 'k', 'pad', 'demodulate'))


@functools.lru_cache(maxsize=None)
def _inputs(key):
    n, i, o, h, w, k, pad, demod = key
    x = np.clip(_rand(91, n, i, h, w) * 20, -256, 256).astype(np.float16).astype(np.float32)       # fp16-representable
    wt = _rand(92, o, i, k, k)
    s = _rand(93, n, i) + 1
    if not demod:
        s = (s * 1000).astype(np.float32)           # |x s| beyond fp16 without the per-sample power-of-two rescale
    return x, wt, s


def inputs(e):
    """(x, w, s) of a row as float32 numpy arrays; x holds fp16-representable values, so both tensor types carry the same numbers."""
    return _inputs(_shape_key(e))


@functools.lru_cache(maxsize=None)
def _reference(key):
    import torch
    from torch_utils.ops import modulated_conv as mc
    x, w, s = (torch.from_numpy(a).double() for a in _inputs(key))
    demod, pad = bool(key[7]), key[6]
    with torch.no_grad():
        ref = mc._composite(x, w, s, demod, pad, torch.tensor(GAIN, dtype=torch.float64) if demod else None)
    return ref, max(1.0, float(ref.abs().max()))


def reference(e):
    """(float64 result on the CPU, scale = max(1, max |ref|)): computed once per shape, shared by every row of that shape."""
    return _reference(_shape_key(e))


def run(e, offer_scratch=True):
    """prep + convolution of row `e` on the GPU.  Returns (out [N,O,outH,outW] in the row's tensor type, the plan the device reports:
    sg3_modconv_dispatch(..., cus=0) on exactly the parameter block that is launched)."""
    import torch
    from torch_utils import _sg3abi as abi
    lib = abi.load()
    x, w, s = (torch.from_numpy(a).to(DEV) for a in inputs(e))
    dtype = (torch.float32, torch.float16)[e['dtype']]
    x = x.to(dtype).contiguous()
    n, ci, co, h, wd, k, pad, prec = (e[c] for c in ('N', 'I', 'O', 'H', 'W', 'k', 'pad', 'precision'))
    oh, ow = mv.out_hw(e)
    wn = torch.empty([int(lib.sg3_modconv_packed_floats(co, ci, k, prec))], dtype=torch.float32, device=DEV)
    wsq = torch.empty([co, ci], dtype=torch.float32, device=DEV)
    s_in = torch.empty([n, ci], dtype=torch.float32, device=DEV)
    dcoef = torch.empty([n, co], dtype=torch.float32, device=DEV) if e['dcoef'] else None
    gain = torch.full([1], GAIN, dtype=torch.float32, device=DEV) if e['demodulate'] else None
    pp = abi.ModconvPrepParams()
    pp.w, pp.s, pp.wPacked, pp.wsq, pp.sIn, pp.dcoef = abi.ptr(w), abi.ptr(s), abi.ptr(wn), abi.ptr(wsq), abi.ptr(s_in), abi.ptr(dcoef)
    pp.inputGain, pp.inputGainMode = abi.ptr(gain), (1 if gain is not None else 0)
    pp.N, pp.I, pp.O, pp.k, pp.demodulate, pp.precision = n, ci, co, k, int(e['demodulate']), prec
    pp.xBound = X_BOUND if prec != mv.CONV_FP32 else 0.0
    pp.xBoundDev, pp.reuseWeights = None, 0
    # the output sits between two runs of a sentinel no result can equal: a store outside the tensor shows
    numel = n * co * oh * ow
    buf = torch.full([GUARD + numel + GUARD], -12288.0, dtype=dtype, device=DEV)
    out = buf[GUARD:GUARD + numel].view(n, co, oh, ow)
    assert out.data_ptr() % 16 == 0
    cp = abi.ModconvParams()
    cp.x, cp.wPacked, cp.sIn, cp.dcoef, cp.out = abi.ptr(x), abi.ptr(wn), abi.ptr(s_in), abi.ptr(dcoef), abi.ptr(out)
    cp.dtype = e['dtype']
    cp.N, cp.I, cp.O, cp.H, cp.W, cp.k, cp.pad = n, ci, co, h, wd, k, pad
    cp.precision, cp.outRowStride = prec, e['outRowStride']
    info = abi.ModconvDispatchInfo()
    stream = abi.stream_ptr(torch.device(DEV))
    prev = lib.sg3_modconv_f23_force_rows(e['forcedRows'])
    try:
        with torch.cuda.device(DEV):
            abi.check(lib.sg3_modulated_conv2d_prep(ctypes.byref(pp), stream), 'sg3_modulated_conv2d_prep')
            if e['scratch'] and offer_scratch:
                need = int(lib.sg3_modconv_split_scratch_floats(ctypes.byref(cp)))       # 0: this call does not split (the plan tells)
                if need > 0:
                    scratch = torch.empty([need], dtype=torch.float32, device=DEV)
                    cp.splitScratch, cp.splitScratchFloats = abi.ptr(scratch), need
            abi.check(lib.sg3_modconv_dispatch(ctypes.byref(cp), 0, ctypes.byref(info)), 'sg3_modconv_dispatch')
            abi.check(lib.sg3_modulated_conv2d(ctypes.byref(cp), stream), 'sg3_modulated_conv2d')
            torch.cuda.synchronize()
    finally:
        lib.sg3_modconv_f23_force_rows(prev)
    assert bool((buf[:GUARD] == -12288.0).all()) and bool((buf[GUARD + numel:] == -12288.0).all()), 'store outside the output tensor'
    return out, {name: getattr(info, name) for name, _ in info._fields_}


def single_product(e):
    """One fp16 product per operand pair (SPLIT = 0 of the direct forms, SG3_CONV_F16_F23): the operands are rounded to fp16 once."""
    v = e['variant']
    return (v[2] in (mv.ROWS, mv.FLAT, mv.GEMM1) and v[7] == 0) or e['precision'] == mv.CONV_F16_F23


def bounds(e):
    """(max, mean or None) of |out - ref| / scale a row must keep: the bounds tests/test_gpu_ops.py holds for the same arithmetic."""
    if single_product(e):
        return 4e-3, 4e-4                           # test_modulated_conv2d_fp16_form
    if e['dtype'] == 0:
        return 5e-6, None                           # test_modulated_conv2d_split_precision: exact or split products, fp32 output
    return 1e-3, None                               # test_modulated_conv2d_fp16_form, exact products: the fp16 rounding of the output


def has_sibling(e):
    """Crossed rows are run on the other tensor type too -- but for the K-split rows of the 1x1 GEMM: the plan splits K for fp32 tensors
    only, so there the two tensor types add in different orders (their unsplit variant rows are compared)."""
    return mv.crossed(e['variant']) and not (e['kind'] == 'ksplit' and e['variant'][2] == mv.GEMM1)


def _ulp16(t):
    """fp16 unit in the last place at |t| (float32 tensor)."""
    import torch
    return torch.exp2(torch.floor(torch.log2(t.abs().clamp(min=2.0 ** -14))) - 10)


def _near_ties(half, full):
    """(elements where half != full.to(float16), those of them that are NOT explained by one rounding against two, largest distance
    of `full` from the fp16 rounding boundary at a mismatch in fp32 ulps).

    The kernels store `(_Float16)(acc * d)`.  Where hipcc contracts product and conversion into one v_fma_mixlo_f16 the exact product
    p = acc d is rounded to fp16 ONCE; the fp32 tensor holds f = fp32(p) and f.to(float16) rounds a second time.  The two differ only
    where p and f lie on different sides of the midpoint m of two neighbouring fp16 values: |f - m| <= |f - p| <= half an fp32 ulp
    of f, and the two results are those neighbours."""
    import torch
    c = full.to(torch.float16)
    mis = half != c
    n = int(mis.sum())
    if n == 0:
        return 0, 0, 0.0
    h, cc, f = half[mis].double(), c[mis].double(), full[mis].double()
    mid = (h + cc) / 2
    ulp32 = torch.exp2(torch.floor(torch.log2(f.abs().clamp(min=2.0 ** -126))) - 23)
    neighbours = (h - cc).abs() <= _ulp16(torch.maximum(h.abs(), cc.abs()).float()).double()
    dist = (f - mid).abs() / ulp32
    return n, int((~neighbours | (dist > 0.5)).sum()), float(dist.max())


def measure(e):
    """Every figure the GPU test asserts for row `e`, as plain numbers (JSON: the M16 = 0 rows are measured in a child process)."""
    import torch
    out, plan = run(e)
    ref, scale = reference(e)
    got = out.double().cpu()
    err = (got - ref).abs()
    bmax, bmean = bounds(e)
    r = dict(id=e['id'], variant=list(mv.variant_of(e, plan)), kSplits=plan['kSplits'], reduceGrid=plan['reduceGrid'], finite=bool(torch.isfinite(got).all()),
             scale=scale, err_max=float(err.max()) / scale, bound_max=bmax, err_mean=float(err.mean()) / scale, bound_mean=bmean)
    if has_sibling(e):
        sib = mv.sibling(e)
        out2, plan2 = run(sib)
        r['sibling_variant'] = list(mv.variant_of(sib, plan2))
        half, full = (out, out2) if e['dtype'] == 1 else (out2, out)
        r['sibling_mismatches'], r['sibling_unexplained'], r['sibling_tie_distance'] = _near_ties(half, full)
        r['sibling_elements'] = half.numel()
        r['sibling_max_diff'] = float((half.double() - full.double()).abs().max())
    if e['kind'] == 'ksplit':
        plain, plan1 = run(e, offer_scratch=False)
        r['unsplit_kSplits'] = plan1['kSplits']
        d = (out.float() - plain.float()).abs()
        if e['dtype'] == 0:
            r['split_diff'], r['split_bound'] = float(d.max()) / scale, 4e-6          # two fp32 summation orders (test_gpu_ops.py, K-split test)
        else:
            # Both are fp16 roundings of fp32 sums that may differ by the 4e-6 scale above, so they differ by at most that plus one
            # fp16 ulp of the result.  (One ulp of the ELEMENT alone cannot hold where the plane passes through zero: an element of
            # 1e-3 scale has an ulp of 5e-7 scale, the size of the fp32 difference itself -- 2 to 12 such ulps measured.)
            ulp = _ulp16(torch.maximum(out.float().abs(), plain.float().abs()))
            r['split_diff'], r['split_bound'] = float((d / (ulp + 4e-6 * scale)).max()), 1.0
            r['split_own_ulps'] = float((d / ulp).max())
        r['split_differs'] = not torch.equal(out, plain)
    return r


def check(e, r):
    """The assertions on measure(e); prints measured / bound first."""
    line = '%-44s max %.3e / %.0e = %.2f' % (e['id'], r['err_max'], r['bound_max'], r['err_max'] / r['bound_max'])
    if r['bound_mean'] is not None:
        line += '   mean %.3e / %.0e = %.2f' % (r['err_mean'], r['bound_mean'], r['err_mean'] / r['bound_mean'])
    if 'sibling_mismatches' in r:
        line += '   sibling: %d of %d differ from float.to(fp16) (%d not at a rounding tie, farthest %.2f fp32 ulp), max |half - float| %.3e' % (
            r['sibling_mismatches'], r['sibling_elements'], r['sibling_unexplained'], r['sibling_tie_distance'], r['sibling_max_diff'])
    if 'split_diff' in r:
        line += '   split - unsplit %.3e / %.0e%s' % (r['split_diff'], r['split_bound'], ' (differs)' if r['split_differs'] else ' (bit-equal)') \
            + (', %.0f fp16 ulps of the element' % r['split_own_ulps'] if 'split_own_ulps' in r else '')
    print(line + '   plan %s kSplits %d' % (tuple(r['variant'][2:]), r['kSplits']))
    assert tuple(r['variant']) == e['variant'], (r['variant'], e['variant'])
    assert r['finite']
    assert r['err_max'] <= r['bound_max'], (r['err_max'], r['bound_max'])
    if r['bound_mean'] is not None:
        assert r['err_mean'] <= r['bound_mean'], (r['err_mean'], r['bound_mean'])
    if has_sibling(e):
        assert tuple(r['sibling_variant']) == mv.sibling(e)['variant'], r['sibling_variant']
        if e['variant'][2] == mv.FLAT:
            assert r['sibling_mismatches'] == 0, (r['sibling_mismatches'], r['sibling_max_diff'])            # bit for bit
        else:
            # ROWS, GEMM1: bit for bit but where one rounding and two part ways (_near_ties): the fp32 result is the midpoint itself
            # (within half an fp32 ulp of a value on the fp32 grid), which one fp32 value in 2^13 is -- 2^-10 of the elements would
            # be something else
            assert r['sibling_unexplained'] == 0, (r['sibling_mismatches'], r['sibling_unexplained'], r['sibling_tie_distance'])
            assert r['sibling_mismatches'] <= max(8, r['sibling_elements'] >> 10), (r['sibling_mismatches'], r['sibling_elements'])
    if e['kind'] == 'ksplit':
        assert r['kSplits'] == e['kSplits'] and r['reduceGrid'] > 0 and r['unsplit_kSplits'] == 1, r
        assert r['split_diff'] <= r['split_bound'], (r['split_diff'], r['split_bound'])
    else:
        assert r['kSplits'] == 1, r


if __name__ == '__main__':
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.join(os.path.dirname(here), 'stylegan3-editing_amd'), here]
    assert sys.argv[1:] == ['m16'] and os.environ.get(mv.M16_ENV[0]) == mv.M16_ENV[1]
    print(json.dumps([measure(e) for e in mv.ENTRIES if e['kind'] == 'm16']))
