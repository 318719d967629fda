"""GPU: every modulated-convolution kernel the launch plan can choose, run through the C ABI and compared with float64.

One test per row of tests/modconv_variant_cases.py (80 variant rows, the padding-0, K-split, ToRGB and demodulation-off extras) and
one for the twelve M16 = 0 kernels of the 1x1 GEMM, which run in one child process with SG3_CONV1_MFMA32=1.  tests/modconv_abi.py
drives prep + convolution with the row's own precision code and tensor type: the 28 crossed kernels (fp32 tensors on the
single-product arithmetic, fp16 tensors on the split arithmetic) are offered by include/sg3_ops.h to any C caller and chosen by no
call of the Python op.

Per row:
  * the plan reported on the device is the variant the row is filed under (an MI355X has the 256 CUs the table was searched at);
  * |out - float64 reference| relative to scale = max(1, max |ref|) keeps the bound tests/test_gpu_ops.py holds for the arithmetic:
    5e-6 for exact or split products into fp32, 1e-3 for the same into fp16, max 4e-3 and mean 4e-4 for single fp16 products
    (modconv_abi.bounds); x is fp16-representable (rand * 20 clipped to +-256), x_bound = 256;
  * no store lands outside the output tensor (sentinels on both sides of it).

The sibling check.  A crossed row is run again on the other tensor type, same values, same template coordinates, same SPLIT.  In all
three families the tensor type T enters the kernel through loads and stores alone: same operand rounding, same accumulation order,
and the fp16 store is `(_Float16)(acc * d)`, round to nearest even as torch's .to(float16).
  * FLAT, modconv_flat_kernel (csrc/sg3_modconv.hip): x is read by bufld<T>::ld in its `fetch` lambda (struct bufld in
    csrc/sg3_split.h: fp16 is widened to fp32, exactly) and is fp32 from there on -- scaled, then split2 / round2 in `stage`; the MFMA
    order (the tap loop) does not name T; the epilogue forms v = acc * d in fp32 and stores v or (_Float16)v (the `desc` loop at the
    end).  With a K split the partial images are fp32 for both T (the `p.kSplits > 1` branch) and modconv_split_reduce_kernel<T>
    rounds `(T)(v * d)`.
    Relation asserted: out_half == out_float.to(float16), BIT FOR BIT (0 of 35.7 million elements differ).
  * ROWS, modconv_f16x3_kernel: load in `fetch`, rounding in `stage`, MFMA order in `mfma_row`, stores in the descriptor branch of
    the epilogue (predicated form below it through io<T>::st, csrc/sg3_common.h).
  * GEMM1, modconv1_f16x3_kernel: pixel pairs by bufld<T>::ld2 in `fetch` and unpack2 in `stage`, rounding in `stage`, MFMA order in
    `mfma_step` and `stage_m16` (32-wide and M16 forms), stores in the three epilogue branches (M16, descriptor, predicated).  The plan
    splits K for fp32 tensors only, so the K-split rows of this family
    have no sibling with the same summation order; their unsplit variant rows are the ones compared.
    The source of ROWS and GEMM1 reads like FLAT's, the machine code does not: hipcc (default -ffp-contract) compiles their
    `(_Float16)(acc * d)` to ONE v_fma_mixlo_f16, which rounds the exact product to fp16 once, where the fp32 kernel's v_mul_f32
    followed by .to(float16) rounds twice (FLAT uses v twice and keeps v_mul_f32 + v_cvt_f16_f32).  One rounding and two part ways
    only where the fp32 result is an exact tie between two fp16 neighbours.  Relation asserted: out_half == out_float.to(float16)
    bit for bit, except where out_float is such a tie and out_half is one of the two neighbours (modconv_abi._near_ties); measured
    1619 of 26.9 million elements (6e-5; one fp32 value in 2^13 is a tie), none unexplained.  This is stronger than the fallback of
    half an fp16 ulp plus the fp32 bound, which it implies.

K-split rows are run a second time without scratch (one workgroup per tile walks all chunks): fp32 outputs agree within 4e-6 scale
(two fp32 summation orders, the bound of test_modulated_conv2d_k_split_on_small_grids_matches_the_unsplit_kernel; 8.8e-7 measured).
fp16 outputs are fp16 roundings of two such fp32 sums, so they agree within ONE FP16 ULP OF THE RESULT BEYOND THAT fp32 difference:
|split - unsplit| <= ulp16(result) + 4e-6 scale per element (measured 0.99 of it; in particular within one fp16 ulp at scale).  One
ulp of the element alone is not a property of any correct kernel: where the plane passes through zero an element of 1e-3 scale has an
ulp of 5e-7 scale, the size of the fp32 difference itself (measured: 2, 10, 12 and 7 such ulps on the four fp16 rows).

Figures of the run this file was written against (MI355X): 152 tests in 6.6 s; largest error / bound 0.43 (ROWS, split into fp16).
"""
import json
import os
import subprocess
import sys

import pytest

import modconv_abi as drv
import modconv_variant_cases as mv

pytestmark = pytest.mark.gpu

IN_PROCESS = [e for e in mv.ENTRIES if e['kind'] != 'm16']
M16 = [e for e in mv.ENTRIES if e['kind'] == 'm16']


@pytest.mark.parametrize('e', IN_PROCESS, ids=[e['id'] for e in IN_PROCESS])
def test_variant_against_float64(e):
    drv.check(e, drv.measure(e))


def test_a_four_way_k_split_differs_from_the_unsplit_result():
    """Proof that the split path ran: four partial sums added in order are not, bit for bit, one sum over all of K."""
    rows = [e for e in IN_PROCESS if e['kind'] == 'ksplit' and e['kSplits'] == 4]
    assert len(rows) == 6
    differs = []
    for e in rows:
        split, plan = drv.run(e)
        plain, plan1 = drv.run(e, offer_scratch=False)
        assert plan['kSplits'] == 4 and plan1['kSplits'] == 1
        differs.append(not bool((split == plain).all()))
    print('kSplits = 4 rows whose result differs from the unsplit one: %d of %d' % (sum(differs), len(rows)))
    assert any(differs)


def test_m16_variants_in_a_child_process():
    """The twelve 32x32x16 kernels of the double-buffered 1x1 tiles: SG3_CONV1_MFMA32 is read once per process, so one fresh child
    measures all twelve rows (tests/modconv_abi.py m16) and this process asserts on the figures.  A child that dies or runs out of
    time fails the test; it is not started again."""
    assert len(M16) == 12
    env = dict(os.environ)
    env[mv.M16_ENV[0]] = mv.M16_ENV[1]
    child = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'modconv_abi.py'), 'm16'],
                           env=env, capture_output=True, text=True, timeout=300)
    assert child.returncode == 0, (child.returncode, child.stdout[-2000:], child.stderr[-2000:])
    results = json.loads(child.stdout.strip().splitlines()[-1])
    assert [r['id'] for r in results] == [e['id'] for e in M16]
    for e, r in zip(M16, results):
        drv.check(e, r)
    assert sum('sibling_mismatches' in r for r in results) == 6
