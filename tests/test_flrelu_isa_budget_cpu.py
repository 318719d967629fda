"""CPU: vector-instruction budget of the streaming filtered_lrelu plain forward, counted by tools/count_flrelu_isa.py in the gfx950
assembly (hipcc cross-compiles without a GPU).

The kernel's time is its vector instruction count, so the count per six-row trip of the fast loop is pinned here next
to the register budget that keeps four waves per SIMD.  PARENT holds what the commit before the trim compiled to (counted with the
same tool from its assembly): .vgpr_count and fast-loop VALU per trip of every separable plain-forward instantiation."""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import pytest

import flrelu_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# <T, U, D, VPH, RADIAL, SIGNS, G, WIDE>: (.vgpr_count, fast-loop VALU per six-row trip) of the parent commit
PARENT = {
    '<float, 2, 2, 0, 0, 0, 1, 0>': (122, 580), '<float, 2, 2, 0, 0, 0, 2, 0>': (122, 582),
    '<float, 2, 2, 1, 0, 0, 1, 0>': (124, 580), '<float, 2, 2, 1, 0, 0, 2, 0>': (126, 582),
    '<float, 4, 2, 0, 0, 0, 1, 0>': (104, 1030), '<float, 4, 2, 0, 0, 0, 1, 1>': (141, 1031),
    '<float, 4, 2, 0, 0, 0, 2, 0>': (109, 1032), '<float, 4, 2, 0, 0, 0, 2, 1>': (145, 1032),
    '<float, 4, 2, 1, 0, 0, 1, 0>': (104, 1030), '<float, 4, 2, 1, 0, 0, 1, 1>': (141, 1030),
    '<float, 4, 2, 1, 0, 0, 2, 0>': (111, 1032), '<float, 4, 2, 1, 0, 0, 2, 1>': (147, 1032),
    '<half, 2, 2, 0, 0, 0, 1, 0>': (120, 592), '<half, 2, 2, 0, 0, 0, 2, 0>': (122, 588),
    '<half, 2, 2, 1, 0, 0, 1, 0>': (124, 592), '<half, 2, 2, 1, 0, 0, 2, 0>': (126, 588),
    '<half, 4, 2, 0, 0, 0, 1, 0>': (104, 1048), '<half, 4, 2, 0, 0, 0, 1, 1>': (140, 1048),
    '<half, 4, 2, 0, 0, 0, 2, 0>': (107, 1044), '<half, 4, 2, 0, 0, 0, 2, 1>': (143, 1044),
    '<half, 4, 2, 1, 0, 0, 1, 0>': (104, 1048), '<half, 4, 2, 1, 0, 0, 1, 1>': (138, 1049),
    '<half, 4, 2, 1, 0, 0, 2, 0>': (107, 1044), '<half, 4, 2, 1, 0, 0, 2, 1>': (145, 1044),
}
# The trim had to take at least 40 instructions out of an up-4 trip: the 24 of the output rows' pair sums (one packed add and three
# moves per row -> two adds) and 18 of the 30 around the prefetched rows' bias, rounded.  It took 45 out of <float, 4, 2, 0, 0, 0, 1>
# (985): that form is held at its count + 4.
UP4_HEADLINE = '<float, 4, 2, 0, 0, 0, 1, 0>'
UP4_HEADLINE_BOUND = 989
UP4_MIN_TRIM = 40
# packed FMAs + first-tap multiplies of the four FIR passes (H-up, V-up, V-down, H-down) in a six-row trip, by up factor
FIR_CHAINS = {2: 6 * (12 + 24 + 24 + 12), 4: 6 * (12 + 48 + 48 + 24)}


@pytest.fixture(scope='module')
def counts():
    """tools/count_flrelu_isa.py --json over the assembly of the parts of csrc/sg3_filtered_lrelu.hip that hold the separable plain
    forward (its part table: family 0 of either tensor type), compiled side by side; the flags are csrc/Makefile's"""
    tmp = tempfile.mkdtemp(prefix='sg3_flrelu_isa_')
    try:
        asm = flrelu_parts.assembly(tmp, flrelu_parts.PLAIN_SEPARABLE)
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'count_flrelu_isa.py'), *asm, '--json'], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res = json.loads(out.stdout)
    for key, r in res.items():
        print(key, r['vgpr_count'], {k: v['valu'] for k, v in r['loops'].items()})
    return res


def test_every_plain_forward_form_is_counted(counts):
    assert set(counts) == set(PARENT)
    for key, r in counts.items():
        assert set(r['loops']) == {'fast', 'redo'}, key
        for kind, loop in r['loops'].items():
            # a parser that matches nothing cannot pass: the FIR chains of a trip are all there
            chains = loop['by_opcode'].get('v_pk_fma_f32', 0) + loop['by_opcode'].get('v_pk_mul_f32', 0)
            assert loop['by_opcode'].get('v_pk_fma_f32', 0) > 0 and chains >= FIR_CHAINS[r['args']['U']], (key, kind)
            assert loop['valu'] >= chains


@pytest.mark.parametrize('key', sorted(PARENT))
def test_registers_and_scratch_hold(counts, key):
    r = counts[key]
    assert r['vgpr_count'] <= PARENT[key][0]
    assert r['scratch_bytes'] == 0 and r['scratch_instructions'] == 0 and r['vgpr_spill_count'] == 0
    for kind, loop in r['loops'].items():
        assert loop['lane_moves'] == 0, (key, kind)
    if key.endswith(', 0>'):
        assert r['vgpr_count'] <= 128                         # four waves per SIMD


def test_up4_headline_form(counts):
    assert counts[UP4_HEADLINE]['loops']['fast']['valu'] <= UP4_HEADLINE_BOUND


@pytest.mark.parametrize('key', [k for k in sorted(PARENT) if k.startswith('<float, 4, 2, ') and k.endswith(', 0>')])
def test_up4_trip_is_trimmed(counts, key):
    assert counts[key]['loops']['fast']['valu'] <= PARENT[key][1] - UP4_MIN_TRIM


@pytest.mark.parametrize('key', [k for k in sorted(PARENT) if k.startswith('<half, 4, 2, ')])
def test_fp16_up4_did_not_grow(counts, key):
    """fp16 I/O: the conversions share registers with the trimmed bookkeeping, so only "no higher than the parent" is pinned"""
    assert counts[key]['loops']['fast']['valu'] <= PARENT[key][1]


@pytest.mark.parametrize('key', [k for k in sorted(PARENT) if ', 2, 2, ' in k[:16]])
def test_up2_count_per_input_row_did_not_grow(counts, key):
    assert counts[key]['loops']['fast']['valu'] <= PARENT[key][1]
    assert counts[key]['loops']['fast']['valu_per_row'] <= PARENT[key][1] / 6


@pytest.mark.parametrize('key', [k for k in sorted(PARENT) if k.endswith(', 1>')])
def test_wide_forms_did_not_grow(counts, key):
    assert counts[key]['loops']['fast']['valu'] <= PARENT[key][1]
