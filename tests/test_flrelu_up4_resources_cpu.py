"""CPU: register budget of the streaming filtered_lrelu kernels, read from the gfx950 assembly (hipcc cross-compiles without a GPU).

A SIMD lane has 512 vector registers, so a kernel is resident at four waves per SIMD when it needs at most 512 / 4 = 128 of them
(architectural + accumulator).  The up-4 separable plain forward must stay there without scratch, without spilled vector registers
and without spilled scalars moving through v_readlane / v_writelane inside its row loops; the up-2 forms must not grow past it."""
import re
import shutil
import tempfile

import pytest

import flrelu_parts

WAVES = 4
VGPR_BUDGET = 512 // WAVES


@pytest.fixture(scope='module')
def listing():
    """{demangled template arguments: (metadata, body lines)} of every separable plain-forward flrelu_stream_kernel (the parts of
    csrc/sg3_filtered_lrelu.hip that hold them, compiled side by side); the flags are csrc/Makefile's."""
    tmp = tempfile.mkdtemp(prefix='sg3_flrelu_res_')
    try:
        text = ''
        for path in flrelu_parts.assembly(tmp, flrelu_parts.PLAIN_SEPARABLE):
            with open(path) as f:
                text += f.read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    lines = text.split('\n')
    meta = {}
    for block in text.split('  - .agpr_count:')[1:]:
        name = re.search(r'\.name:\s+(\S+)', block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r'\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)', block)}
    out = {}
    for name, m in meta.items():
        t = re.match(r'_ZN3sg320flrelu_stream_kernelI(f|DF16_)((?:Li\d+E)+)EEvNS_12StreamParamsE$', name)
        if not t:
            continue
        start = lines.index(next(l for l in lines if l.startswith(name + ':')))
        end = next(i for i in range(start, len(lines)) if 's_endpgm' in lines[i])
        key = ('float' if t.group(1) == 'f' else 'half',) + tuple(int(v) for v in re.findall(r'Li(\d+)E', t.group(2)))
        out[key] = (m, lines[start:end + 1])
    assert out
    return out


def _row_loops(body):
    """the instruction lines of every loop of a kernel, from the first block the compiler marks as belonging to it to the end of the last"""
    loops = []
    for i, l in enumerate(body):
        if 'Loop Header' not in l:
            continue
        tag = 'Header=' + re.match(r'^\.L(BB\d+_\d+):', l).group(1)
        member = [j for j, m in enumerate(body) if tag in m] + [i]
        last = max(member) + 1
        while last < len(body) and not body[last].startswith('.LBB'):
            last += 1
        loops.append([m.split(';')[0].strip() for m in body[min(member):last]])
    return loops


# <T, U, D, VPH, RADIAL, SIGNS, G, WIDE>: the plain forward, separable, both vertical phases, one and two planes per wave
UP4 = [('float', 4, 2, v, 0, 0, g, 0) for v in (0, 1) for g in (1, 2)]
UP2 = [('float', 2, 2, v, 0, 0, g, 0) for v in (0, 1) for g in (1, 2)]


@pytest.mark.parametrize('key', UP4, ids=lambda k: 'x'.join(str(v) for v in k))
def test_up4_plain_forward_fits_four_waves_per_simd(listing, key):
    meta, body = listing[key]
    print(key, meta)
    assert meta['vgpr_count'] <= VGPR_BUDGET
    assert meta['private_segment_fixed_size'] == 0 and meta['vgpr_spill_count'] == 0
    assert not [l for l in body if re.match(r'\s*scratch_', l)]
    loops = _row_loops(body)
    assert len(loops) == 2                     # the fast pass and the redo pass, six rows per trip each
    for loop in loops:
        fmas = [l for l in loop if l.startswith('v_pk_fma_f32') or l.startswith('v_pk_mul_f32')]
        assert len(fmas) >= 6 * (12 + 48 + 48 + 24)          # the row loop, not some other loop
        assert not [l for l in loop if l.startswith('v_readlane') or l.startswith('v_writelane')]
        assert not [l for l in loop if l.startswith('ds_read2_b64')]


def test_fp16_up4_comes_along(listing):
    for v in (0, 1):
        for g in (1, 2):
            meta, body = listing[('half', 4, 2, v, 0, 0, g, 0)]
            assert meta['vgpr_count'] <= VGPR_BUDGET and meta['private_segment_fixed_size'] == 0 and meta['vgpr_spill_count'] == 0
            for loop in _row_loops(body):
                assert not [l for l in loop if l.startswith('v_readlane') or l.startswith('v_writelane')]


@pytest.mark.parametrize('key', UP2, ids=lambda k: 'x'.join(str(v) for v in k))
def test_up2_plain_forward_did_not_grow(listing, key):
    meta, _ = listing[key]
    print(key, meta)
    assert meta['vgpr_count'] <= VGPR_BUDGET and meta['private_segment_fixed_size'] == 0 and meta['vgpr_spill_count'] == 0


def test_the_wide_form_is_still_built(listing):
    """the earlier form of the up-4 kernels stays selectable (A/B timing, the bit-identity test)"""
    for v in (0, 1):
        for g in (1, 2):
            assert ('float', 4, 2, v, 0, 0, g, 1) in listing
