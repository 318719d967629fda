"""CPU: the streaming filtered_lrelu kernels are compiled in parts (csrc/sg3_filtered_lrelu.hip, its part table) and looked up from
another translation unit (csrc/sg3_flrelu_host.hip).  Two things keep that honest without a GPU:

  * every call of tests/golden/flrelu_dispatch.json goes through sg3_filtered_lrelu_dispatch, which resolves the kernel pointer of every
    launch of its plan (host only: it follows no pointer) -- SG3_OK for every call the table records launches for, the recorded refusal
    for the others;
  * the kernel NAMES in the library's gfx950 code objects (their symbol tables; no instruction is looked at) are exactly the 164 the
    lookup can return, each in one code object only -- a leaf listed in two parts would link (the host stubs are merged) and load."""
import ctypes
import struct

import pytest

import test_flrelu_dispatch_cpu as D


@pytest.fixture(scope='module')
def table():
    return D._load_table()


def test_every_table_call_resolves_its_kernels(table):
    """SG3_FLRELU_NOPACK is read once per process, so the rows recorded under it run here without it: another plan than the recorded
    one, whose kernels must be there all the same."""
    abi, lib = D._lib()
    ok = 0
    for c, q in zip(table['calls'], table['queries']):
        p = D._params(c)
        info = abi.FilteredLreluDispatchInfo()
        if c['knob'] == D.KNOB_NOPACK:
            rc = lib.sg3_filtered_lrelu_dispatch(ctypes.byref(p), ctypes.byref(info))
        else:
            with D._knob(lib, c['knob']):
                rc = lib.sg3_filtered_lrelu_dispatch(ctypes.byref(p), ctypes.byref(info))
        if q['rc'] == abi.SG3_OK:
            assert rc == abi.SG3_OK, (c, rc, lib.sg3_last_error())
            ok += 1
        else:
            # a refusal names no kernel: it is the plan's (kind NONE) or an argument check's, never a missing instantiation
            assert rc == q['rc'] and 'no flrelu_stream_kernel<' not in abi.last_error(), (c, rc, abi.last_error())
            assert rc != abi.SG3_NO_KERNEL or info.kind == abi.SG3_FLRELU_NONE, c
    assert ok > 2000


def _code_objects(path):
    """the gfx950 code objects of a library: the entries of every clang offload bundle in it"""
    magic = b'__CLANG_OFFLOAD_BUNDLE__'
    with open(path, 'rb') as f:
        data = f.read()
    out = []
    at = data.find(magic)
    while at >= 0:
        count, = struct.unpack_from('<Q', data, at + len(magic))
        pos = at + len(magic) + 8
        for _ in range(count):
            offset, size, triple_len = struct.unpack_from('<QQQ', data, pos)
            triple = data[pos + 24:pos + 24 + triple_len]
            pos += 24 + triple_len
            if b'gfx950' in triple and size:
                out.append(data[at + offset:at + offset + size])
        at = data.find(magic, at + 1)
    return out


def _kernel_descriptors(elf):
    """names of the kernel descriptor symbols (`<kernel>.kd`) in the symbol table of one ELF64 little-endian code object"""
    assert elf[:6] == b'\x7fELF\x02\x01', elf[:6]
    shoff, = struct.unpack_from('<Q', elf, 0x28)
    shentsize, shnum = struct.unpack_from('<HH', elf, 0x3A)
    sections = [struct.unpack_from('<IIQQQQIIQQ', elf, shoff + i * shentsize) for i in range(shnum)]
    names = []
    for _, kind, _, _, offset, size, link, _, _, entsize in sections:
        if kind != 2:                                                   # SHT_SYMTAB
            continue
        str_off = sections[link][4]
        for i in range(size // entsize):
            name_at, = struct.unpack_from('<I', elf, offset + i * entsize)
            end = elf.index(b'\0', str_off + name_at)
            name = elf[str_off + name_at:end].decode()
            if name.endswith('.kd'):
                names.append(name[:-3])
    return names


def _lookup_kernels():
    """Mangled names of what `stream_kernel` (csrc/sg3_flrelu_host.hip) can return: per tensor type the two WIDE leaves, the six adjoint
    leaves and the thirty forward leaves, each with the D vertical phases of its down factor."""
    leaves = [(4, 2, 0, 0, g, 1) for g in (1, 2)]                                                          # (U, D, RADIAL, SIGNS, G, WIDE)
    leaves += [(2, d, r, 2, 1, 0) for d in (2, 4) for r in (0, 3, 4)]
    leaves += [(u, 2, r, s, g, 0) for s, g in ((1, 1), (0, 1), (0, 2)) for u in (2, 4) for r in (0, 1, 2, 5, 6)]
    assert len(leaves) == len(set(leaves)) == 38
    out = set()
    for t in ('f', 'DF16_'):
        for u, d, r, s, g, w in leaves:
            for v in range(d):
                out.add('_ZN3sg320flrelu_stream_kernelI%s%sEEvNS_12StreamParamsE' % (t, ''.join('Li%dE' % a for a in (u, d, v, r, s, g, w))))
    assert len(out) == 164
    return out


def test_library_holds_each_lookup_kernel_once(table):
    from torch_utils import _sg3abi
    objects = _code_objects(_sg3abi.LIB_PATH)
    assert len(objects) >= 13                      # the twelve parts and the host file, next to the other sources
    found = [n for elf in objects for n in _kernel_descriptors(elf) if 'flrelu_stream_kernel' in n]
    assert len(found) == len(set(found)), sorted(n for n in set(found) if found.count(n) > 1)
    want = _lookup_kernels()
    assert set(found) == want, (sorted(want - set(found)), sorted(set(found) - want))
    # the table's launches name kernels of that set (what test_table_reaches_every_kernel_of_the_library reads off the host stubs)
    for c, launches in zip(table['calls'], table['launches']):
        for la in launches:
            if la['kind'] == 2:
                name = '_ZN3sg320flrelu_stream_kernelI%s%sEEvNS_12StreamParamsE' % ('f' if c['dtype'] == 0 else 'DF16_', ''.join('Li%dE' % la[k] for k in D.STREAM_COORDS))
                assert name in want, (c, la)
