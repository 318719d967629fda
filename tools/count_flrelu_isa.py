"""Instruction budget of the streaming filtered_lrelu plain forward, counted in the compiler's gfx950 assembly.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -fvisibility=hidden -fno-honor-nans --cuda-device-only -DSG3_FLRELU_PART=0 \\
          -Istylegan3-editing_amd/csrc -Iinclude -c stylegan3-editing_amd/csrc/sg3_filtered_lrelu.hip -save-temps -o /tmp/flrelu.o
    python tools/count_flrelu_isa.py sg3_filtered_lrelu-hip-amdgcn-amd-amdhsa-gfx950.s [more.s ...] [--json] [--all]

The kernel file is compiled in parts (its part table; the library links all twelve): -DSG3_FLRELU_PART=0 and =6 hold the separable
plain forward for float and half, without the macro the one compile holds every kernel (minutes, and the same instructions).  Several
assembly files -- one per part, each compiled in a directory of its own -- are read as one.

For every separable plain-forward instantiation flrelu_stream_kernel<T, U, 2, VPH, 0, 0, G, WIDE> (--all: every instantiation) it
prints the vector instructions of one six-row trip of the fast loop (one-instruction activation: v_med3 alone) and of the redo loop
(lrelu + clamp + NaN guard: the loop that holds the v_max of the leaky ReLU), by opcode, next to .vgpr_count, the scratch size, the spill counts and the lane moves
(v_readlane / v_writelane) inside the loops.  The kernel's time is its vector instruction count: this is the table of
profiles/r06_flrelu_up4_ab.txt section 2, made reproducible.

A loop is the text from the first block the compiler marks `Header=<label>` to the end of the last one; the row loops hold no inner
loop and no call, so every instruction of that text executes once per trip (row-validity branches jump over stores only).
"""
import json
import re
import sys

KERNEL = re.compile(r'^_ZN3sg320flrelu_stream_kernelI(f|DF16_)((?:Li\d+E)+)EEvNS_12StreamParamsE$')
META = r'\.(vgpr_count|vgpr_spill_count|sgpr_count|sgpr_spill_count|private_segment_fixed_size):\s+(\d+)'
ARGS = ('T', 'U', 'D', 'VPH', 'RADIAL', 'SIGNS', 'G', 'WIDE')
ROWS_PER_TRIP = 6


def instructions(lines):
    """mnemonic + operands of every instruction line (inline asm included), comments and directives dropped"""
    out = []
    for l in lines:
        code = l.split(';')[0].strip()
        if not code or code.startswith('.') or code.startswith('#') or code.endswith(':'):
            continue
        out.append(code)
    return out


def row_loops(body):
    loops = []
    for i, l in enumerate(body):
        if 'Loop Header' not in l:
            continue
        tag = 'Header=' + re.match(r'^\.L(BB\d+_\d+):', l).group(1)
        member = [j for j, m in enumerate(body) if tag in m] + [i]
        last = max(member) + 1
        while last < len(body) and not body[last].startswith('.LBB'):
            last += 1
        loops.append(instructions(body[min(member):last]))
    return loops


def count_loop(loop):
    ops = {}
    for code in loop:
        op = code.split()[0]
        if op.startswith('v_'):
            op = re.sub(r'_e(32|64)$', '', op)
            ops[op] = ops.get(op, 0) + 1
    lane = sum(n for op, n in ops.items() if op.startswith('v_readlane') or op.startswith('v_writelane'))
    return {'valu': sum(ops.values()), 'valu_per_row': sum(ops.values()) / ROWS_PER_TRIP, 'by_opcode': dict(sorted(ops.items(), key=lambda kv: (-kv[1], kv[0]))),
            'salu': sum(1 for c in loop if c.startswith('s_')), 'lds': sum(1 for c in loop if c.startswith('ds_')),
            'vmem': sum(1 for c in loop if c.startswith('buffer_') or c.startswith('global_')), 'lane_moves': lane}


def analyse(text, every=False):
    lines = text.split('\n')
    meta = {}
    for block in text.split('  - .agpr_count:')[1:]:
        name = re.search(r'\.name:\s+(\S+)', block).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(META, block)}
    out = {}
    for name, m in meta.items():
        t = KERNEL.match(name)
        if not t:
            continue
        args = ('float' if t.group(1) == 'f' else 'half',) + tuple(int(v) for v in re.findall(r'Li(\d+)E', t.group(2)))
        a = dict(zip(ARGS, args))
        if not every and (a['SIGNS'] != 0 or a['RADIAL'] != 0):
            continue
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ':'))
        end = next(i for i in range(start, len(lines)) if 's_endpgm' in lines[i])
        body = lines[start:end + 1]
        rec = {'args': a, 'vgpr_count': m['vgpr_count'], 'sgpr_count': m.get('sgpr_count'), 'scratch_bytes': m['private_segment_fixed_size'],
               'vgpr_spill_count': m['vgpr_spill_count'], 'sgpr_spill_count': m['sgpr_spill_count'],
               'scratch_instructions': sum(1 for c in instructions(body) if c.startswith('scratch_')), 'loops': {}}
        for loop in row_loops(body):
            c = count_loop(loop)
            if c['by_opcode'].get('v_pk_fma_f32', 0) < 100:
                continue                                   # not a row loop
            kind = 'redo' if c['by_opcode'].get('v_max_f32', 0) else 'fast'
            assert kind not in rec['loops'], (name, kind)
            rec['loops'][kind] = c
        out['<' + ', '.join(str(v) for v in args) + '>'] = rec
    return dict(sorted(out.items()))


def main():
    argv = [a for a in sys.argv[1:] if not a.startswith('--')]
    if not argv:
        sys.exit(__doc__)
    text = ''
    for path in argv:                                      # one assembly file per part: kernel names are unique across them
        with open(path) as f:
            text += f.read()
    res = analyse(text, every='--all' in sys.argv)
    if not res:
        sys.exit('no flrelu_stream_kernel in ' + ' '.join(argv))
    if '--json' in sys.argv:
        print(json.dumps(res, indent=1))
        return
    for key, r in res.items():
        print(f"{key}: .vgpr_count {r['vgpr_count']}, scratch {r['scratch_bytes']} B ({r['scratch_instructions']} scratch instructions), "
              f"vector spills {r['vgpr_spill_count']}, scalar spills {r['sgpr_spill_count']}")
        for kind in ('fast', 'redo'):
            c = r['loops'].get(kind)
            if c is None:
                continue
            print(f"    {kind} loop: {c['valu']} VALU per six-row trip ({c['valu_per_row']:.1f} per input row), {c['salu']} SALU, {c['lds']} LDS, "
                  f"{c['vmem']} VMEM, lane moves {c['lane_moves']}")
            print('        ' + ', '.join(f'{n} {op}' for op, n in c['by_opcode'].items()))


if __name__ == '__main__':
    main()
