"""Audit of the hand-issued loads of modconv_f23_kernel in the compiler's output (hipcc -save-temps .s):
between an inline-asm buffer_load and the inline-asm `s_waitcnt vmcnt` that follows it in the text, no instruction may mention
the load's destination registers (vector registers of buffer_load, scalar registers of s_buffer_load until an asm lgkmcnt(0)) (hipcc treats an asm load's destination as written when the load is ISSUED, so a copy, spill or
read placed there moves stale data: cdna_hip_programming.md section 5.7 item 1).  Also reports scratch use, compiler-generated accumulator-register
accesses, and compiler-COUNTED vmcnt waits (N > 0) issued while hand-issued loads are still in flight (the compiler's count does not
include them, so such a wait can release a consumer early).
A linear scan: the pending set is dropped at an unconditional branch (the rotated tile loop places the tile's end in front of its
head; the requests issued before the loop are waited for at the head, not in the text that follows them).
A second pass (transform_rule) covers what the linear scan cannot: the output transform of the cross-tile pipeline, which runs with
the next tile's requests in flight.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -Istylegan3-editing_amd/csrc -c stylegan3-editing_amd/csrc/sg3_modconv_f23.hip -save-temps -o /tmp/x.o
    python tools/audit_f23_asm.py sg3_modconv_f23-hip-amdgcn-amd-amdhsa-gfx950.s
"""
import re
import sys

text = open(sys.argv[1]).read().split('\n')
kern = None
bad = 0
pending = {}          # vector register number -> line of the load
spending = {}         # scalar register number -> line of the scalar-cache load (s_buffer_load into SGPRs, round 4)
apending = 0          # line of the last hand-issued load into accumulator registers that no asm vmcnt wait has covered yet
queue = []            # the hand-issued vector-memory loads in flight, oldest first: (line, [vector destination registers])
in_asm = False
for ln, line in enumerate(text, 1):
    m = re.match(r'^(_ZN3sg318modconv_f23_kernel\w+):', line)
    if m:
        kern, pending, spending, apending, queue = m.group(1), {}, {}, 0, []
    if kern is None:
        continue
    if 's_endpgm' in line:
        kern = None
        continue
    if '#ASMSTART' in line:
        in_asm = True
        continue
    if '#ASMEND' in line:
        in_asm = False
        continue
    code = line.split(';')[0]
    if in_asm and 'buffer_load' in code and 's_buffer_load' not in code:
        d = re.search(r'buffer_load_\w+\s+v\[(\d+):(\d+)\]|buffer_load_\w+\s+v(\d+)', code)
        if d is None:
            apending = ln                                  # destination in the accumulator file: not compiler-visible, but IN FLIGHT
            queue.append((ln, []))
            continue
        lo, hi = (int(d.group(1)), int(d.group(2))) if d.group(1) else (int(d.group(3)), int(d.group(3)))
        for r in range(lo, hi + 1):
            pending[r] = ln
        queue.append((ln, list(range(lo, hi + 1))))
        continue
    if in_asm and 's_buffer_load' in code:
        d = re.search(r's_buffer_load_\w+\s+s\[(\d+):(\d+)\]|s_buffer_load_\w+\s+s(\d+)', code)
        lo, hi = (int(d.group(1)), int(d.group(2))) if d.group(1) else (int(d.group(3)), int(d.group(3)))
        for r in range(lo, hi + 1):
            spending[r] = ln
        continue
    if in_asm and 's_waitcnt' in code:
        w = re.search(r'vmcnt\((\d+)\)', code)
        if w:
            # the counter is in order: all but the N youngest entries have landed.  A wait may say in a comment that K of the
            # entries it leaves out are the output transform's stores ("; +K stores": they are issued by the compiler, in text that
            # the rotated tile loop places elsewhere): it then leaves N - K loads out.
            st = re.search(r';\s*\+(\d+) stores', line)
            keep = max(0, int(w.group(1)) - (int(st.group(1)) if st else 0))
            queue = queue[len(queue) - keep:] if keep else []
            pending = {r: l for l, regs in queue for r in regs}
            apending = max([l for l, regs in queue if not regs], default=0)
        if 'lgkmcnt(0)' in code:
            spending = {}
        continue
    if not in_asm and re.match(r'\s*s_branch\b', code):
        pending, spending, apending, queue = {}, {}, 0, []  # the text behind an unconditional branch is entered from elsewhere (rotated tile loop)
        continue
    if not in_asm and (pending or apending):
        # the compiler counts only the loads IT issued: a counted wait of its own (vmcnt(N), N > 0) while hand-issued loads are in
        # flight behind it lets N of ITS loads... in fact N loads of the whole queue stay out: its consumer may read a register that
        # has not landed.  (vmcnt(0) over-waits, which is only slow.)
        w = re.search(r's_waitcnt.*vmcnt\((\d+)\)', code)
        if w and int(w.group(1)) > 0:
            print(f'{kern}: line {ln}: compiler-counted {code.strip()} while hand-issued loads (line {apending or min(pending.values())}) are in flight'); bad += 1
    if not in_asm and 'v_accvgpr' in code:
        print(f'{kern}: compiler-generated accumulator-register access at line {ln}: {code.strip()}'); bad += 1
    if 'scratch_' in code:
        print(f'{kern}: scratch access at line {ln}: {code.strip()}'); bad += 1
    if not code.strip() or code.strip().startswith('.'):
        continue
    if spending:
        sregs = set()
        for a, b in re.findall(r'\bs\[(\d+):(\d+)\]', code):
            sregs.update(range(int(a), int(b) + 1))
        sregs.update(int(r) for r in re.findall(r'\bs(\d+)\b', code))
        hit = sorted(r for r in sregs if r in spending)
        if hit:
            print(f'{kern}: line {ln} touches s{hit} loaded at line {spending[hit[0]]} before its wait: {code.strip()}'); bad += 1
    if not pending:
        continue
    regs = set()
    for a, b in re.findall(r'v\[(\d+):(\d+)\]', code):
        regs.update(range(int(a), int(b) + 1))
    regs.update(int(r) for r in re.findall(r'\bv(\d+)\b', code))
    hit = sorted(r for r in regs if r in pending)
    if hit:
        print(f'{kern}: line {ln} touches v{hit} loaded at line {pending[hit[0]]} before its wait: {code.strip()}'); bad += 1


def transform_rule(lines):
    """Cross-tile pipeline: the output transform of a tile runs while the NEXT tile's requests are in flight, and the wait that
    names their destinations is the next staging block's -- in the rotated tile loop that is not the text that follows, so the
    linear scan above does not see it.  Rule of its own, per kernel:
      R = the vector destinations of every hand-issued request that is PIPELINED (the next asm vmcnt wait in the text leaves
          loads out: N > 0; a request drained at once by vmcnt(0), the prologue's first, is not in flight later);
      the transform = from the asm statement that loads the demodulation coefficients (s_buffer_load ... s_nop 15) to the next
          branch (it is straight-line code), unless the asm statement in front of it is a vmcnt(0) drain (per-tile flow);
      inside it nothing, compiler's or asm, may mention a register of R, and nothing may wait on the vector-memory counter."""
    found = []
    blocks, cur_block = [], None           # asm statements: (first line, last line, [code lines])
    R, cur = set(), set()
    in_asm = False
    for ln, line in lines:
        code = line.split(';')[0] if '#ASM' not in line else line
        if '#ASMSTART' in line:
            in_asm, cur_block = True, [ln, ln, []]
            continue
        if '#ASMEND' in line:
            in_asm = False
            cur_block[1] = ln
            blocks.append(cur_block)
            continue
        if not in_asm:
            continue
        cur_block[2].append(code)
        if 'buffer_load' in code and 's_buffer_load' not in code:
            d = re.search(r'buffer_load_\w+\s+v\[(\d+):(\d+)\]|buffer_load_\w+\s+v(\d+)', code)
            if d:
                lo, hi = (int(d.group(1)), int(d.group(2))) if d.group(1) else (int(d.group(3)), int(d.group(3)))
                cur.update(range(lo, hi + 1))
        w = re.search(r's_waitcnt.*vmcnt\((\d+)\)', code)
        if w:
            if int(w.group(1)) > 0:
                R |= cur
            cur = set()
    by_line = dict(lines)
    last = max(by_line) if by_line else 0
    for k, (b0, b1, codes) in enumerate(blocks):
        if not (any('s_buffer_load' in c for c in codes) and any(re.search(r's_nop\s+15', c) for c in codes)):
            continue
        if k > 0 and any(re.search(r's_waitcnt.*vmcnt\(0\)', c) for c in blocks[k - 1][2]):
            continue                                             # drained in front of the transform: nothing in flight
        ln = b1 + 1
        while ln <= last:
            code = by_line.get(ln, '').split(';')[0]
            if re.match(r'\s*(s_cbranch\w*|s_branch|s_endpgm|s_setpc_b64)\b', code):
                break
            if code.strip() and not code.strip().startswith('.'):
                regs = set()
                for a, b in re.findall(r'v\[(\d+):(\d+)\]', code):
                    regs.update(range(int(a), int(b) + 1))
                regs.update(int(r) for r in re.findall(r'\bv(\d+)\b', code))
                hit = sorted(r for r in regs if r in R)
                if hit:
                    found.append(f'line {ln}: the output transform touches v{hit}, destination of a request in flight across it: {code.strip()}')
                if re.search(r's_waitcnt.*vmcnt', code):
                    found.append(f'line {ln}: the output transform waits on the vector-memory counter while the next tile\'s requests are in flight: {code.strip()}')
            ln += 1
    return found


kern, klines = None, []
for ln, line in enumerate(text, 1):
    m = re.match(r'^(_ZN3sg318modconv_f23_kernel\w+):', line)
    if m:
        kern, klines = m.group(1), []
    if kern is None:
        continue
    klines.append((ln, line))
    if re.match(r'^\.Lfunc_end', line) or ln == len(text):     # a kernel's text may hold more than one s_endpgm: it ends at its end label
        for f in transform_rule(klines):
            print(f'{kern}: {f}'); bad += 1
        kern = None
print('audit:', 'CLEAN' if bad == 0 else f'{bad} finding(s)')
sys.exit(1 if bad else 0)
