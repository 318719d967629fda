"""The audit's rule for the cross-tile pipeline of csrc/sg3_modconv_f23.hip (tools/audit_f23_asm.py, transform_rule): the output
transform runs while the next tile's requests are in flight, so it may neither touch their destination registers nor wait on the
vector-memory counter.  Tested on synthetic listings, as the other rules are in test_f23_audit_cpu.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUDIT = os.path.join(ROOT, 'tools', 'audit_f23_asm.py')

HEAD = '_ZN3sg318modconv_f23_kernelILi7EfEEvNS_9F23ParamsE:\n'
TAIL = '\ts_endpgm\n.Lfunc_end0:\n'

# a pipelined request (waited for with loads left out), then the transform's opening statement, its body and the loop's back branch
REQUEST = ('\t;;#ASMSTART\n\ts_nop 4\n\tbuffer_load_dwordx2 v[16:17], v53, s[56:59], s10 offen\n\t;;#ASMEND\n'
           '\t;;#ASMSTART\n\ts_waitcnt vmcnt(16)\n\t;;#ASMEND\n')
DRAIN = '\t;;#ASMSTART\n\ts_waitcnt vmcnt(0) lgkmcnt(0)\n\t;;#ASMEND\n'
OPEN = '\t;;#ASMSTART\n\ts_nop 4\n\ts_buffer_load_dwordx8 s[72:79], s[4:7], s9\n\ts_nop 15\n\ts_nop 7\n\ts_waitcnt lgkmcnt(0)\n\t;;#ASMEND\n'
BODY = '\tv_mov_b32_e32 v3, v48\n\tbuffer_store_dwordx2 v[50:51], v9, s[52:55], 0 offen\n\ts_barrier\n'
BACK = '\ts_branch .LBB5_7\n\tv_mov_b32_e32 v4, v16\n'                   # behind the branch: not the transform any more


def _audit(text, tmp_path):
    f = tmp_path / 'k.s'
    f.write_text(HEAD + text + TAIL)
    r = subprocess.run([sys.executable, AUDIT, str(f)], capture_output=True, text=True)
    return r.returncode, r.stdout


def test_counted_wait_keeps_the_youngest_loads_in_flight(tmp_path):
    """The queue model: an asm vmcnt(N) leaves the N youngest hand-issued loads in flight.  The case that got through before it: the
    wait that lands the A fragments (vmcnt(2) here) is followed by copies of the sample registers in front of THEIR wait."""
    loads = ('\t;;#ASMSTART\n\ts_nop 4\n\tbuffer_load_dwordx2 v[16:17], v53, s[56:59], s10 offen\n'
             '\tbuffer_load_dwordx2 v[18:19], v54, s[56:59], s10 offen\n\t;;#ASMEND\n'
             '\t;;#ASMSTART\n\ts_waitcnt vmcnt(2)\n\t;;#ASMEND\n')
    wait = '\t;;#ASMSTART\n\ts_waitcnt vmcnt(0)\n\t;;#ASMEND\n\tv_mov_b64_e32 v[52:53], v[18:19]\n'
    assert _audit(loads + '\tv_add_u32_e32 v2, v3, v4\n' + wait, tmp_path)[0] == 0
    rc, out = _audit(loads + '\tv_mov_b64_e32 v[52:53], v[18:19]\n' + wait, tmp_path)
    assert rc == 1 and 'touches v[18, 19]' in out
    # vmcnt(1): the older load has landed, the younger has not
    one = loads.replace('vmcnt(2)', 'vmcnt(1)')
    assert _audit(one + '\tv_mov_b32_e32 v2, v16\n' + wait, tmp_path)[0] == 0
    rc, out = _audit(one + '\tv_mov_b32_e32 v2, v19\n' + wait, tmp_path)
    assert rc == 1 and 'touches v[19]' in out
    # a wait that declares stores among the entries it leaves out: vmcnt(3) with two stores leaves ONE load out
    st = loads.replace('s_waitcnt vmcnt(2)', 's_waitcnt vmcnt(3) ; +2 stores')
    assert _audit(st + '\tv_mov_b32_e32 v2, v17\n' + wait, tmp_path)[0] == 0
    rc, out = _audit(st + '\tv_mov_b32_e32 v2, v18\n' + wait, tmp_path)
    assert rc == 1 and 'touches v[18]' in out


def test_transform_rule_fires_on_synthetic_violations(tmp_path):
    assert _audit(REQUEST + OPEN + BODY + BACK, tmp_path)[0] == 0
    # the transform reads, copies or overwrites a destination of the request in flight
    rc, out = _audit(REQUEST + OPEN + BODY.replace('v3, v48', 'v3, v17') + BACK, tmp_path)
    assert rc == 1 and 'output transform touches v[17]' in out
    rc, out = _audit(REQUEST + OPEN + BODY.replace('v[50:51]', 'v[16:17]') + BACK, tmp_path)
    assert rc == 1 and 'output transform touches v[16, 17]' in out
    # a wait on the vector-memory counter inside the transform drains the next tile's requests
    rc, out = _audit(REQUEST + OPEN + '\ts_waitcnt vmcnt(0)\n' + BODY + BACK, tmp_path)
    assert rc == 1 and 'waits on the vector-memory counter' in out
    # the transform laid out in FRONT of the request in the text (the rotated tile loop) is covered as well
    rc, out = _audit(OPEN + BODY.replace('v3, v48', 'v3, v17') + BACK + REQUEST, tmp_path)
    assert rc == 1 and 'output transform touches v[17]' in out
    # per-tile flow: everything drained in front of the transform, the registers are free
    assert _audit(REQUEST + DRAIN + OPEN + BODY.replace('v3, v48', 'v3, v17') + BACK, tmp_path)[0] == 0
    # a request that is drained at once (the prologue's first) is not in flight later
    first = REQUEST.replace('vmcnt(16)', 'vmcnt(0) lgkmcnt(0)').replace('v[16:17]', 'v[0:1]')
    assert _audit(first + REQUEST + OPEN + BODY.replace('v3, v48', 'v3, v1') + BACK, tmp_path)[0] == 0
