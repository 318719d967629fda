"""The parts csrc/sg3_filtered_lrelu.hip is compiled in (its part table is the authority; csrc/Makefile: FLRELU_PARTS), for the CPU
tests that read the compiler's gfx950 assembly (hipcc cross-compiles without a GPU)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'stylegan3-editing_amd', 'csrc')
PARTS = tuple(range(12))
PLAIN_SEPARABLE = (0, 6)          # family 0 (plain forward, separable filters, the WIDE forms included) of float and half
# csrc/Makefile's flags for those objects, device side only
FLAGS = ['-O3', '-std=c++17', '-fPIC', '--offload-arch=gfx950', '-fvisibility=hidden', '-fno-honor-nans', '--cuda-device-only']


def assembly(tmp, parts):
    """Compiles `parts` side by side with -save-temps, each in a directory of its own under `tmp` -> the paths of their gfx950 assembly"""
    procs = []
    for k in parts:
        d = os.path.join(tmp, f'p{k}')
        os.mkdir(d)
        procs.append((d, subprocess.Popen(['/opt/rocm/bin/hipcc', *FLAGS, f'-DSG3_FLRELU_PART={k}', '-I' + CSRC, '-I' + os.path.join(ROOT, 'include'), '-c',
                                           os.path.join(CSRC, 'sg3_filtered_lrelu.hip'), '-save-temps', '-o', os.path.join(d, 'flrelu.o')],
                                          cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)))
    out = []
    for d, p in procs:
        assert p.wait() == 0, d
        asm = [f for f in os.listdir(d) if f.endswith('gfx950.s')]
        assert len(asm) == 1, asm
        out.append(os.path.join(d, asm[0]))
    return out
