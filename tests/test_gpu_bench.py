"""GPU: what `bench.py` prints.  A plain run carries the headline alone (the secondary figures are null); `--full` adds the per-kernel
roofline figures, measured from an eager pass after the timed graph replays."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ('roofline', 'modconv', 'inversion', 'inversion_T1024', 'extras', 'cpu_baseline')


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1'] + args, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out['metric'] == 'FFHQ-1024 StyleGAN3-T synthesis imgs/sec' and out['unit'] == 'imgs/s' and out['dtype'] == 'f32'
    assert out['higher_is_better'] is True and out['steps'] == 2 and out['warmup'] == 1 and out['n_gpus'] == 1
    assert out['value'] > 0 and out['value'] * out['ms_per_step'] == pytest.approx(8 * 1e3)     # batch 8: images per second <-> ms per step
    assert out['config']['launch'] == 'hipGraph replay'
    return out


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    out = _bench(['--dump-outputs', str(tmp_path)])
    assert all(out[k] is None for k in SECONDARY), {k: out[k] for k in SECONDARY}
    assert sorted(os.listdir(tmp_path)) == ['image0.npy', 'images_channel_mean.npy', 'images_sample.npy']


@pytest.mark.gpu
def test_full_run_adds_the_kernel_figures():
    out = _bench(['--full', '--no-inversion', '--no-extras', '--no-cpu-baseline'])
    assert out['roofline']['kernel_ms_per_step'] > 0 and out['roofline']['algorithmic_bytes_per_step'] > 0
    assert out['modconv']['kernel_ms_per_step'] > 0 and out['modconv']['f23_layers'] > 0
    assert all(out[k] is None for k in ('inversion', 'inversion_T1024', 'extras', 'cpu_baseline'))
