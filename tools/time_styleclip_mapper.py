"""Time the StyleCLIP latent mapper on seeded weights (tests/mapper_cases.py, LevelsMapper with all three groups): one forward
`w + 0.1 * mapper(w)` on the fused HIP path (`LevelsMapper.edit`, five launches) and on the torch composite (the reference's
module arithmetic), eager and graph-replayed, at N = 1, 8, 32, 256; then `run_on_batch` on R-1024 at batch 1 and 8.  HIP
events, median of --reps timed repetitions of --iters calls each; every shape is warmed first.  Prints one JSON line.
    python tools/time_styleclip_mapper.py [--reps 5] [--iters 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests'), ROOT):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import mapper_cases as cases  # noqa: E402
from helpers import build_product_generator  # noqa: E402

DEV = 'cuda:0'


def event_time(fn, reps, iters):
    """Median over reps of the mean per-call time (microseconds) of `iters` back-to-back calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / iters)
    return float(np.median(ts))


def graphed(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    o = cases.opts('levels_all')
    m = cases.build_mapper(o, cases.state_dict(o), DEV).requires_grad_(False)
    res = {'what': 'styleclip_mapper', 'mapper': 'LevelsMapper (3 groups)', 'unit': 'us per forward (w + 0.1 * mapper(w))'}
    with torch.no_grad():
        for n in (1, 8, 32, 256):
            x = torch.from_numpy(cases.latents(n)).to(DEV)
            fused = lambda: m.edit(x)                                                   # noqa: E731
            m.train()                                                                   # train mode keeps the module on the composite
            composite = lambda: x + 0.1 * m(x)                                          # noqa: E731
            t_comp = event_time(composite, args.reps, args.iters)
            g_comp = graphed(composite)
            t_comp_g = event_time(g_comp, args.reps, args.iters)
            m.eval()
            t_fused = event_time(fused, args.reps, args.iters)
            g_fused = graphed(fused)
            t_fused_g = event_time(g_fused, args.reps, args.iters)
            res[f'N{n}'] = {'fused_eager': round(t_fused, 2), 'fused_graph': round(t_fused_g, 2),
                            'torch_eager': round(t_comp, 2), 'torch_graph': round(t_comp_g, 2)}
        from editing.styleclip_mapper.scripts.inference import run_on_batch
        net = torch.nn.Module()
        net.mapper = m
        net.decoder = build_product_generator('R1024', device=DEV)
        for b in (1, 8):
            w = torch.from_numpy(cases.latents(b)).to(DEV)
            t = torch.eye(3, device=DEV).expand(b, 3, 3).contiguous()
            res[f'run_on_batch_R1024_b{b}_ms'] = round(event_time(lambda: run_on_batch(w, t, net), max(3, args.reps // 2), 3) / 1e3, 3)
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
