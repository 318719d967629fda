"""Time StyleCLIP mapper training on seeded weights (tests/mapper_cases.py, LevelsMapper with all three groups):
  mapper   forward + backward of `w + 0.1 * mapper(w)` to the input and every parameter, on the HIP path (training mode: two ABI
           calls, 5 + 10 launches) and on the torch composite (eval mode under autograd), at N = 2, 8, 32; and the rebuild of the
           prepared weights that follows every optimizer step (one stack and one multiply per tensor kind);
  ranger   one Ranger step of the mapper's 24 parameters, fused (one launch) and on the torch path;
  step     one whole Coach training step on R-1024 at batch 2 with the CLIP loss (seeded ViT-B/32-shaped tower) and latent L2:
           mapper on the HIP path with the fused Ranger, against the composite mapper with the torch-path Ranger, which is what
           the same step costs without the training kernels.  --no_step skips it; --step_only runs one fused step and nothing
           else (for a kernel trace).
HIP events, median of --reps timed repetitions of --iters calls each; every shape is warmed first.  Prints one JSON line.
    python tools/time_styleclip_mapper_train.py [--reps 5] [--iters 20] [--no_step | --step_only]"""
import argparse
import json
import os
import sys
import tempfile
import types

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


def build_coach(tmp):
    import clip_cases
    from criteria.clip_loss import CLIPLoss
    from editing.styleclip_mapper.training.coach import Coach
    torch.save(torch.from_numpy(cases.latents(4)), os.path.join(tmp, 'train.pt'))
    torch.save(torch.from_numpy(cases.latents(2, seed=2)), os.path.join(tmp, 'test.pt'))
    o = types.SimpleNamespace(**dict(
        cases.CASES['levels_all'], exp_dir=os.path.join(tmp, 'exp'), latents_train_path=os.path.join(tmp, 'train.pt'),
        latents_test_path=os.path.join(tmp, 'test.pt'), train_dataset_size=4, test_dataset_size=2, batch_size=2, test_batch_size=1,
        workers=0, test_workers=0, learning_rate=0.5, optim_name='ranger', id_lambda=0.0, clip_lambda=1.0, latent_l2_lambda=0.3,
        stylegan_weights=None, truncation_psi=0.7, stylegan_size=1024, checkpoint_path=None, max_steps=1, image_interval=10 ** 9,
        board_interval=10 ** 9, val_interval=10 ** 9, save_interval=10 ** 9, description='seeded tokens', device=DEV, clip_checkpoint_path=None))
    net = torch.nn.Module()
    net.mapper = cases.build_mapper(cases.opts('levels_all'), cases.state_dict(cases.opts('levels_all')), DEV)
    net.decoder = build_product_generator('R1024', device=DEV)
    clip = clip_cases.build('b32', device=DEV, half=True)
    loss = CLIPLoss(types.SimpleNamespace(stylegan_size=1024, clip_checkpoint_path=None), model=clip)
    return Coach(o, net=net, clip_loss=loss, text_tokens=torch.from_numpy(clip_cases.tokens('b32', 1)))


def train_step(coach, w, fused):
    coach.net.mapper.train(fused)              # eval mode under autograd is the composite
    coach.optimizer.fused = fused
    coach.optimizer.zero_grad()
    with torch.no_grad():
        x = coach.net.decoder.synthesis(w)
    w_hat = coach.edit(w)
    loss, _ = coach.calc_loss(w, x, w_hat, coach.net.decoder.synthesis(w_hat))
    loss.backward()
    coach.optimizer.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--no_step', action='store_true')
    ap.add_argument('--step_only', action='store_true')
    args = ap.parse_args()
    from torch_utils.ops import latent_mapper
    from utils.ranger import Ranger
    res = {'what': 'styleclip_mapper_train', 'mapper': 'LevelsMapper (3 groups)'}
    if args.step_only:
        with tempfile.TemporaryDirectory() as tmp:
            coach = build_coach(tmp)
            w = torch.from_numpy(cases.latents(2)).to(DEV)
            for _ in range(3):
                train_step(coach, w, True)
            torch.cuda.synchronize()
        print(json.dumps({'what': 'styleclip_mapper_train', 'fused_steps_run': 3}))
        return
    o = cases.opts('levels_all')
    m = cases.build_mapper(o, cases.state_dict(o), DEV)
    for n in (2, 8, 32):
        x = torch.from_numpy(cases.latents(n)).to(DEV).requires_grad_(True)
        g = torch.randn(n, 16, 512, device=DEV)

        def fb():
            m.zero_grad(set_to_none=True)
            x.grad = None
            m.edit(x).backward(g)
        m.train()
        t_fused = event_time(fb, args.reps, args.iters)
        m.eval()
        t_comp = event_time(fb, args.reps, args.iters)
        res[f'mapper_fwd_bwd_N{n}_us'] = {'fused': round(t_fused, 2), 'torch': round(t_comp, 2)}
        print(f'N={n}: {res[f"mapper_fwd_bwd_N{n}_us"]}', file=sys.stderr, flush=True)
    mappers = [g for _, g in m._groups()]
    res['prepare_weights_us'] = round(event_time(lambda: latent_mapper.PreparedMapper(mappers, torch.device(DEV)), args.reps, args.iters), 2)
    for p in m.parameters():
        p.grad = torch.randn_like(p)
    for name, fused in (('fused', True), ('torch', False)):
        opt = Ranger(list(m.parameters()), lr=1e-3)
        opt.fused = fused
        res.setdefault('ranger_step_us', {})[name] = round(event_time(opt.step, args.reps, args.iters), 2)
    print(json.dumps(res), file=sys.stderr, flush=True)
    if not args.no_step:
        with tempfile.TemporaryDirectory() as tmp:
            coach = build_coach(tmp)
            w = torch.from_numpy(cases.latents(2)).to(DEV)
            reps, iters = max(3, args.reps // 2), 3
            res['train_step_R1024_b2_ms'] = {
                'fused': round(event_time(lambda: train_step(coach, w, True), reps, iters) / 1e3, 3),
                'torch': round(event_time(lambda: train_step(coach, w, False), reps, iters) / 1e3, 3)}
    res['device'] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
