"""Time the LPIPS criterion (AlexNet, seeded weights from tests/lpips_cases.py; kernel time does not depend on the weights' values) at
1 x 3 x 1024 x 1024 with a cached target, as PTI calls it 350 times per image:

  (a) the HIP path, forward and backward, and (b) the package's float32 composite under autograd (the library's convolutions, MIOpen
      enabled and warmed) on the same GPU, the two alternated inside one timed loop so clock drift hits both alike;
  the HIP path's forward and backward apart, and every kernel of it alone (one call each on the tensors of a real step);
  a T-1024 PTI step (forward + backward + fused Adam) with the MSE term alone and with the criterion added.

Device events around each call, `--warmup` untimed rounds, `--reps` timed rounds; median, min and max are reported.  The clock is
whatever the device runs at under this load (not pinned).  Prints one JSON line.
    python tools/time_lpips.py [--reps 20] [--warmup 5] [--size 1024] [--no-pti]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'stylegan3-editing_amd'), os.path.join(ROOT, 'tests'), ROOT, os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
import torch  # noqa: E402

import lpips_cases as cases  # noqa: E402
from time_clip_encoder import alternate  # noqa: E402

DEV = 'cuda:0'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--no-pti', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_lpips.py measures on a GPU; none is visible')
    from torch_utils import _sg3abi as abi
    from torch_utils.ops import lpips_ops
    m = cases.build(torch.float32, DEV)
    y = cases.images(1, a.size, a.size, seed=1).to(DEV)
    x = cases.perturbed(y, seed=2).requires_grad_(True)
    assert m.uses_hip(x)
    res = {'box': torch.cuda.get_device_name(0), 'model': 'LPIPS AlexNet v0.1, seeded weights', 'size': a.size, 'batch': 1, 'reps': a.reps,
           'warmup': a.warmup, 'clock': 'not pinned', 'ms': '[median, min, max] per call', 'target': 'cached'}

    def step(fn):
        x.grad = None
        fn(x, y).backward()

    step(m)                                      # packs the weights and caches the target's features
    before = abi.launch_count
    step(m)
    res['hip_calls_per_step'] = abi.launch_count - before
    with torch.backends.cudnn.flags(enabled=True):
        step(m.composite)
        hip, comp = alternate(lambda: step(m), lambda: step(m.composite), a.reps, a.warmup)
    res['hip_fwd_bwd_ms'], res['torch_fp32_fwd_bwd_ms'], res['hip_over_torch_time'] = hip, comp, hip[0] / comp[0]

    state = {}

    def fwd():
        state['loss'] = m(x, y)

    def bwd():
        torch.autograd.grad(state['loss'], x, retain_graph=True)

    fwd()
    res['hip_forward_ms'], res['hip_backward_ms'] = alternate(fwd, bwd, a.reps, a.warmup)

    # every kernel alone, on the tensors of a real step
    ops = m._operands(x.device)
    xd = x.detach()
    with torch.no_grad():
        canvas = lpips_ops.prepare(xd, ops.mean, ops.std)
        f = m._features_hip(xd, ops)
        fy = m._y_features(y, ops)
        p1, p2 = lpips_ops.maxpool3s2(f[0]), lpips_ops.maxpool3s2(f[1])
        heads = [lpips_ops.head(u, v, lin, want_grad=True, relu_mask=(i == 4))[1] for i, (u, v, lin) in enumerate(zip(f, fy, ops.lin))]
        oh, ow = int(f[0].shape[2]), int(f[0].shape[3])
        ring = torch.zeros([1, 64, oh + 2, ow + 2], dtype=torch.float32, device=DEV)
        dcanvas = torch.randn_like(canvas) * 1e-6
        dp = [torch.randn_like(p1) * 1e-6, torch.randn_like(p2) * 1e-6]
        kernels = {
            'prepare': lambda: lpips_ops.prepare(xd, ops.mean, ops.std),
            'conv1_11x11s4_as_3x3_48ch': lambda: ops.conv[0](canvas),
            'pool1': lambda: lpips_ops.maxpool3s2(f[0]),
            'conv2_5x5_64_192': lambda: ops.conv[1](p1),
            'pool2': lambda: lpips_ops.maxpool3s2(f[1]),
            'conv3_3x3_192_384': lambda: ops.conv[2](p2),
            'conv4_3x3_384_256': lambda: ops.conv[3](f[2]),
            'conv5_3x3_256_256': lambda: ops.conv[4](f[3]),
            'head1_grad': lambda: lpips_ops.head(f[0], fy[0], ops.lin[0], want_grad=True),
            'head2_grad': lambda: lpips_ops.head(f[1], fy[1], ops.lin[1], want_grad=True),
            'head3_grad': lambda: lpips_ops.head(f[2], fy[2], ops.lin[2], want_grad=True),
            'head5_grad': lambda: lpips_ops.head(f[4], fy[4], ops.lin[4], want_grad=True, relu_mask=True),
            'dgrad5': lambda: ops.dgrad[4].run(heads[4], f[3].shape[2:], act=f[3], slope=ops.zeros[256], addend=heads[3]),
            'dgrad4': lambda: ops.dgrad[3].run(heads[3], f[2].shape[2:], act=f[2], slope=ops.zeros[384], addend=heads[2]),
            'dgrad3': lambda: ops.dgrad[2].run(heads[2], f[2].shape[2:]),
            'pool2_bwd': lambda: lpips_ops.maxpool3s2_bwd(f[1], dp[1], addend=heads[1], relu_mask=True),
            'dgrad2_5x5_192_64': lambda: ops.dgrad[1].run(heads[1]),
            'pool1_bwd': lambda: lpips_ops.maxpool3s2_bwd(f[0], dp[0], addend=heads[0], relu_mask=True, out=ring[:, :, 1:-1, 1:-1]),
            'dgrad1': lambda: ops.dgrad[0].run(ring, (oh + 2, ow + 2)),
            'prepare_bwd': lambda: lpips_ops.prepare_bwd(dcanvas, (a.size, a.size), ops.mean, ops.std),
        }
        res['kernel_us'] = {}
        for name, fn in kernels.items():
            t, _ = alternate(fn, lambda: None, a.reps, a.warmup)
            res['kernel_us'][name] = [v * 1e3 for v in t]

        # the library's convolutions on the same operands, layer by layer (forward only)
        import torch.nn.functional as F
        convs = [m.net.layers[i] for i in (0, 3, 6, 8, 10)]
        z = m.net.z_score(xd)
        lib_in = [z, p1, p2, f[2], f[3]]
        res['torch_conv_forward_us'] = {}
        with torch.backends.cudnn.flags(enabled=True):
            for i, (c, inp) in enumerate(zip(convs, lib_in)):
                fn = lambda c=c, inp=inp: F.relu(c(inp))          # noqa: E731
                t, _ = alternate(fn, lambda: None, a.reps, a.warmup)
                res['torch_conv_forward_us'][f'conv{i + 1}_relu'] = [v * 1e3 for v in t]

    if not a.no_pti:
        from helpers import build_product_generator
        from inversion.scripts.run_pti_images import PTI, default_opts, tuning_optimizer
        from synth_weights import synth_ws
        G = build_product_generator('T1024', device=DEV)
        G.requires_grad_(True)
        opt = tuning_optimizer(PTI.tunable_parameters(G), 3e-4)
        ws = torch.from_numpy(synth_ws(1, G.num_ws, G.w_dim, 1)).to(DEV)
        target = cases.images(1, G.img_resolution, G.img_resolution, seed=3).to(DEV)
        plain = PTI(default_opts(device=DEV, lpips_lambda=0.0))
        full = PTI(default_opts(device=DEV), lpips_loss=m)

        def pti_step(pti):
            out = G.synthesis(ws, noise_mode='const', force_fp32=True)
            loss = pti.calc_loss(out, target)[0]
            opt.zero_grad()
            loss.backward()
            opt.step()

        pti_step(full)
        res['pti_t1024_mse_ms'], res['pti_t1024_mse_lpips_ms'] = alternate(lambda: pti_step(plain), lambda: pti_step(full), a.reps, a.warmup)

    def rnd(v):
        if isinstance(v, float):
            return round(v, 4)
        if isinstance(v, list):
            return [rnd(q) for q in v]
        return {k: rnd(q) for k, q in v.items()} if isinstance(v, dict) else v
    print(json.dumps({k: rnd(v) for k, v in res.items()}))


if __name__ == '__main__':
    main()
