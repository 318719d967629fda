"""Recorder of every filtered_lrelu call of one pivotal-tuning step (force_fp32, MSE; `synth_ws` seed 3), shared by the CPU and
GPU tests of tests/flrelu_ref.py: per layer the call's inputs, output, sign tensor, dy, and the dx / db its backward returned."""
import torch

from synth_weights import synth_ws


def setup_kwargs(e):
    return dict(up=e['up'], down=e['down'], padding=e['padding'], gain=e['gain'], slope=e['slope'], clamp=e['clamp'], flip=False)


def record_step(cfg, n, device, impl='cuda'):
    """-> (layer names, {name: dict(x, b, fu, fd, up, down, padding, gain, slope, clamp, y, signs, dy, dx, db)}).  `signs` is None
    where the call kept none (impl='ref')."""
    from helpers import build_product_generator
    from torch_utils.ops import filtered_lrelu as fl
    G = build_product_generator(cfg, device=device)
    ws = torch.from_numpy(synth_ws(n, G.num_ws, G.w_dim, seed=3)).to(device)
    with torch.no_grad():
        ref_img = G.synthesis(ws, noise_mode='const', force_fp32=True)
    target = (0.5 * ref_img + 0.1).detach()
    G.requires_grad_(True)
    params = list(G.synthesis.parameters())
    names = list(G.synthesis.layer_names)
    rec, order = {}, []
    orig = fl.filtered_lrelu

    def recording(x, fu=None, fd=None, b=None, up=1, down=1, padding=0, gain=2 ** 0.5, slope=0.2, clamp=None, flip_filter=False, impl_=impl):
        if not torch.is_grad_enabled():
            return orig(x=x, fu=fu, fd=fd, b=b, up=up, down=down, padding=padding, gain=gain, slope=slope, clamp=clamp,
                        flip_filter=flip_filter, impl=impl_)
        assert not flip_filter
        name = names[len(order)]
        order.append(name)
        e = rec[name] = dict(x=x.detach(), b=b.detach(), fu=fu, fd=fd, up=int(up), down=int(down), padding=list(padding),
                             gain=float(gain), slope=float(slope), clamp=clamp)
        xv, bv = x.view_as(x), b.view_as(b)        # own autograd nodes: their gradients are exactly what this call's backward returned
        xv.register_hook(lambda g: e.__setitem__('dx', g))
        bv.register_hook(lambda g: e.__setitem__('db', g))
        y = orig(x=xv, fu=fu, fd=fd, b=bv, up=up, down=down, padding=padding, gain=gain, slope=slope, clamp=clamp,
                 flip_filter=flip_filter, impl=impl_)
        saved = getattr(y.grad_fn, 'saved_tensors', ()) if impl_ == 'cuda' and x.is_cuda else ()
        e['signs'] = saved[2] if len(saved) == 3 and saved[2].dtype == torch.uint8 else None
        e['y'] = y.detach()
        y.register_hook(lambda g: e.__setitem__('dy', g))
        return y

    fl.filtered_lrelu = recording
    try:
        out = G.synthesis(ws, noise_mode='const', force_fp32=True)
        loss = torch.nn.functional.mse_loss(out, target)
        torch.autograd.grad(loss, params)
    finally:
        fl.filtered_lrelu = orig
    assert order == names, order
    for nm in names:
        assert all(k in rec[nm] for k in ('dx', 'db', 'dy')), nm
    return names, rec
