"""GPU: the image-finishing kernel (csrc/sg3_image_finish.hip) against tensor2im + PIL on the same tensors, bit for bit, and
InterFaceGAN editing on the MI355X: the reference fixture, the CPU oracle, the per-factor loop at R-1024 and run_editing's strips."""
import types

import numpy as np
import pytest
import torch

import interfacegan_cases as cases
from helpers import build_oracle_generator, build_product_generator, build_restyle_pair, golden, maxabs
from test_image_finish_cpu import SIZES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def pil_finish(x, size=None):
    """The definition: np.array(tensor2im(x[b]).resize(size)) per image."""
    from utils.common import tensor2im
    out = []
    for i in range(x.shape[0]):
        im = tensor2im(x[i])
        if size is not None and tuple(size) != im.size:
            im = im.resize(tuple(size))
        out.append(np.array(im))
    return np.stack(out)


def images(b, h, w, seed):
    r = np.random.RandomState(seed)
    x = r.uniform(-1.3, 1.3, size=(b, 3, h, w)).astype(np.float32)
    k = r.randint(0, 256, size=x.size // 3)
    edges = (k / 255.0 * 2 - 1).astype(np.float32)                                   # values on k / 255 boundaries
    flat = x.reshape(-1)
    idx = r.choice(flat.size, size=edges.size, replace=False)
    flat[idx] = edges
    flat[idx[: edges.size // 4]] = np.nextafter(edges[: edges.size // 4], np.float32(2))
    x[:, :, : h // 4, : w // 3] = 1.0                                                  # saturated blocks: overshoot into the clamps
    x[:, :, h // 2:, w // 2:] = -1.0
    return x


@pytest.mark.parametrize('src,dst', SIZES)
def test_kernel_equals_tensor2im_and_pil(src, dst):
    from torch_utils.ops.image_finish import to_uint8
    x = images(6, src[1], src[0], seed=src[0] + dst[0])
    got = to_uint8(torch.from_numpy(x).to(DEV), dst).cpu().numpy()
    ref = pil_finish(torch.from_numpy(x), dst)
    assert got.shape == ref.shape
    assert np.array_equal(got, ref), int(np.abs(got.astype(int) - ref).max())


@pytest.mark.parametrize('src,dst', [((1024, 1024), (256, 256)), ((256, 256), (1024, 1024)), ((1024, 1024), (1024, 1024)),
                                     ((512, 384), (256, 192))])
def test_kernel_strided_input_and_strip_output(src, dst):
    """Input: a strided slice of a larger batch (odd column offset: the scalar load path, and every other image); output: the
    columns of a wider strip."""
    from torch_utils.ops.image_finish import to_uint8
    big = torch.from_numpy(images(10, src[1], src[0] + 3, seed=5)).to(DEV)
    x = big[1:9:2, :, :, 3:]
    w, h = dst
    strip = torch.full([4, h, 3 * w, 3], 7, dtype=torch.uint8, device=DEV)
    out = to_uint8(x, dst, out=strip[:, :, w:2 * w])
    assert out.data_ptr() == strip[:, :, w:2 * w].data_ptr()
    ref = pil_finish(x.cpu(), dst)
    s = strip.cpu().numpy()
    assert np.array_equal(s[:, :, w:2 * w], ref)
    assert (s[:, :, :w] == 7).all() and (s[:, :, 2 * w:] == 7).all()
    # a channels-last input (stride-1 channels, x stride 3) takes the scalar path as well
    xc = big[:4, :, :, :src[0]].contiguous(memory_format=torch.channels_last)
    assert np.array_equal(to_uint8(xc, dst).cpu().numpy(), pil_finish(xc.cpu(), dst))


def test_kernel_batch_120():
    from torch_utils.ops.image_finish import to_uint8
    x = torch.from_numpy(images(120, 1024, 1024, seed=9)).to(DEV)
    got = to_uint8(x, (256, 256)).cpu().numpy()
    assert np.array_equal(got, pil_finish(x.cpu(), (256, 256)))


def test_op_errors():
    from torch_utils.ops.image_finish import to_uint8
    x = torch.zeros([2, 3, 8, 8], device=DEV)
    with pytest.raises(RuntimeError, match='out'):
        to_uint8(x, (4, 4), out=torch.zeros([2, 4, 4, 3], dtype=torch.float32, device=DEV))
    with pytest.raises(RuntimeError, match='out'):
        to_uint8(x, (4, 4), out=torch.zeros([2, 4, 5, 3], dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match='x must be'):
        to_uint8(torch.zeros([2, 4, 8, 8], device=DEV))
    with pytest.raises(RuntimeError, match='x must be'):
        to_uint8(torch.zeros([2, 3, 8, 8], dtype=torch.int32, device=DEV))


def oracle_loop(cfg, lat, d, factors, transform, mixed=False):
    from oracle import oracle as O
    sd, sched = build_oracle_generator(cfg)
    t = transform.cpu().numpy()
    return np.stack([O.synthesis(sd, sched, ws=(lat + f * d).cpu().numpy(), transform=t, mixed_fp16=mixed) for f in factors])


@pytest.mark.parametrize('cfg', ['Ttiny', 'Rtiny'])
def test_face_editor_against_fixture_and_oracle(cfg):
    from editing.interfacegan.face_editor import FaceEditor
    gold = golden('interfacegan')
    G = build_product_generator(cfg, device=DEV)
    editor = FaceEditor(G, directions=cases.directions(G.w_dim), max_batch=3)
    lat = torch.from_numpy(cases.latents(G.num_ws, G.w_dim)).to(DEV)
    lm = torch.from_numpy(cases.landmarks()).to(DEV)
    for case in cases.CASES:
        if case['seed'] is not None:
            np.random.seed(case['seed'])
        imgs, _ = editor.edit(lat, force_fp32=True, **cases.edit_kwargs(case, lm))
        got = np.stack([np.stack([np.array(im) for im in step]) for step in (imgs if 'factor_range' in case else [imgs])])
        ref = gold[f'ig/{cfg}/{case["key"]}/images']
        assert np.abs(got.astype(int) - ref).max() <= 1, case['key']
        assert np.array_equal(G.synthesis.input.transform.cpu().numpy(), gold[f'ig/{cfg}/{case["key"]}/transform'])
    d = editor.interfacegan_directions['age']
    out, _ = editor.edit_tensors(lat, 'age', factor_range=(-2, 2), user_transforms=lm, apply_user_transformations=True, force_fp32=True)
    assert maxabs(out.cpu().numpy(), oracle_loop(cfg, lat, d, range(-2, 2), lm)) <= 1e-4
    mixed, _ = editor.edit_tensors(lat, 'age', factor_range=(-2, 2), user_transforms=lm, apply_user_transformations=True)
    assert maxabs(mixed.cpu().numpy(), oracle_loop(cfg, lat, d, range(-2, 2), lm, mixed=True)) <= 2e-3


def test_r1024_sweep_and_strips():
    """README command's shape at full size: N = 4, factors range(-5, 5), [4,3,3] landmark transforms, max_batch 16."""
    from editing.interfacegan.face_editor import FaceEditor
    from torch_utils.ops.image_finish import to_uint8
    G = build_product_generator('R1024', device=DEV)
    editor = FaceEditor(G, directions=cases.directions(G.w_dim, scale=0.5), max_batch=16)
    lat = torch.from_numpy(cases.latents(G.num_ws, G.w_dim, n=4)).to(DEV)
    lm = torch.from_numpy(np.concatenate([cases.landmarks(), cases.landmarks()])).to(DEV)
    imgs, _ = editor.edit_tensors(lat, 'age', factor_range=(-5, 5), user_transforms=lm, apply_user_transformations=True, force_fp32=True)
    assert tuple(imgs.shape) == (10, 4, 3, 1024, 1024)
    d = editor.interfacegan_directions['age']
    G.synthesis.input.transform = lm
    with torch.no_grad():
        for k, f in enumerate(range(-5, 5)):
            ref = G.synthesis(lat + f * d, noise_mode='const', force_fp32=True)
            assert maxabs(imgs[k].cpu().numpy(), ref.cpu().numpy()) <= 1e-5, f
    for s in (256, 1024):
        strip = torch.empty([4, s, 10 * s, 3], dtype=torch.uint8, device=DEV)
        for k in range(10):
            to_uint8(imgs[k], (s, s), out=strip[:, :, k * s:(k + 1) * s])
        host = imgs.cpu()
        ref = np.concatenate([pil_finish(host[k], (s, s)) for k in range(10)], axis=2)
        assert np.array_equal(strip.cpu().numpy(), ref), s


@pytest.mark.parametrize('resize_outputs', [False, True])
def test_run_editing_end_to_end(tmp_path, resize_outputs):
    from PIL import Image
    from editing.interfacegan.face_editor import FaceEditor
    from inversion.scripts import inference_editing as ie
    from utils.common import tensor2im
    net, opts, *_ = build_restyle_pair('Rmini', device=DEV, n_iters=2)
    opts = types.SimpleNamespace(**vars(opts))
    opts.resize_outputs = resize_outputs
    opts.edit_directions, opts.factor_ranges = ['age', 'smile'], ['(-2_2)', (-1, 1)]
    x = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, size=(3, 3, 256, 256)).astype(np.float32))
    lm = torch.from_numpy(np.concatenate([cases.landmarks(), cases.landmarks(1)]))
    editor = FaceEditor(net.decoder, directions=cases.directions(512, scale=0.5))
    ie.run_editing(net, opts, x, ['a.png', 'b.png', 'c.png'], str(tmp_path), landmarks_transforms=lm, editor=editor, batch_size=2)
    s = 256 if resize_outputs else 64
    with torch.no_grad():
        avg = ie.get_average_image(net)
        xs, ls = x[2:].to(DEV), lm[2:].to(DEV)
        y_hat, latents = ie.get_inversions_on_batch(xs, net, avg, opts, landmarks_transform=ls)
        edits, _ = editor.edit_tensors(latents, 'age', factor_range=(-2, 2), apply_user_transformations=True, user_transforms=ls)
    tiles = [tensor2im(xs[0]), tensor2im(y_hat[0])] + [tensor2im(edits[k, 0]) for k in range(4)]
    ref = np.concatenate([np.array(t.resize((s, s))) for t in tiles], axis=1)
    got = np.array(Image.open(tmp_path / 'editing_results' / 'age' / 'c.png'))
    assert got.shape == (s, 6 * s, 3)
    assert np.array_equal(got, ref)
