"""Shared cases of the StyleCLIP delta_i_c tests and their fixture (tests/golden/make_golden_delta_i_c.py): the seeded StyleSpace
latents and statistics, the stand-in image encoder (CLIP weights are not available offline), the shapes of the preprocessing
tests and an fp64 restatement of the preprocessing that takes its coordinates in float32 as torch does."""
import numpy as np

CONFIGS = ('Ttiny', 'Rtiny')
NUM_SAMPLES = 2
NUM_STATS = 256
STRENGTH = 5
FEATURE_DIM = 16
SUBGRID = 7

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

# (B, H, W, h, w) of the preprocessing tests
SHAPES = [
    (1, 16, 16, 224, 224),        # upsampling, all four borders clamped
    (3, 37, 53, 224, 224),        # odd and non-square: catches swapped axes
    (2, 224, 224, 224, 224),      # identity scale
    (2, 256, 256, 224, 224),
    (1, 1024, 1024, 224, 224),    # the largest float32 coordinates
    (33, 64, 64, 31, 47),         # a batch beyond one grid row of any plausible launch shape, non-square output
]


def noise(shape, scale, seed=0):
    return (np.random.RandomState(1000 * seed + int(np.prod(shape)) % 997).randn(*shape) * scale).astype(np.float32)


def stats_latents(G, seed=3):
    """(S [NUM_SAMPLES rows per layer] float32, s_mean, s_std) as s_statistics.py computes them from NUM_STATS seeded z.  The
    statistics are widened to float64: the reference's loop assigns `mean[layer][channel] + direction * std[layer][channel]` to a
    tensor element, which the installed torch accepts from a numpy float64 scalar (a Python float) but not from a float32 one."""
    import torch
    z = np.random.RandomState(seed).randn(NUM_STATS, G.z_dim).astype(np.float32)
    with torch.no_grad():
        ws = G.mapping(z=torch.from_numpy(z), c=None, truncation_psi=0.7)
        all_s = {k: v.numpy() for k, v in G.synthesis.W2S(ws).items()}
    return ({k: v[:NUM_SAMPLES].copy() for k, v in all_s.items()}, {k: v.mean(axis=0).astype(np.float64) for k, v in all_s.items()},
            {k: v.std(axis=0).astype(np.float64) for k, v in all_s.items()})


def encoder_matrix(seed=77):
    """[192, FEATURE_DIM]; every column has unit L1 norm, so a feature moves by at most the largest pixel error."""
    m = np.random.RandomState(seed).randn(3 * 8 * 8, FEATURE_DIM)
    return (m / np.abs(m).sum(axis=0, keepdims=True)).astype(np.float32)


class StandInEncoder:
    """Stand-in for CLIP's image encoder: 8 x 8 average pooling, flatten, a fixed [192, 16] matrix.  Samples are independent."""

    def __init__(self):
        import torch
        self.matrix = torch.from_numpy(encoder_matrix())
        self.calls = []

    def __call__(self, images):
        import torch.nn.functional as F
        self.calls.append(int(images.shape[0]))
        return F.adaptive_avg_pool2d(images, 8).flatten(1) @ self.matrix.to(images.device)

    encode_image = __call__


def subgrid(images):
    """What the fixture keeps of [n,3,224,224] images: every SUBGRID-th pixel, the last row and the last column."""
    return images[:, :, ::SUBGRID, ::SUBGRID], images[:, :, -1, :], images[:, :, :, -1]


def load_case(g, cfg):
    """(latents_s, s_mean, s_std) of `cfg` from the fixture, numpy, in the fixture's layer order."""
    layers = [str(k) for k in g[f'{cfg}/layers']]
    return ({k: g[f'{cfg}/S/{k}'] for k in layers}, {k: g[f'{cfg}/mean/{k}'] for k in layers}, {k: g[f'{cfg}/std/{k}'] for k in layers})


def _taps64(n_in, n_out):
    """Indices [n_out, 4] and fp64 cubic-convolution weights [n_out, 4] (A = -0.75) from torch's float32 source coordinates."""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = (scale * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    fl = np.floor(src)
    t = (src - fl).astype(np.float32).astype(np.float64)
    a = -0.75

    def c1(x):
        return ((a + 2) * x - (a + 3)) * x * x + 1

    def c2(x):
        return ((a * x - 5 * a) * x + 8 * a) * x - 4 * a

    wts = np.stack([c2(t + 1), c1(t), c1(1 - t), c2(2 - t)], axis=1)
    idx = np.clip(fl.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, wts


def preprocess_ref64(x, size=(224, 224), mean=CLIP_MEAN, std=CLIP_STD):
    """fp64 restatement of the CLIP preprocessing: bicubic align_corners=True resize with t taken from float32 coordinates,
    (y + 1) / 2, clip to [0, 1], (y - mean) / std with the float32 constants."""
    x = np.asarray(x, dtype=np.float64)
    iy, wy = _taps64(x.shape[2], size[0])
    ix, wx = _taps64(x.shape[3], size[1])
    rows = (x[:, :, iy, :] * wy[None, None, :, :, None]).sum(axis=3)              # [B,3,h,W]
    y = (rows[:, :, :, ix] * wx[None, None, None, :, :]).sum(axis=4)              # [B,3,h,w]
    y = np.clip((y + 1) / 2, 0, 1)
    m = np.asarray(mean, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    s = np.asarray(std, dtype=np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    return (y - m) / s
