"""Stand-in for the module sources next to `G_ema` in an upstream training snapshot (`D`, `augment_pipe`).  TEXT ONLY:
the tests hand it to torch_utils.persistence as `module_src`; nothing imports it.

What matters is the import line: upstream's discriminator source imports `conv2d_resample` and `fma`, its augmentation
source imports `grid_sample_gradfix`, all by name from `torch_utils.ops`, and that happens while the snapshot is
unpickled -- before anybody asks for `G_ema`.  The few layers below call each of the three once.
"""
import numpy as np
import torch

from torch_utils import misc, persistence
from torch_utils.ops import bias_act, conv2d_resample, fma, grid_sample_gradfix, upfirdn2d


@persistence.persistent_class
class Conv2dLayer(torch.nn.Module):
    def __init__(self, in_channels, out_channels, kernel_size, up=1, down=1, resample_filter=[1, 3, 3, 1]):
        super().__init__()
        self.up, self.down, self.padding = up, down, kernel_size // 2
        self.register_buffer('resample_filter', upfirdn2d.setup_filter(resample_filter))
        self.weight = torch.nn.Parameter(torch.randn([out_channels, in_channels, kernel_size, kernel_size]))
        self.bias = torch.nn.Parameter(torch.zeros([out_channels]))
        self.weight_gain = 1 / np.sqrt(in_channels * kernel_size ** 2)

    def forward(self, x):
        x = conv2d_resample.conv2d_resample(x=x, w=(self.weight * self.weight_gain).to(x.dtype), f=self.resample_filter, up=self.up,
                                            down=self.down, padding=self.padding, flip_weight=(self.up == 1))
        return bias_act.bias_act(x, self.bias.to(x.dtype), act='lrelu')


@persistence.persistent_class
class Discriminator(torch.nn.Module):
    def __init__(self, c_dim, img_resolution, img_channels, channels=8):
        super().__init__()
        self.c_dim, self.img_resolution, self.img_channels = c_dim, img_resolution, img_channels
        self.fromrgb = Conv2dLayer(img_channels, channels, kernel_size=1)
        self.conv0 = Conv2dLayer(channels, channels, kernel_size=3)
        self.conv1 = Conv2dLayer(channels, channels, kernel_size=3, down=2)
        self.out = torch.nn.Linear(channels, 1)
        self.register_buffer('noise_strength', torch.full([], 0.1))

    def forward(self, img, c=None, **_unused):
        misc.assert_shape(img, [None, self.img_channels, self.img_resolution, self.img_resolution])
        n = img.shape[0]
        # a half-texel shift through the sampler, as the augmentation pipeline's geometric transforms do
        theta = torch.eye(2, 3, device=img.device).unsqueeze(0).repeat([n, 1, 1])
        theta[:, 0, 2] = 1 / self.img_resolution
        grid = torch.nn.functional.affine_grid(theta, list(img.shape), align_corners=False)
        x = grid_sample_gradfix.grid_sample(img, grid)
        x = self.conv1(self.conv0(self.fromrgb(x)))
        x = fma.fma(x, self.noise_strength.to(x.dtype), x.mean(dim=[2, 3], keepdim=True))
        return self.out(x.mean(dim=[2, 3]))
