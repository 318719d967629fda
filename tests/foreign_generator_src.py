"""Stand-in for the module source inside an official StyleGAN3 pickle.  TEXT ONLY: the tests read this file and hand it
to torch_utils.persistence as `module_src`; nothing imports it.

Written for the tests, compactly, against the upstream class names, constructor arguments and parameter / buffer
names.  Its forward uses the public operator API alone -- `filtered_lrelu`, `bias_act`, `conv2d_gradfix.conv2d(groups=N)`,
`misc`, `persistence` -- which is what a foreign pickle's graph reaches in this package.  Filter taps and layer sizes
come from this package's `design_lowpass_filter` / `synthesis_schedule`.  c_dim = 0, the W path and fp32 only.
tests/test_checkpoint_pkl_cpu.py pins it to the reference's images in tests/golden/net_tiny.npz.
"""
import numpy as np
import torch

from models.stylegan3.networks_stylegan3 import design_lowpass_filter, synthesis_schedule
from torch_utils import misc, persistence
from torch_utils.ops import bias_act, conv2d_gradfix, filtered_lrelu


def _rms(t, dims=None):
    """Root mean square over `dims` (all of them when None), kept for broadcasting."""
    return t.pow(2).mean().sqrt() if dims is None else t.pow(2).mean(dim=dims, keepdim=True).sqrt()


def modulated_conv2d(x, w, s, demodulate=True, padding=0, input_gain=None):
    """Sample n is convolved with its own kernel  k[n,o,i] = w[o,i] * s[n,i]  (times input_gain[i]).  With `demodulate`, w and s are
    first brought to unit RMS and every k[n,o] is divided by its Euclidean norm.  The N kernels run as one grouped convolution:
    samples stacked along the channel axis, one group per sample."""
    n, c_in, height, width = x.shape
    c_out = w.shape[0]
    if demodulate:
        w, s = w / _rms(w, [1, 2, 3]), s / _rms(s)
    kernels = torch.einsum('oikl,ni->noikl', w, s)
    if demodulate:
        kernels = kernels / (kernels.pow(2).sum(dim=[2, 3, 4], keepdim=True) + 1e-8).sqrt()
    if input_gain is not None:
        kernels = kernels * input_gain.expand(n, c_in)[:, None, :, None, None]
    stacked = conv2d_gradfix.conv2d(input=x.reshape(1, n * c_in, height, width), weight=kernels.flatten(0, 1).to(x.dtype),
                                    padding=padding, groups=n)
    return stacked.unflatten(1, (n, c_out)).squeeze(0)


@persistence.persistent_class
class FullyConnectedLayer(torch.nn.Module):
    """act(x W^T g_w + b g_b) with the equalised-learning-rate gains g_w = lr_multiplier / sqrt(in_features), g_b = lr_multiplier;
    the stored parameters are the trained values divided by lr_multiplier."""

    def __init__(self, in_features, out_features, activation='linear', bias=True, lr_multiplier=1, weight_init=1, bias_init=0):
        super().__init__()
        self.activation, self.lr_multiplier, self.fan_in = activation, float(lr_multiplier), in_features
        self.weight = torch.nn.Parameter(torch.randn(out_features, in_features) * weight_init / lr_multiplier)
        self.bias = None
        if bias:
            start = torch.as_tensor(bias_init, dtype=torch.float32).expand(out_features)
            self.bias = torch.nn.Parameter(start / lr_multiplier)

    def forward(self, x):
        weight = self.weight.to(x.dtype) * (self.lr_multiplier / np.sqrt(self.fan_in))
        bias = None if self.bias is None else self.bias.to(x.dtype) * self.lr_multiplier
        if self.activation == 'linear':
            return torch.nn.functional.linear(x, weight, bias)
        return bias_act.bias_act(torch.nn.functional.linear(x, weight), bias, act=self.activation)


@persistence.persistent_class
class MappingNetwork(torch.nn.Module):
    def __init__(self, z_dim, c_dim, w_dim, num_ws, num_layers=2, lr_multiplier=0.01, w_avg_beta=0.998):
        super().__init__()
        assert c_dim == 0
        self.z_dim, self.c_dim, self.w_dim, self.num_ws, self.num_layers = z_dim, c_dim, w_dim, num_ws, num_layers
        for i in range(num_layers):
            setattr(self, f'fc{i}', FullyConnectedLayer(z_dim if i == 0 else w_dim, w_dim, activation='lrelu', lr_multiplier=lr_multiplier))
        self.register_buffer('w_avg', torch.zeros([w_dim]))

    def forward(self, z, c, truncation_psi=1, truncation_cutoff=None, update_emas=False):
        misc.assert_shape(z, [None, self.z_dim])
        z = z.to(torch.float32)
        w = z / (z.pow(2).mean(dim=1, keepdim=True) + 1e-8).sqrt()
        for i in range(self.num_layers):
            w = getattr(self, f'fc{i}')(w)
        ws = w[:, None, :].expand(-1, self.num_ws, -1)
        if truncation_psi == 1:
            return ws.contiguous()
        # the first `truncation_cutoff` copies (all of them by default) are pulled towards the running mean of w
        pulled = torch.arange(self.num_ws, device=ws.device) < (self.num_ws if truncation_cutoff is None else truncation_cutoff)
        return torch.where(pulled[None, :, None], self.w_avg + truncation_psi * (ws - self.w_avg), ws)


@persistence.persistent_class
class SynthesisInput(torch.nn.Module):
    """Fourier features  sin(2 pi (f_c . p + phi_c))  at the pixel centres p of a size[0] x size[1] canvas sampled at `sampling_rate`,
    mixed by `weight / sqrt(channels)`.  Frequencies and phases are first carried through  M = R(w) T(w) U:  U the `transform`
    buffer, R / T the rotation and translation predicted from w by `affine` (rotation part normalised).  A frequency pushed
    beyond `bandwidth` fades out linearly and is gone at the Nyquist rate."""

    def __init__(self, w_dim, channels, size, sampling_rate, bandwidth):
        super().__init__()
        self.channels, self.size = channels, [int(v) for v in np.broadcast_to(np.asarray(size), [2])]
        self.sampling_rate, self.bandwidth = float(sampling_rate), float(bandwidth)
        angle, radius = torch.rand(channels) * (2 * np.pi), torch.rand(channels).sqrt() * bandwidth      # uniform over the disc
        self.weight = torch.nn.Parameter(torch.randn([channels, channels]))
        self.affine = FullyConnectedLayer(w_dim, 4, weight_init=0, bias_init=[1, 0, 0, 0])
        self.register_buffer('transform', torch.eye(3))
        self.register_buffer('freqs', torch.stack([radius * angle.cos(), radius * angle.sin()], dim=1))
        self.register_buffer('phases', torch.rand(channels) - 0.5)

    def forward(self, w):
        t = self.affine(w)
        cos, sin, dx, dy = (t / t[:, :2].norm(dim=1, keepdim=True)).unbind(1)
        rotation = torch.stack([torch.stack([cos, -sin], 1), torch.stack([sin, cos], 1)], 1)              # [N,2,2]
        shift = torch.stack([dx, dy], 1)
        top = torch.cat([rotation, -(rotation @ shift.unsqueeze(2))], dim=2)                                # R T = [R | -R d]
        bottom = torch.tensor([0.0, 0.0, 1.0], device=w.device).expand(w.shape[0], 1, 3)
        m = torch.cat([top, bottom], dim=1) @ self.transform
        freqs = self.freqs @ m[:, :2, :2]                                                                   # [N,C,2]
        phases = self.phases + (self.freqs @ m[:, :2, 2:]).squeeze(2)                                       # [N,C]
        nyquist = self.sampling_rate / 2
        amps = ((nyquist - freqs.norm(dim=2)) / (nyquist - self.bandwidth)).clamp(0, 1)
        # pixel centres, in units of 1 / sampling_rate, origin in the middle of the canvas
        px, py = ((torch.arange(n, device=w.device, dtype=torch.float64) + 0.5 - n / 2) / self.sampling_rate for n in self.size)
        px, py = px.to(torch.float32), py.to(torch.float32)
        cycles = (px[None, None, None, :] * freqs[:, :, 0, None, None] + py[None, None, :, None] * freqs[:, :, 1, None, None]
                  + phases[:, :, None, None])                                                               # [N,C,H,W]
        features = torch.sin(cycles * (2 * np.pi)) * amps[:, :, None, None]
        return torch.einsum('nchw,oc->nohw', features, self.weight / np.sqrt(self.channels))


@persistence.persistent_class
class SynthesisLayer(torch.nn.Module):
    def __init__(self, w_dim, is_torgb, is_critically_sampled, use_fp16, in_channels, out_channels, in_size, out_size,
                 in_sampling_rate, out_sampling_rate, in_cutoff, out_cutoff, in_half_width, out_half_width,
                 conv_kernel=3, filter_size=6, lrelu_upsampling=2, use_radial_filters=False, conv_clamp=256, magnitude_ema_beta=0.999,
                 standin_only=None):
        super().__init__()
        self.is_torgb, self.in_channels, self.conv_clamp = is_torgb, in_channels, conv_clamp
        self.conv_kernel = k = 1 if is_torgb else conv_kernel
        in_size, out_size = (np.broadcast_to(np.asarray(v), [2]) for v in (in_size, out_size))
        self.in_size, self.out_size, self.out_channels = in_size, out_size, out_channels
        work_rate = max(in_sampling_rate, out_sampling_rate) * (1 if is_torgb else lrelu_upsampling)
        self.affine = FullyConnectedLayer(w_dim, in_channels, bias_init=1)
        self.weight = torch.nn.Parameter(torch.randn([out_channels, in_channels, k, k]))
        self.bias = torch.nn.Parameter(torch.zeros([out_channels]))
        self.register_buffer('magnitude_ema', torch.ones([]))
        self.up = int(np.rint(work_rate / in_sampling_rate))
        self.down = int(np.rint(work_rate / out_sampling_rate))
        up_taps = filter_size * self.up if self.up > 1 and not is_torgb else 1
        down_taps = filter_size * self.down if self.down > 1 and not is_torgb else 1
        self.register_buffer('up_filter', design_lowpass_filter(up_taps, in_cutoff, in_half_width * 2, work_rate))
        self.register_buffer('down_filter', design_lowpass_filter(down_taps, out_cutoff, out_half_width * 2, work_rate,
                                                                  radial=use_radial_filters and not is_critically_sampled))
        # samples the filters and the convolution consume beyond what out_size needs, split with the odd one in front
        spare = (out_size - 1) * self.down + 1 - (in_size + k - 1) * self.up + up_taps + down_taps - 2
        front = (spare + self.up) // 2
        self.padding = [int(front[0]), int(spare[0] - front[0]), int(front[1]), int(spare[1] - front[1])]
        # EXTRA_BUFFER_HOOK

    def forward(self, x, w):
        misc.assert_shape(x, [None, self.in_channels, int(self.in_size[1]), int(self.in_size[0])])
        styles = self.affine(w)
        if self.is_torgb:
            styles = styles * (1 / np.sqrt(self.in_channels * self.conv_kernel ** 2))
        x = modulated_conv2d(x.to(torch.float32), self.weight, styles, demodulate=not self.is_torgb, padding=self.conv_kernel - 1,
                             input_gain=self.magnitude_ema.rsqrt())
        return filtered_lrelu.filtered_lrelu(x=x, fu=self.up_filter, fd=self.down_filter, b=self.bias.to(x.dtype), up=self.up, down=self.down,
                                             padding=self.padding, gain=(1 if self.is_torgb else np.sqrt(2)),
                                             slope=(1 if self.is_torgb else 0.2), clamp=self.conv_clamp)


@persistence.persistent_class
class SynthesisNetwork(torch.nn.Module):
    def __init__(self, w_dim, img_resolution, img_channels, channel_base=32768, channel_max=512, num_layers=14, num_critical=2,
                 first_cutoff=2, first_stopband=2 ** 2.1, last_stopband_rel=2 ** 0.3, margin_size=10, output_scale=0.25,
                 num_fp16_res=4, **layer_kwargs):
        super().__init__()
        self.w_dim, self.num_ws, self.output_scale = w_dim, num_layers + 2, output_scale
        self.img_resolution, self.img_channels = img_resolution, img_channels
        input_spec, table = synthesis_schedule(
            img_resolution, img_channels, channel_base=channel_base, channel_max=channel_max, num_layers=num_layers,
            num_critical=num_critical, first_cutoff=first_cutoff, first_stopband=first_stopband,
            last_stopband_rel=last_stopband_rel, margin_size=margin_size, num_fp16_res=num_fp16_res)
        self.input = SynthesisInput(w_dim=w_dim, **input_spec)
        self.layer_names = []
        for g in table:
            kw = {k: v for k, v in g._asdict().items() if k != 'index'}
            name = f'L{g.index}_{g.out_size}_{g.out_channels}'
            setattr(self, name, SynthesisLayer(w_dim=w_dim, **kw, **layer_kwargs))
            self.layer_names.append(name)

    def forward(self, ws, **_unused):
        misc.assert_shape(ws, [None, self.num_ws, self.w_dim])
        ws = ws.to(torch.float32).unbind(dim=1)
        x = self.input(ws[0])
        for name, w in zip(self.layer_names, ws[1:]):
            x = getattr(self, name)(x, w)
        if self.output_scale != 1:
            x = x * self.output_scale
        misc.assert_shape(x, [None, self.img_channels, self.img_resolution, self.img_resolution])
        return x.to(torch.float32)


@persistence.persistent_class
class Generator(torch.nn.Module):
    def __init__(self, z_dim, c_dim, w_dim, img_resolution, img_channels, mapping_kwargs={}, **synthesis_kwargs):
        super().__init__()
        self.z_dim, self.c_dim, self.w_dim = z_dim, c_dim, w_dim
        self.img_resolution, self.img_channels = img_resolution, img_channels
        self.synthesis = SynthesisNetwork(w_dim=w_dim, img_resolution=img_resolution, img_channels=img_channels, **synthesis_kwargs)
        self.num_ws = self.synthesis.num_ws
        self.mapping = MappingNetwork(z_dim=z_dim, c_dim=c_dim, w_dim=w_dim, num_ws=self.num_ws, **mapping_kwargs)

    def forward(self, z, c, truncation_psi=1, truncation_cutoff=None, update_emas=False, **synthesis_kwargs):
        ws = self.mapping(z, c, truncation_psi=truncation_psi, truncation_cutoff=truncation_cutoff)
        return self.synthesis(ws, **synthesis_kwargs)
