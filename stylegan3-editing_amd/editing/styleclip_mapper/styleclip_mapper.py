"""StyleCLIPMapper: a latent mapper plus the package's StyleGAN3 decoder (reference editing/styleclip_mapper/styleclip_mapper.py).

The mapper's weights come from a training checkpoint under the `mapper.` prefix, optionally inside 'state_dict' (`get_keys`,
reference :8-13), and load with strict=True (:39-43).
"""
import torch
from torch import nn

from editing.styleclip_mapper import latent_mappers
from models.stylegan3.model import SG3Generator


def get_keys(d, name):
    """Entries of `d` (or of d['state_dict']) whose key starts with `name`, with `name.` stripped."""
    if 'state_dict' in d:
        d = d['state_dict']
    return {k[len(name) + 1:]: v for k, v in d.items() if k[:len(name)] == name}


class StyleCLIPMapper(nn.Module):

    def __init__(self, opts):
        super().__init__()
        self.opts = opts
        self.mapper = self.set_mapper()
        self.decoder = SG3Generator(opts.stylegan_weights, res=opts.stylegan_size).decoder
        self.face_pool = torch.nn.AdaptiveAvgPool2d((256, 256))
        self.load_weights()

    def set_mapper(self):
        if self.opts.mapper_type == 'SingleMapper':
            return latent_mappers.SingleMapper(self.opts)
        if self.opts.mapper_type == 'LevelsMapper':
            return latent_mappers.LevelsMapper(self.opts)
        raise Exception(f'{self.opts.mapper_type} is not a valid mapper')

    def load_weights(self):
        if self.opts.checkpoint_path is not None:
            print(f'Loading from checkpoint: {self.opts.checkpoint_path}')
            ckpt = torch.load(self.opts.checkpoint_path, map_location='cpu', weights_only=False)
            self.mapper.load_state_dict(get_keys(ckpt, 'mapper'), strict=True)

    def forward(self, x, input_code=False):
        return x if input_code else self.mapper(x)
