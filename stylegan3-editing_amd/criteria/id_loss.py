"""The identity loss of the StyleCLIP mapper and the encoder coaches (reference criteria/id_loss.py): one minus the cosine between
the IR-SE50 (ArcFace) features of the edited image and those of the detached target.

The reference constructs `IDLoss()` and reads `model_paths['ir_se50']`; there is no `configs/` in this package, so the weights come
from `opts.ir_se50_weights` (a state_dict of `Backbone(112, 50, mode='ir_se')`; the network is frozen, `requires_grad_(False)`,
when loaded that way) or a ready `facenet` module is given and left as the caller set it.  The image is
prepared as the reference prepares it -- pool to 256 unless the height is 256 already, crop [35:223, 32:220], pool to 112 -- by the
fused `face_pool`.  `forward` keeps the reference's values, types and log keys, and gets there with less work: features of `x` and
`y` are constants of the loss (computed under no_grad, once when `y is x`, as in the coach's `id_loss(x_hat, x, x)`), and the
3 B dot products reach the host in one copy instead of 3 B synchronising `float()` calls.

On CUDA float32 input, with the facenet in eval mode, a 112 x 112 `Backbone` and no facenet parameter recording a gradient, the
network runs on libsg3hip, forward and backward (models/setgan/encoder/encoders/model_irse.py `features_hip`); otherwise it is
the composite under autograd -- the same rule as CLIPLoss._image_impl."""
import torch
from torch import nn

from models.setgan.encoder.encoders.model_irse import Backbone
from torch_utils.ops.face_pool import face_pool


class IDLoss(nn.Module):
    def __init__(self, opts=None, facenet=None):
        super().__init__()
        if facenet is None:
            path = getattr(opts, 'ir_se50_weights', None)
            if not path:
                raise ValueError('IDLoss: give the IR-SE50 weights as opts.ir_se50_weights, or a facenet module')
            print('Loading ResNet ArcFace')
            facenet = Backbone(input_size=112, num_layers=50, drop_ratio=0.6, mode='ir_se')
            state = torch.load(path, map_location='cpu')
            facenet.load_state_dict(state.get('state_dict', state) if isinstance(state, dict) else state)
            facenet.requires_grad_(False)          # the loss never trains it; frozen parameters are what the HIP path asks for
        self.facenet = facenet
        self.facenet.eval()

    def uses_hip(self, x):
        """Does `extract_feats(x)` take the HIP path?"""
        net = self.facenet
        return isinstance(net, Backbone) and x.is_cuda and x.dtype == torch.float32 and x.ndim == 4 and x.shape[1] == 3 and net.hip_ready()

    def extract_feats(self, x):
        hip = self.uses_hip(x)
        x = face_pool(x)
        return self.facenet.features_hip(x) if hip else self.facenet(x)

    def forward(self, y_hat, y, x):
        n_samples = x.shape[0]
        with torch.no_grad():
            x_feats = self.extract_feats(x)
            y_feats = x_feats if y is x else self.extract_feats(y)
        y_hat_feats = self.extract_feats(y_hat)
        diff_target = (y_hat_feats * y_feats).sum(dim=1)
        dots = torch.stack([diff_target.detach(), (y_hat_feats.detach() * x_feats).sum(dim=1), (y_feats * x_feats).sum(dim=1)]).cpu().tolist()
        id_logs = [{'diff_target': dots[0][i], 'diff_input': dots[1][i], 'diff_views': dots[2][i]} for i in range(n_samples)]
        sim_improvement = 0
        for i in range(n_samples):
            sim_improvement += dots[0][i] - dots[2][i]
        loss = (1 - diff_target).sum()
        return loss / n_samples, sim_improvement / n_samples, id_logs
