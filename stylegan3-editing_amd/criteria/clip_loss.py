"""The CLIP loss of StyleCLIP (reference criteria/clip_loss.py): 1 - logits_per_image / 100 between images and tokenised text.

The reference loads OpenAI's ViT-B/32 through the `clip` package and takes strings tokenised by it; here the model is given, or
loaded from `opts.clip_checkpoint_path` by `models.clip.load`, and `text` is token ids [n_text, context_length] as everywhere in
this package.  The image is prepared as the reference prepares it, nearest upsampling by 7 and average pooling by
stylegan_size // 32 (224 x 224 for every multiple of 32), by the fused `nearest_up_avg_pool`.  Text features are constants of the
loss (computed under no_grad); the gradient flows to the image.  On CUDA, with a tower the kernels support and no parameter of
the image tower recording a gradient, the image tower runs as impl='hip' forward and backward."""
import torch

from torch_utils.ops import clip_transformer
from torch_utils.ops.clip_resample import nearest_up_avg_pool


class CLIPLoss(torch.nn.Module):
    def __init__(self, opts, model=None):
        super().__init__()
        if model is None:
            from models.clip import load
            model = load(opts.clip_checkpoint_path, device='cuda' if torch.cuda.is_available() else 'cpu')
        self.model = model
        self.up = 7
        self.kernel_size = int(opts.stylegan_size) // 32
        if self.kernel_size < 1:
            raise ValueError(f'CLIPLoss: stylegan_size must be at least 32, got {opts.stylegan_size}')

    def _image_impl(self, image):
        """'hip' where CLIP.encode_image accepts it by name, else None (the model's own choice, which is the composite under autograd)."""
        m = self.model
        if not (image.is_cuda and m.impl in (None, 'hip') and clip_transformer.image_supported(m)):
            return None
        if not torch.is_grad_enabled() or not (image.requires_grad or any(q.requires_grad for q in m.parameters())):
            return 'hip'
        return 'hip' if image.requires_grad and not any(q.requires_grad for q in m.visual.parameters()) else None

    def forward(self, image, text):
        """image [B, 3, stylegan_size, stylegan_size], text token ids [n_text, context_length] -> [B, n_text]."""
        m = self.model
        image = nearest_up_avg_pool(image, self.up, self.kernel_size)
        image_features = m.encode_image(image, impl=self._image_impl(image))
        with torch.no_grad():
            text_features = m.encode_text(text).to(image_features.dtype)
            text_features = text_features / text_features.norm(dim=-1, keepdim=True)
            logit_scale = m.logit_scale.exp().to(image_features.dtype)
        image_features = image_features / image_features.norm(dim=-1, keepdim=True)
        logits_per_image = logit_scale * image_features @ text_features.t()
        return 1 - logits_per_image / 100
