"""Command-line options of mapper training (reference editing/styleclip_mapper/options/train_options.py): the reference's
arguments and defaults, plus `--clip_checkpoint_path` (the CLIP weights `criteria.clip_loss.CLIPLoss` loads) and `--text_tokens`
(a .npy / .pt file of token ids [n_text, context_length]: text arrives tokenised everywhere in this package)."""
from argparse import ArgumentParser


class TrainOptions:

    def __init__(self):
        self.parser = ArgumentParser()
        self.initialize()

    def initialize(self):
        p = self.parser
        p.add_argument('--exp_dir', type=str, help='Path to experiment output directory')
        p.add_argument('--mapper_type', default='LevelsMapper', type=str, help='Which mapper to use')
        p.add_argument('--no_coarse_mapper', default=False, action='store_true')
        p.add_argument('--no_medium_mapper', default=False, action='store_true')
        p.add_argument('--no_fine_mapper', default=False, action='store_true')
        p.add_argument('--latents_train_path', type=str, required=True, help='The latents for the training')
        p.add_argument('--latents_test_path', type=str, required=True, help='The latents for the validation')
        p.add_argument('--train_dataset_size', default=10000, type=int, help='Will be used only if no latents are given')
        p.add_argument('--test_dataset_size', default=1000, type=int, help='Will be used only if no latents are given')

        p.add_argument('--batch_size', default=2, type=int, help='Batch size for training')
        p.add_argument('--test_batch_size', default=1, type=int, help='Batch size for testing and inference')
        p.add_argument('--workers', default=4, type=int, help='Number of train dataloader workers')
        p.add_argument('--test_workers', default=1, type=int, help='Number of test/inference dataloader workers')

        p.add_argument('--learning_rate', default=0.5, type=float, help='Optimizer learning rate')
        p.add_argument('--optim_name', default='ranger', type=str, help='Which optimizer to use')

        p.add_argument('--id_lambda', default=0.06, type=float, help='ID loss multiplier factor')
        p.add_argument('--clip_lambda', default=1.0, type=float, help='CLIP loss multiplier factor')
        p.add_argument('--latent_l2_lambda', default=0.3, type=float, help='Latent L2 loss multiplier factor')

        p.add_argument('--stylegan_weights', default='/path/to/weights', type=str, help='Path to StyleGAN model weights')
        p.add_argument('--truncation_psi', default=0.7, type=int)
        p.add_argument('--stylegan_size', default=1024, type=int)
        p.add_argument('--ir_se50_weights', default='/path/to/model_ir_se50.pth', type=str,
                       help='Path to facial recognition network used in ID loss')
        p.add_argument('--checkpoint_path', default=None, type=str, help='Path to StyleCLIP model checkpoint')

        p.add_argument('--max_steps', default=50000, type=int, help='Maximum number of training steps')
        p.add_argument('--image_interval', default=100, type=int, help='Interval for logging train images during training')
        p.add_argument('--board_interval', default=50, type=int, help='Interval for logging metrics')
        p.add_argument('--val_interval', default=2000, type=int, help='Validation interval')
        p.add_argument('--save_interval', default=2000, type=int, help='Model checkpoint interval')

        p.add_argument('--description', required=True, type=str, help='Driving text prompt (kept in the checkpoint; see --text_tokens)')
        p.add_argument('--clip_checkpoint_path', default=None, type=str, help='Path to the CLIP ViT-B/32 weights')
        p.add_argument('--text_tokens', default=None, type=str, help='Path to the token ids of the prompt, [n_text, context_length]')

    def parse(self, args=None):
        return self.parser.parse_args(args)
