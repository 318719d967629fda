"""Command-line options of mapper inference (reference editing/styleclip_mapper/options/test_options.py)."""
from argparse import ArgumentParser


class TestOptions:

    def __init__(self):
        self.parser = ArgumentParser()
        self.initialize()

    def initialize(self):
        p = self.parser
        p.add_argument('--exp_dir', type=str, help='Path to experiment output directory')
        p.add_argument('--checkpoint_path', default=None, type=str, help='Path to model checkpoint')
        p.add_argument('--couple_outputs', action='store_true', help='Whether to also save inputs + outputs side-by-side')
        p.add_argument('--mapper_type', default='LevelsMapper', type=str, help='Which mapper to use')
        p.add_argument('--no_coarse_mapper', default=False, action='store_true')
        p.add_argument('--no_medium_mapper', default=False, action='store_true')
        p.add_argument('--no_fine_mapper', default=False, action='store_true')
        p.add_argument('--stylegan_size', default=1024, type=int)
        p.add_argument('--test_batch_size', default=2, type=int, help='Batch size for testing and inference')
        p.add_argument('--latents_test_path', default=None, type=str, help='The latents for the validation')
        p.add_argument('--test_workers', default=0, type=int, help='Number of test/inference dataloader workers')
        p.add_argument('--fourier_features_transforms_path', default=None, type=str, help='Optional path to transforms')
        p.add_argument('--n_images', type=int, default=None, help='Number of images to output. If None, run on all data')

    def parse(self, args=None):
        return self.parser.parse_args(args)
