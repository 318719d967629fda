"""Mapper training entry point (reference editing/styleclip_mapper/scripts/train.py): make `exp_dir`, write `opt.json`, run
the Coach."""
import json
import os
import pprint
import sys

sys.path.append('.')
sys.path.append('..')

from editing.styleclip_mapper.options.train_options import TrainOptions  # noqa: E402
from editing.styleclip_mapper.training.coach import Coach  # noqa: E402


def main(opts):
    if os.path.exists(opts.exp_dir):
        raise Exception(f'Oops... {opts.exp_dir} already exists')
    os.makedirs(opts.exp_dir, exist_ok=True)
    opts_dict = vars(opts)
    pprint.pprint(opts_dict)
    with open(os.path.join(opts.exp_dir, 'opt.json'), 'w') as f:
        json.dump(opts_dict, f, indent=4, sort_keys=True, default=str)
    Coach(opts).train()


if __name__ == '__main__':
    main(TrainOptions().parse())
