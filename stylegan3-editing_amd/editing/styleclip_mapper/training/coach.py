"""Training of a StyleCLIP latent mapper for one text prompt (reference editing/styleclip_mapper/training/coach.py).

The control flow is the reference's: `train` (w_hat = w + 0.1 * mapper(w), CLIP + latent-L2 (+ ID) loss, optimizer step, image /
metric logging, validation, checkpoints), `validate`, `checkpoint_me`, `configure_optimizers`, `configure_datasets`, `calc_loss`.
Checkpoints are {'state_dict': net.state_dict(), 'opts': vars(opts)}, which `StyleCLIPMapper.load_weights` and the reference's
loader both read.  In training mode the mapper runs its HIP forward and backward (editing/styleclip_mapper/latent_mappers.py) and
Ranger steps in one launch (utils/ranger.py).

What differs from the reference:
  decoder   It is put in eval mode with requires_grad_(False) and only `mapper.train()` is called: the optimizer holds the mapper's
            parameters alone, so weight gradients of the generator would be computed and thrown away.  The decoder still carries
            the image gradient back to w_hat.
  text      The prompt arrives as token ids [n_text, context_length]: the `text_tokens` argument, or the file `opts.text_tokens`
            (.npy or .pt).  There is no tokenizer in this package; `opts.description` is only recorded.
  logging   Scalars go to `logs/metrics.jsonl`, one JSON object per logged step and prefix, and to a tensorboard SummaryWriter
            only if that is importable.  Image grids (inputs above, edits below) are finished by
            torch_utils.ops.image_finish.to_uint8 and written with PIL; torchvision is not needed.
  ID loss   With `opts.id_lambda > 0` (the reference's default is 0.06) the loss is `criteria.id_loss.IDLoss(opts)` when
            `opts.ir_se50_weights` names an existing file, or a module given as `Coach(opts, id_loss=module)` with the reference's
            call, `loss, sim_improvement, logs = id_loss(x_hat, x, x)`.  With neither, a NotImplementedError says so (the weights
            are no part of this package: pass --ir_se50_weights, a module, or --id_lambda 0).
  scalars   `float(loss)` waits for the device, so `calc_loss` returns tensors and they are read only on steps that log,
            validate or write a checkpoint.
  device    `opts.device` when set, else cuda:0 when there is one.  `net` and `clip_loss` may be passed ready-made.
"""
import json
import os

import numpy as np
import torch
from torch import nn
from torch.utils.data import DataLoader

from editing.styleclip_mapper.datasets.latents_dataset import LatentsDataset
from utils import train_utils
from utils.ranger import Ranger


def _load_tokens(path):
    tokens = torch.load(path, map_location='cpu') if str(path).endswith(('.pt', '.pth')) else torch.from_numpy(np.load(path))
    return tokens.long()


class Coach:
    def __init__(self, opts, id_loss=None, net=None, clip_loss=None, text_tokens=None):
        self.opts = opts
        self.global_step = 0
        self.device = getattr(opts, 'device', None) or ('cuda:0' if torch.cuda.is_available() else 'cpu')
        self.opts.device = self.device

        if self.opts.id_lambda > 0 and id_loss is None:
            weights = getattr(opts, 'ir_se50_weights', None)
            if not (weights and os.path.isfile(weights)):
                raise NotImplementedError('the IR-SE50 ID loss is not part of this package: pass an id_loss module to Coach, or train '
                                          'with --id_lambda 0')
            from criteria.id_loss import IDLoss
            id_loss = IDLoss(opts)
        if net is None:
            from editing.styleclip_mapper.styleclip_mapper import StyleCLIPMapper
            net = StyleCLIPMapper(self.opts)
        self.net = net.to(self.device)
        self.net.decoder.eval().requires_grad_(False)

        if self.opts.id_lambda > 0:
            self.id_loss = id_loss.to(self.device).eval()
        if self.opts.clip_lambda > 0:
            if clip_loss is None:
                from criteria.clip_loss import CLIPLoss
                clip_loss = CLIPLoss(opts)
            self.clip_loss = clip_loss
            if text_tokens is None:
                if not getattr(opts, 'text_tokens', None):
                    raise ValueError('Coach: the prompt is given as token ids, by the text_tokens argument or --text_tokens')
                text_tokens = _load_tokens(opts.text_tokens)
            self.text_inputs = torch.as_tensor(text_tokens).to(self.device)
        if self.opts.latent_l2_lambda > 0:
            self.latent_l2_loss = nn.MSELoss().to(self.device).eval()

        self.optimizer = self.configure_optimizers()

        self.train_dataset, self.test_dataset = self.configure_datasets()
        self.train_dataloader = DataLoader(self.train_dataset, batch_size=self.opts.batch_size, shuffle=True,
                                           num_workers=int(self.opts.workers), drop_last=True)
        self.test_dataloader = DataLoader(self.test_dataset, batch_size=self.opts.test_batch_size, shuffle=False,
                                          num_workers=int(self.opts.test_workers), drop_last=True)

        self.log_dir = os.path.join(opts.exp_dir, 'logs')
        os.makedirs(self.log_dir, exist_ok=True)
        self.metrics_path = os.path.join(self.log_dir, 'metrics.jsonl')
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.logger = SummaryWriter(log_dir=self.log_dir)
        except ImportError:
            self.logger = None

        self.checkpoint_dir = os.path.join(opts.exp_dir, 'checkpoints')
        os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.best_val_loss = None
        if self.opts.save_interval is None:
            self.opts.save_interval = self.opts.max_steps

    def train(self):
        self.net.mapper.train()
        while self.global_step < self.opts.max_steps:
            for batch in self.train_dataloader:
                self.optimizer.zero_grad()
                w = batch.to(self.device)
                with torch.no_grad():
                    x = self.net.decoder.synthesis(w)
                w_hat = self.edit(w)
                x_hat = self.net.decoder.synthesis(w_hat)
                loss, loss_dict = self.calc_loss(w, x, w_hat, x_hat)
                loss.backward()
                self.optimizer.step()

                if self.global_step % self.opts.image_interval == 0 or (self.global_step < 1000 and self.global_step % 1000 == 0):
                    self.parse_and_log_images(x, x_hat, title='images_train')
                if self.global_step % self.opts.board_interval == 0:
                    scalars = _scalars(loss_dict)
                    self.print_metrics(scalars, prefix='train')
                    self.log_metrics(scalars, prefix='train')

                val_loss_dict = None
                if self.global_step % self.opts.val_interval == 0 or self.global_step == self.opts.max_steps:
                    val_loss_dict = self.validate()
                    if val_loss_dict and (self.best_val_loss is None or val_loss_dict['loss'] < self.best_val_loss):
                        self.best_val_loss = val_loss_dict['loss']
                        self.checkpoint_me(val_loss_dict, is_best=True)

                if self.global_step % self.opts.save_interval == 0 or self.global_step == self.opts.max_steps:
                    self.checkpoint_me(val_loss_dict if val_loss_dict is not None else _scalars(loss_dict), is_best=False)

                if self.global_step == self.opts.max_steps:
                    print('OMG, finished training!')
                    break

                self.global_step += 1

    def edit(self, w):
        """w + 0.1 * mapper(w), from the mapper's own `edit` where it has one (one HIP forward, one HIP backward)."""
        edit = getattr(self.net.mapper, 'edit', None)
        return edit(w, 0.1) if edit is not None else w + 0.1 * self.net.mapper(w)

    def validate(self):
        self.net.mapper.eval()
        agg_loss_dict = []
        for batch_idx, batch in enumerate(self.test_dataloader):
            if batch_idx > 200:
                break
            w = batch.to(self.device)
            with torch.no_grad():
                x = self.net.decoder.synthesis(w)
                w_hat = self.edit(w)
                x_hat = self.net.decoder.synthesis(w_hat)
                _, cur_loss_dict = self.calc_loss(w, x, w_hat, x_hat)
            agg_loss_dict.append(cur_loss_dict)
            self.parse_and_log_images(x, x_hat, title='images_val', index=batch_idx)
            # for the first step just do a sanity test on a small amount of data
            if self.global_step == 0 and batch_idx >= 4:
                self.net.mapper.train()
                return None
        loss_dict = train_utils.aggregate_loss_dict([_scalars(d) for d in agg_loss_dict])
        self.log_metrics(loss_dict, prefix='test')
        self.print_metrics(loss_dict, prefix='test')
        self.net.mapper.train()
        return loss_dict

    def checkpoint_me(self, loss_dict, is_best):
        save_name = 'best_model.pt' if is_best else f'iteration_{self.global_step}.pt'
        torch.save(self._get_save_dict(), os.path.join(self.checkpoint_dir, save_name))
        with open(os.path.join(self.checkpoint_dir, 'timestamp.txt'), 'a') as f:
            if is_best:
                f.write(f'**Best**: Step - {self.global_step}, Loss - {self.best_val_loss:.3f} \n{loss_dict}\n')
            else:
                f.write(f'Step - {self.global_step}, \n{loss_dict}\n')

    def configure_optimizers(self):
        params = list(self.net.mapper.parameters())
        if self.opts.optim_name == 'adam':
            return torch.optim.Adam(params, lr=self.opts.learning_rate)
        return Ranger(params, lr=self.opts.learning_rate)

    def _generate_latents(self, count, batch_size):
        z = torch.randn(self.opts.train_dataset_size, 512, device=self.device)
        mapping = self.net.decoder.mapping
        latents = []
        for b in range(count // batch_size):
            with torch.no_grad():
                w = mapping(z[b: b + batch_size], None)
                latents.append(mapping.w_avg.lerp(w, self.opts.truncation_psi))
        return torch.cat(latents)

    def configure_datasets(self):
        if self.opts.latents_train_path and os.path.exists(self.opts.latents_train_path):
            print('Loading train dataset...')
            train_latents = torch.load(self.opts.latents_train_path, map_location='cpu')
        else:
            print('Generating train dataset...')
            train_latents = self._generate_latents(self.opts.train_dataset_size, self.opts.batch_size)
            torch.save(train_latents, self.opts.latents_train_path)
        if self.opts.latents_test_path and os.path.exists(self.opts.latents_test_path):
            print('Loading test dataset...')
            test_latents = torch.load(self.opts.latents_test_path, map_location='cpu')
        else:
            print('Generating test dataset...')
            test_latents = self._generate_latents(self.opts.test_dataset_size, self.opts.test_batch_size)
            torch.save(test_latents, self.opts.latents_test_path)
        train_dataset = LatentsDataset(latents=train_latents.cpu(), opts=self.opts)
        test_dataset = LatentsDataset(latents=test_latents.cpu(), opts=self.opts)
        print(f'Number of training samples: {len(train_dataset)}')
        print(f'Number of test samples: {len(test_dataset)}')
        return train_dataset, test_dataset

    def calc_loss(self, w, x, w_hat, x_hat):
        """(loss, {name: 0-dim tensor}); the entries are read with `float` only where they are logged."""
        loss_dict = {}
        loss = 0.0
        if self.opts.id_lambda > 0:
            loss_id, sim_improvement, _ = self.id_loss(x_hat, x, x)
            loss_dict['loss_id'] = torch.as_tensor(loss_id).detach()
            loss_dict['id_improve'] = torch.as_tensor(sim_improvement).detach()
            loss = loss_id * self.opts.id_lambda
        if self.opts.clip_lambda > 0:
            loss_clip = self.clip_loss(x_hat, self.text_inputs).mean()
            loss_dict['loss_clip'] = loss_clip.detach()
            loss = loss + loss_clip * self.opts.clip_lambda
        if self.opts.latent_l2_lambda > 0:
            loss_l2_latent = self.latent_l2_loss(w_hat, w)
            loss_dict['loss_l2_latent'] = loss_l2_latent.detach()
            loss = loss + loss_l2_latent * self.opts.latent_l2_lambda
        loss_dict['loss'] = torch.as_tensor(loss).detach()
        return loss, loss_dict

    def log_metrics(self, metrics_dict, prefix):
        with open(self.metrics_path, 'a') as f:
            f.write(json.dumps({'step': self.global_step, 'prefix': prefix, **{k: float(v) for k, v in metrics_dict.items()}}) + '\n')
        for key, value in metrics_dict.items():
            print(f'step: {self.global_step} \t metric: {prefix}/{key} \t value: {value}')
            if self.logger is not None:
                self.logger.add_scalar(f'{prefix}/{key}', value, self.global_step)

    def print_metrics(self, metrics_dict, prefix):
        print(f'Metrics for {prefix}, step {self.global_step}')
        for key, value in metrics_dict.items():
            print(f'\t{key} = ', value)

    def parse_and_log_images(self, x, x_hat, title, index=None):
        from PIL import Image
        from torch_utils.ops.image_finish import to_uint8
        name = f'{str(self.global_step).zfill(5)}.jpg' if index is None else f'{str(self.global_step).zfill(5)}_{str(index).zfill(5)}.jpg'
        path = os.path.join(self.log_dir, title, name)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        tiles = to_uint8(torch.cat([x.detach(), x_hat.detach()]).float()).cpu().numpy()        # [2B, H, W, 3]
        rows = [np.concatenate(list(tiles[r:r + x.shape[0]]), axis=1) for r in range(0, tiles.shape[0], x.shape[0])]
        Image.fromarray(np.concatenate(rows, axis=0)).save(path)

    def _get_save_dict(self):
        return {'state_dict': self.net.state_dict(), 'opts': vars(self.opts)}


def _scalars(loss_dict):
    return {k: float(v) for k, v in loss_dict.items()}
