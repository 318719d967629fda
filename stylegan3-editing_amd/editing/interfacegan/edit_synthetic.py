"""InterFaceGAN edits of random synthetic images, with optional interpolation animations (reference
editing/interfacegan/edit_synthetic.py:21-151).

The reference renders an animation with one batch-1 synthesis call per frame: (F - 1) x 25 calls for F editing factors, 200
for `pose`.  `prepare_animation` here builds the same frame latents (same order, including the duplicated frame where two
segments meet) and renders them as one batched sweep, finished on the device by `to_uint8`.  `main` takes an `EditConfig`
(no pyrallis CLI); as this package has no configs/paths_config.py, the config carries the generator path and, optionally, the
InterFaceGAN directions (see FaceEditor)."""
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np
import torch

from editing.interfacegan.face_editor import FaceEditor, render_items
from models.stylegan3.model import GeneratorType
from utils.common import generate_mp4, make_transform, tensor2im

INTERFACEGAN_RANGES = {
    "pose": (-4, 5),
    "age": (-5, 5),
    "smile": (-2, 2),
    "Male": (-2, 4)
}
N_TRANSITIONS = 25


@dataclass
class EditConfig:
    # path to the SG3 generator (.pkl or state dict)
    generator_path: Optional[Path] = None
    # aligned or unaligned generator: selects the direction set when `directions` is not given
    generator_type: GeneratorType = GeneratorType.ALIGNED
    # where the edits and animations go
    output_path: Path = Path("./edit_results")
    # attributes to edit, each one of INTERFACEGAN_RANGES
    attributes_to_edit: List[str] = field(default_factory=lambda: ["age", "smile", "pose", "Male"])
    # images generated and edited per direction
    n_images_per_edit: int = 100
    # truncation psi for sampling
    truncation_psi: float = 0.7
    # whether to apply random user transformations when editing
    apply_random_transforms: bool = False
    # whether to render an interpolation animation of each edit
    generate_animation: bool = False
    # frames per second of the animation
    fps: int = 25
    # {name: .npy path or array} of the InterFaceGAN directions (None: configs.paths_config)
    directions: Optional[Dict[str, object]] = None


def main(opts: EditConfig):
    from models.stylegan3.model import SG3Generator
    kwargs = {'fps': opts.fps}
    save_path = Path(opts.output_path) / str(opts.generator_type)
    save_path.mkdir(exist_ok=True, parents=True)
    generator = SG3Generator(checkpoint_path=opts.generator_path).decoder
    if torch.cuda.is_available():
        generator = generator.cuda()
    for direction in opts.attributes_to_edit:
        if direction not in INTERFACEGAN_RANGES:
            raise ValueError(f"Given invalid direction {direction}. Must be one of {list(INTERFACEGAN_RANGES.keys())}!")
        print(f"Performing edits on attribute: {direction}")
        direction_output_path = save_path / direction
        direction_output_path.mkdir(exist_ok=True, parents=True)
        for idx in range(opts.n_images_per_edit):
            image, latent = get_random_image(generator, truncation_psi=opts.truncation_psi)
            edit_images, edit_latents = edit(generator=generator, latent=latent, direction=direction, generator_type=opts.generator_type,
                                             apply_user_transformations=opts.apply_random_transforms, directions=opts.directions)
            save_coupled_images(edit_images, output_path=direction_output_path / f"{idx}.jpg")
            if opts.generate_animation:
                edit_latents = torch.stack(edit_latents)
                all_images = prepare_animation(latents=edit_latents, generator=generator)
                # duplicate and reverse images for animation
                all_images = all_images + all_images[::-1]
                generate_mp4(direction_output_path / f"{idx}_animation", all_images, kwargs)


def get_random_image(generator, truncation_psi):
    """(PIL image, w [1,num_ws,w_dim]) of z ~ np.random.randn(1, z_dim) with the identity user transform (reference :84-95)."""
    device = next(generator.parameters()).device
    with torch.no_grad():
        z = torch.from_numpy(np.random.randn(1, 512).astype('float32')).to(device)
        if hasattr(generator.synthesis, 'input'):
            m = make_transform(translate=(0, 0), angle=0)
            m = np.linalg.inv(m)
            generator.synthesis.input.transform.copy_(torch.from_numpy(m))
        w = generator.mapping(z, None, truncation_psi=truncation_psi)
        img = generator.synthesis(w, noise_mode='const')
        res_image = tensor2im(img[0])
        return res_image, w


def edit(generator, latent, direction, generator_type, apply_user_transformations=False, directions=None):
    editor = FaceEditor(generator, generator_type, directions=directions)
    return editor.edit(latents=latent, direction=direction, factor_range=INTERFACEGAN_RANGES[direction],
                       apply_user_transformations=apply_user_transformations)


def animation_latents(latents, n_transitions=N_TRANSITIONS):
    """The frame latents of the reference's loop: for each pair (i-1, i) and alpha in linspace(0, 1, n_transitions),
    latents[i][0] * alpha + latents[i-1][0] * (1 - alpha).  [(F-1) * n_transitions, num_ws, w_dim]."""
    alpha_vals = np.linspace(0, 1, n_transitions).tolist()
    frames = [latents[i][0] * alpha + latents[i - 1][0] * (1 - alpha) for i in range(1, len(latents)) for alpha in alpha_vals]
    if not frames:
        return latents[:0, 0]
    return torch.stack(frames)


def prepare_animation(latents, generator, n_transitions=N_TRANSITIONS, max_batch=16, **synthesis_kwargs):
    """latents: [F, 1, num_ws, w_dim] (the stacked edit latents).  Returns the (F-1) * n_transitions frames as uint8 [R,R,3]
    arrays, in the reference's order."""
    from torch_utils.ops.image_finish import to_uint8
    ws = animation_latents(latents, n_transitions)
    if ws.shape[0] == 0:
        return []
    images = render_items(generator, ws, max_batch=max_batch, **synthesis_kwargs)
    frames = to_uint8(images).cpu().numpy()
    return [frames[i] for i in range(frames.shape[0])]


def get_result_from_vecs(generator, vectors_a, vectors_b, alpha):
    """One batch-1 synthesis per vector pair (reference :123-131), kept for callers of the reference API."""
    device = next(generator.parameters()).device
    results = []
    for i in range(len(vectors_a)):
        with torch.no_grad():
            cur_vec = vectors_b[i] * alpha + vectors_a[i] * (1 - alpha)
            res = generator.synthesis(cur_vec.unsqueeze(0).to(device), noise_mode='const')
            results.append(res[0])
    return results


def save_coupled_images(images, output_path):
    from PIL import Image
    if type(images[0]) == list:
        images = [image[0] for image in images]
    res = np.array(images[0])
    for image in images[1:]:
        res = np.concatenate([res, image], axis=1)
    res = Image.fromarray(res).convert("RGB")
    res.save(output_path)
