"""CLIP (ViT image tower) on the native transformer kernels: see model.py."""
from .model import CLIP, build_model, convert_weights, load  # noqa: F401
