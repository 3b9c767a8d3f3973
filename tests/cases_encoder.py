"""What the encoder-family case modules (tests/cases_dinov2.py, tests/cases_dinov3.py) share: the encoder-only model and the seeded images
of an encoder case."""
from __future__ import annotations

import torch

from labelanything_amd.config import ENCODER_SPECS, LamConfig


def encoder_config(case: dict) -> LamConfig:
    """The encoder-only model of an encoder case (what ``ImageEncoder`` builds)."""
    spec = ENCODER_SPECS[case["encoder"]]
    return LamConfig(encoder=case["encoder"], image_size=case["side"], vit_patch_size=spec.patch, image_embed_dim=spec.dim)


def encoder_images(case: dict) -> torch.Tensor:
    """Seeded normal images [images, 3, side, side] (the value range of normalised pixels)."""
    g = torch.Generator().manual_seed(case["image_seed"])
    return torch.randn(case["images"], 3, case["side"], case["side"], generator=g)
