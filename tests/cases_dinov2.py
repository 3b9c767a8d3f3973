"""DINOv2 ViT parity cases: encoder geometries with seeded weights and images, and the tiny encoder inside a model.

Shared by tools/make_golden_dinov2.py (transformers' Dinov2Model -> tests/golden/dinov2_*), tests/test_dinov2_cpu.py and
tests/test_dinov2_model_gpu.py, so all three see the same weights and inputs.  Importing the module registers the reduced geometries.
"""
from __future__ import annotations

from labelanything_amd.config import EncoderSpec, LamConfig, register_encoder
from tests.cases_encoder import encoder_config, encoder_images     # noqa: F401  (the family's importers take them from here)

_D2 = dict(patch=14, layer_scale=True, ln_eps=1e-6)
# position table 5 x 5 (img_size 70): used as stored at 70 px, resampled bicubically at every other side
register_encoder("dinov2_tiny", EncoderSpec("dinov2", dim=128, depth=2, heads=2, mlp=512, img_size=70, **_D2))
# 32-wide heads: zero-padded to 64 columns by the packed weights
register_encoder("dinov2_hd32", EncoderSpec("dinov2", dim=128, depth=2, heads=4, mlp=512, img_size=70, **_D2))
# ViT-B width, two layers: the narrowest geometry that takes the folded-LayerNorm block driver (dim >= 512, t >= 128 tokens); table 16 x 16
register_encoder("dinov2_fold", EncoderSpec("dinov2", dim=768, depth=2, heads=12, mlp=3072, img_size=224, **_D2))

# name -> encoder, input side, images, the seeds, and the block driver the engine must take ("plain": LayerNorm kernels, "fold": LayerNorm
# folded into the neighbour GEMMs).  t = (side / 14)^2 + 1 tokens per image: 26, 10, 26, 145.  Three images at 70 px give 75 patch rows and
# four at 42 px 36: the patch embedding's plane-pair operand (la_gemm a_kmod) needs more than 32.
ENCODER_CASES = {
    "tiny": dict(encoder="dinov2_tiny", side=70, images=3, weight_seed=41, image_seed=141, path="plain"),
    "resample": dict(encoder="dinov2_tiny", side=42, images=4, weight_seed=41, image_seed=142, path="plain"),
    "hd32": dict(encoder="dinov2_hd32", side=70, images=3, weight_seed=43, image_seed=143, path="plain"),
    "fold": dict(encoder="dinov2_fold", side=168, images=2, weight_seed=44, image_seed=144, path="fold"),
}


# The tiny encoder inside the full model at 112 px (8 x 8 grid, 65 tokens, position table resampled 5 -> 8): LAM neck 128 -> 64, mask
# prompts, 1-way 1-shot, two episodes.
MODEL_CASES = {
    "model_tiny_1w1s": dict(
        cfg=LamConfig(encoder="dinov2_tiny", image_size=112, vit_patch_size=14, image_embed_dim=128, embed_dim=64, spatial_convs=3,
                      example_class_attention=False, custom_preprocess=False),
        weight_seed=59,         # (45 - 58: refused by the generator, 8 - 41 % of the reference's pixels inside the margin band)
        episode=dict(batch=2, n_ways=1, k_shots=1, image_size=112, seed=145, prompts=("mask",)),
    ),
}
MARGIN = 2e-3               # argmax must agree wherever the reference's top-2 margin exceeds this share of its largest logit
MAX_BAND_SHARE = 0.05       # the generator refuses a seed with more of the reference's pixels inside the band
