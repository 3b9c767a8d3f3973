"""DINOv3 ViT parity cases: encoder geometries with seeded weights and images, and the tiny encoder inside a model.

Shared by tools/make_golden_dinov3.py (transformers' DINOv3ViTModel -> tests/golden/dinov3_*), tests/test_dinov3_cpu.py and
tests/test_dinov3_model_gpu.py, so all three see the same weights and inputs.  Importing the module registers the reduced geometries.
"""
from __future__ import annotations

from labelanything_amd.config import EncoderSpec, LamConfig, register_encoder
from tests.cases_encoder import encoder_config, encoder_images     # noqa: F401  (the family's importers take them from here)

_D3 = dict(prefix_tokens=5, rope_theta=100.0, layer_scale=True, key_bias=False, ln_eps=1e-5)
register_encoder("dinov3_tiny", EncoderSpec("dinov3", dim=128, depth=2, heads=2, mlp=512, img_size=64, **_D3))
# 32-wide heads: zero-padded to 64 columns by the packed weights, la_rope_qk rotates the first 32 of every 64
register_encoder("dinov3_hd32", EncoderSpec("dinov3", dim=128, depth=2, heads=4, mlp=512, img_size=64, **_D3))
# ViT-B width, two layers: the narrowest geometry that takes the folded-LayerNorm block driver (dim >= 512, t >= 128 tokens)
register_encoder("dinov3_fold", EncoderSpec("dinov3", dim=768, depth=2, heads=12, mlp=3072, img_size=192, **_D3))

# name -> encoder, input side, images, the seeds, and the block driver the engine must take ("plain": LayerNorm kernels, "fold": LayerNorm
# folded into the neighbour GEMMs).  t = (side / 16)^2 + 5 tokens per image: 21, 21, 149.  Three images at 64 px: the patch embedding's
# plane-pair operand (la_gemm a_kmod) needs more than 32 rows, 3 x 16 patches is the smallest batch that has them.
ENCODER_CASES = {
    "tiny": dict(encoder="dinov3_tiny", side=64, images=3, weight_seed=31, image_seed=131, path="plain"),
    "hd32": dict(encoder="dinov3_hd32", side=64, images=3, weight_seed=32, image_seed=132, path="plain"),
    "fold": dict(encoder="dinov3_fold", side=192, images=2, weight_seed=33, image_seed=133, path="fold"),
}


# The tiny encoder inside the full model at 128 px (8 x 8 grid, 69 tokens): LAM neck 128 -> 64, mask prompts, 1-way 1-shot, two episodes.
MODEL_CASES = {
    "model_tiny_1w1s": dict(
        cfg=LamConfig(encoder="dinov3_tiny", image_size=128, image_embed_dim=128, embed_dim=64, spatial_convs=3,
                      example_class_attention=False, custom_preprocess=False),
        weight_seed=39,         # (34 - 38: refused by the generator, 7 - 18 % of the reference's pixels inside the margin band)
        episode=dict(batch=2, n_ways=1, k_shots=1, image_size=128, seed=134, prompts=("mask",)),
    ),
}
MARGIN = 2e-3               # argmax must agree wherever the reference's top-2 margin exceeds this share of its largest logit
MAX_BAND_SHARE = 0.05       # the generator refuses a seed with more of the reference's pixels inside the band
