"""Parity cases of the one-way mask decoder (``fusion_transformer="OneWayTransformer"``, models/transformer.py:26-154; the model section of
parameters/trainval/Ablations/mae_transformer.yaml).

tools/make_golden_oneway.py turns them into tests/golden/oneway_<name>.{safetensors,json} (+ ``_train`` for the stored training step);
tests/test_oneway_*.py read them.
"""
from __future__ import annotations

import dataclasses

from tests.cases import CASES, TRAIN_CASE

_BASE = CASES["novit_d256_2w3s"]
_OW = dict(fusion_transformer="OneWayTransformer")

OW_CASES = {
    # geometry and episode of novit_d256_2w3s: D = 256, 16 x 16 grid, C = 3 classes, class encoder on: the fused path (la_twoway_i2t +
    # la_stream_mlp per layer)
    "ow_d256": dict(cfg=dataclasses.replace(_BASE["cfg"], **_OW), weight_seed=_BASE["weight_seed"], episode=dict(_BASE["episode"])),
    # TRAIN_CASE: D = 64 behind the 96 -> 64 neck, 8 x 8 grid, B = 2: the unfused chain; also the stored training step.  The weight seed
    # is not TRAIN_CASE's: see KINK_BAND
    "ow_d64": dict(cfg=dataclasses.replace(TRAIN_CASE["cfg"], **_OW), weight_seed=109, episode=dict(TRAIN_CASE["episode"])),
    # the recipe's model section: no class encoder, example_class_attention off, masks only
    "ow_masks": dict(cfg=dataclasses.replace(_BASE["cfg"], class_encoder=None, example_class_attention=False, **_OW),
                     weight_seed=_BASE["weight_seed"], episode=dict(_BASE["episode"], prompts=("mask",))),
}

# the decoder-only training step stored for ow_d64: ground-truth seed of tests.test_train_gpu.make_gt (as TP_TRAIN)
OW_TRAIN = dict(case="ow_d64", seed_gt=17)

# full gradients kept in the fixture (the others are held by their norms)
OW_TRAIN_FULL = [
    "mask_decoder.transformer.layers.1.mlp.lin1.weight", "mask_decoder.transformer.layers.0.cross_attn_image_to_token.k_proj.weight",
    "mask_decoder.transformer.layers.0.mlp.lin2.bias", "mask_decoder.transformer.layers.1.norm2.weight",
    "mask_decoder.transformer.layers.0.cross_attn_image_to_token.q_proj.weight", "mask_decoder.class_mlp.layers.0.weight",
    "prompt_encoder.class_encoder.pos_embedding", "neck.0.weight",
]

SRC_STRIDE = 4          # the transformer's image output is stored at every fourth pixel row, pixel column and channel
MARGIN = 2e-3           # the project's argmax margin band: pixels whose top-two logit gap lies inside it are not compared
MAX_BAND_SHARE = 0.05   # ... and may be at most this share of the reference's own pixels

# The stream MLP puts 2 x 128 x 2048 ReLU pre-activations into the training step, and a gradient is only defined to the tests' bound where
# none of them changes sign under an fp32 evaluation: ONE flipped unit on one pixel row moves a whole row of lin1's weight gradient by
# that pixel's share (2e-2 of the tensor's scale here) and everything upstream of it by 1e-3, while every gradient norm stays within 1e-4.
# With TRAIN_CASE's weight seed (21) the reference's fp64 forward has a pre-activation of 3.4e-7 (8e-8 of the largest) in layer 1, below
# one fp32 ulp of the products that are summed into it.  The generator therefore records the smallest |pre-activation| of both layers in the
# reference's fp64 forward, relative to the largest, and refuses a case where it lies inside this band - sqrt(K) u sum|x_i w_i| of the
# K = 64 term fp32 dot product, about 1e-6 of the largest pre-activation; the remedy is the one of the argmax band, another weight seed.
KINK_BAND = 1e-6
