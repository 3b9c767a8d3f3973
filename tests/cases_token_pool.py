"""Parity cases of the TokenPool prompt encoder (``prompt_encoder="TokenPool"``, PromptImagePoolEncoder, prompt_encoder.py:830-915; the
model section of parameters/trainval/{pascal,coco20i}/mae_pool.yaml).

tools/make_golden_token_pool.py turns them into tests/golden/token_pool_<name>.{safetensors,json} (+ ``_train`` for the stored training
step); tests/test_token_pool_*.py read them.
"""
from __future__ import annotations

import dataclasses

from tests.cases import CASES, TRAIN_CASE

_BASE = CASES["novit_d256_2w3s"]

TP_CASES = {
    # geometry and episode of novit_d256_2w3s: D = 256, 16 x 16 grid, B M = 6 supports of C = 3 classes, masks + points (Ns = 2: 6 tokens
    # a support), one missing mask, class encoder on, class_example_attention on
    "tp_d256": dict(cfg=dataclasses.replace(_BASE["cfg"], prompt_encoder="TokenPool"), weight_seed=_BASE["weight_seed"],
                    episode=dict(_BASE["episode"])),
    # TRAIN_CASE: D = 64 behind the 96 -> 64 neck, 8 x 8 grid, B = 2, M = 4, C = 3, masks + points + boxes
    "tp_d64": dict(cfg=dataclasses.replace(TRAIN_CASE["cfg"], prompt_encoder="TokenPool"), weight_seed=TRAIN_CASE["weight_seed"],
                   episode=dict(TRAIN_CASE["episode"])),
    # the recipe's prompt type: masks only (Ns = 1, the "no sparse prompt" token), no class encoder, no merge attention
    "tp_masks": dict(cfg=dataclasses.replace(_BASE["cfg"], prompt_encoder="TokenPool", class_encoder=None, example_class_attention=False),
                     weight_seed=_BASE["weight_seed"], episode=dict(_BASE["episode"], prompts=("mask",))),
}

# the decoder-only training step stored for tp_d64: ground-truth seed of tests.test_train_gpu.make_gt
TP_TRAIN = dict(case="tp_d64", seed_gt=17)

# full gradients kept in the fixture (the others are held by their norms)
TP_TRAIN_FULL = [
    "prompt_encoder.transformer.final_attn_token_to_image.out_proj.weight", "prompt_encoder.transformer.norm_final_attn.weight",
    "prompt_encoder.mask_downscaling.0.weight", "prompt_encoder.mask_downscaling.6.bias", "prompt_encoder.not_a_mask_embed.weight",
    "prompt_encoder.class_encoder.pos_embedding", "prompt_encoder.point_embeddings.2.weight",
    "prompt_encoder.transformer.layers.1.cross_attn_image_to_token.k_proj.weight", "mask_decoder.class_mlp.layers.2.weight",
    "neck.0.weight",
]

SRC_STRIDE = 4          # class_examples_src is stored at every fourth pixel and channel
