"""Parity cases of the two-level classification head (``classification_levels=2``, mask_decoder.py:204,345-362).

Both run the ``novit_d256_2w3s`` episode and geometry of tests/cases.py (decoder only, D = 256, 16 x 16 grid, 2-way 3-shot + background, one
missing mask, masks + points, class encoder on).  The ``level_reducer`` tensors come from ``init_state_dict`` like every other tensor
(fan-in 18: weights of order 0.24).  tools/make_golden_levels.py turns the cases into tests/golden/levels_<name>.{safetensors,json};
tests/test_levels_*.py read them.
"""
from __future__ import annotations

import dataclasses

from tests.cases import CASES

_BASE = CASES["novit_d256_2w3s"]


def _case(**over):
    cfg = dataclasses.replace(_BASE["cfg"], classification_levels=2, **over)
    return dict(cfg=cfg, weight_seed=_BASE["weight_seed"], episode=dict(_BASE["episode"]))


LV_CASES = {
    # the base case with the switch on
    "l2": _case(),
    # the model section of parameters/trainval/pascal/mae_levels.yaml: example_class_attention off
    "l2_noeca": _case(example_class_attention=False),
}

# the decoder-only training step stored for l2 (tools/make_golden_levels.py): ground truth seed of tests.test_train_gpu.make_gt
LV_TRAIN = dict(case="l2", seed_gt=17)

# full gradients kept in the fixture (the others are held by their norms)
LV_TRAIN_FULL = [
    "mask_decoder.level_reducer.weight", "mask_decoder.level_reducer.bias",
    "mask_decoder.class_mlp.layers.2.weight", "mask_decoder.output_upscaling.3.bias", "mask_decoder.spatial_convs.3.weight",
    "mask_decoder.transformer.norm_final_attn.weight", "mask_decoder.transformer.layers.1.norm4.bias",
    "mask_decoder.transformer.final_attn_token_to_image.q_proj.weight", "prompt_encoder.not_a_mask_embed.weight",
    "prompt_encoder.class_encoder.pos_embedding",
]
