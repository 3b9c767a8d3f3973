"""Parity cases of ``conv_classification`` and ``classification_layer_downsample_rate=1`` (mask_decoder.py:198-271,299-309;
parameters/trainval/pascal/mae_nodown.yaml).

All run the ``novit_d256_2w3s`` episode and geometry of tests/cases.py (decoder only, D = 256, 16 x 16 grid, 2-way 3-shot + background, one
missing mask, masks + points, class encoder on): a 64 x 64 x cf feature map.  The ``prototype_tconv`` tensors come from ``init_state_dict``
like every other tensor.  tools/make_golden_convcls.py turns the cases into tests/golden/<name>.{safetensors,json};
tests/test_convcls_*.py read them.
"""
from __future__ import annotations

import dataclasses

from tests.cases import CASES

_BASE = CASES["novit_d256_2w3s"]


def _case(rate, conv):
    cfg = dataclasses.replace(_BASE["cfg"], classification_layer_downsample_rate=rate, conv_classification=conv)
    return dict(cfg=cfg, weight_seed=_BASE["weight_seed"], episode=dict(_BASE["episode"]))


CC_CASES = {
    "convcls_r1": _case(1, True),        # the recipe's two switches
    "convcls_r8": _case(8, True),
    "nodown_r1": _case(1, False),
}

# the decoder-only training step stored for convcls_r1: ground truth seed of tests.test_train_gpu.make_gt
CC_TRAIN = dict(case="convcls_r1", seed_gt=17)

# a second stored step: plain classification on the 256-wide map (the training graph's la_classify_wide branch)
CC_TRAIN_PLAIN = dict(case="nodown_r1", seed_gt=17)

# full gradients kept in the fixture (the others are held by their norms); of the two prototype_tconv tensors (2.4 MB each) the first
# CC_TCONV_ROWS input channels
CC_TCONV = ["mask_decoder.prototype_tconv.0.weight", "mask_decoder.prototype_tconv.1.weight"]
CC_TCONV_ROWS = 8
CC_TRAIN_FULL = [
    "mask_decoder.class_mlp.layers.2.weight", "mask_decoder.output_upscaling.3.bias", "mask_decoder.spatial_convs.3.bias",
    "mask_decoder.transformer.norm_final_attn.weight", "mask_decoder.transformer.layers.1.norm4.bias",
    "prompt_encoder.not_a_mask_embed.weight", "prompt_encoder.class_encoder.pos_embedding",
]
