"""Parity cases of the per-example family (``segment_example_logits`` / ``embeddings_per_example``, build_lam.py:126,145-148).

All three run the ``novit_d256_2w3s`` episode and geometry of tests/cases.py (decoder only, D = 256, 16 x 16 grid, 2-way 3-shot + background,
one missing mask, masks + points, class encoder on) so that only the configuration family differs.  tools/make_golden_multi_embedding.py
turns them into tests/golden/multi_embedding_<name>.{safetensors,json}; tests/test_multi_embedding_*.py read them.
"""
from __future__ import annotations

import dataclasses

from labelanything_amd.config import resolve_examples
from tests.cases import CASES

_BASE = CASES["novit_d256_2w3s"]


def _case(embeddings_per_example, segment_example_logits, attn: bool):
    seg, epe = resolve_examples(segment_example_logits, embeddings_per_example)
    cfg = dataclasses.replace(_BASE["cfg"], segment_example_logits=seg, embeddings_per_example=epe, class_attention=attn,
                              example_attention=attn, example_class_attention=attn)
    return dict(cfg=cfg, weight_seed=_BASE["weight_seed"], episode=dict(_BASE["episode"]))


ME_CASES = {
    # the model section of parameters/trainval/pascal/mae_multiemb.yaml: 4 embeddings per example, no merge attention.
    # 16 x 16 grid pooled 2 x 2: N = 6 supports x 4 bins = 24 examples of C = 3 classes, 72 decoder tokens (the unfused two-way chain)
    "e4": _case(4, False, attn=False),
    # 3 x 3 bins on the 16 x 16 grid overlap (rows 0-5, 5-10, 10-15); all three merge attentions over M k k = 54 examples, 162 tokens
    "e9_attn": _case(9, False, attn=True),
    # segment_example_logits alone: one embedding per example (the plain mean), maximum over the 6 supports, 18 tokens (the fused two-way kernels)
    "e1": _case(None, True, attn=False),
}

# the decoder-only training step stored for e4 (tools/make_golden_multi_embedding.py): ground truth seed of tests.test_train_gpu.make_gt
ME_TRAIN = dict(case="e4", seed_gt=17)

# full gradients kept in the fixture (the others are held by their norms)
ME_TRAIN_FULL = [
    "mask_decoder.class_mlp.layers.2.weight", "mask_decoder.class_mlp.layers.0.bias", "mask_decoder.output_upscaling.3.bias",
    "mask_decoder.spatial_convs.3.weight", "mask_decoder.transformer.layers.1.norm4.bias",
    "mask_decoder.transformer.final_attn_token_to_image.q_proj.weight", "prompt_encoder.not_a_mask_embed.weight",
    "prompt_encoder.mask_downscaling.0.weight", "prompt_encoder.point_embeddings.1.weight",
    "prompt_encoder.transformer.layers.0.mlp.lin1.bias", "prompt_encoder.transformer.layers.1.cross_attn_image_to_token.k_proj.weight",
    "prompt_encoder.class_encoder.pos_embedding",
]
