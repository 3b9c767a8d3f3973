#!/usr/bin/env python
"""Golden vectors of the DINOv3 ViT encoder from transformers' ``DINOv3ViTModel`` (build container only; tools/golden_lib.py makes the
reference importable for the model case):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dinov3.py [--only NAME] [--no-write]

Encoder cases (tests/cases_dinov3.py ENCODER_CASES): the seeded weights (``init_state_dict``; LayerScale drawn from [0.05, 1.5]) are
strict-loaded into a ``DINOv3ViTModel`` of the case's geometry - in the ``model.layer.N.`` spelling this transformers prints - and the
seeded images run through it on CPU / fp32.  tests/golden/dinov3_<case>.safetensors holds ``patch_tokens`` = last_hidden_state without
the five prefix rows, [images, hw, E]; the json the seeds, the geometry and the model's state-dict keys and shapes in its order.

Model case (MODEL_CASES): the same encoder behind the adapter of tools/golden_lib.py (``PatchGrid``) that drops the prefix tokens and reshapes to [B, E, g, g] - what
the reference's ``ViTModelWrapper`` does for a plain ViT - inside the reference's ``_build_lam``; the seeded episode runs through
``Lam.forward``.  The fixture holds low_res_logits, logits and argmax; the json the share of pixels whose top-two logit gap lies inside the
2e-3 margin band on the reference's own logits, which must be at most 5 % (otherwise pick another weight seed).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

from transformers import DINOv3ViTConfig, DINOv3ViTModel    # noqa: E402
import tests.cases_dinov3 as C      # noqa: E402


def hf_model(spec, side):
    """transformers' model of an EncoderSpec, eval mode."""
    cfg = DINOv3ViTConfig(hidden_size=spec.dim, num_hidden_layers=spec.depth, num_attention_heads=spec.heads, intermediate_size=spec.mlp,
                          patch_size=spec.patch, image_size=side, num_register_tokens=spec.prefix_tokens - 1, rope_theta=spec.rope_theta,
                          layer_norm_eps=spec.ln_eps, key_bias=spec.key_bias, use_gated_mlp=False, hidden_act="gelu")
    return DINOv3ViTModel(cfg).eval()


def spell(key, local):
    """``layer.N.`` of the published checkpoints, or the ``model.layer.N.`` this transformers prints."""
    return key if key in local else "model." + key


if __name__ == "__main__":
    GL.encoder_family_main("dinov3", C, hf_model, spell)
