#!/usr/bin/env python
"""Golden vectors of the DINOv2 ViT encoder from transformers' ``Dinov2Model`` (build container only; tools/golden_lib.py makes the
reference importable for the model case):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dinov2.py [--only NAME] [--no-write]

Encoder cases (tests/cases_dinov2.py ENCODER_CASES): the seeded weights (``init_state_dict``; LayerScale drawn from [0.05, 1.5]) are
strict-loaded into a ``Dinov2Model`` of the case's geometry - its position table is the spec's ``pos_grid``, whatever side the case runs
at - and the seeded images run through it on CPU / fp32.  tests/golden/dinov2_<case>.safetensors holds ``patch_tokens`` =
last_hidden_state without the CLS row, [images, hw, E]; the json the seeds, the geometry and the model's state-dict keys and shapes in
its order.

Model case (MODEL_CASES): the same encoder behind the adapter of tools/golden_lib.py (``PatchGrid``) that drops CLS and reshapes to [B, E, g, g] - what the
reference's ``ViTModelWrapper`` does for a plain ViT - inside the reference's ``_build_lam``; the seeded episode runs through
``Lam.forward``.  The fixture holds low_res_logits, logits and argmax; the json the share of pixels whose top-two logit gap lies inside the
2e-3 margin band on the reference's own logits, which must be at most 5 % (otherwise pick another weight seed).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

from transformers import Dinov2Config, Dinov2Model    # noqa: E402
import tests.cases_dinov2 as C      # noqa: E402


def hf_model(spec, side):
    """transformers' model of an EncoderSpec, eval mode (the position table is the spec's, whatever side the case runs at)."""
    assert spec.mlp % spec.dim == 0
    cfg = Dinov2Config(hidden_size=spec.dim, num_hidden_layers=spec.depth, num_attention_heads=spec.heads, mlp_ratio=spec.mlp // spec.dim,
                       patch_size=spec.patch, image_size=spec.img_size, layer_norm_eps=spec.ln_eps, qkv_bias=True, use_swiglu_ffn=False,
                       hidden_act="gelu")
    return Dinov2Model(cfg).eval()


if __name__ == "__main__":
    GL.encoder_family_main("dinov2", C, hf_model)
