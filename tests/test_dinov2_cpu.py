"""CPU: the DINOv2 ViT encoder's configuration, weights layout and refusals (no device code runs)."""
import json
import os

import pytest
import torch
from safetensors.torch import save_file

from labelanything_amd.config import ENCODER_SPECS, EncoderSpec, dinov2_spec_from_hf_config
from labelanything_amd.models import ImageEncoder, Lam
from labelanything_amd.weights import encoder_shapes, init_state_dict
from tests.cases_dinov2 import ENCODER_CASES, MODEL_CASES, encoder_config

# config.json of facebook/dinov2-base, the fields the encoder depends on
HF_CONFIG = {"model_type": "dinov2", "hidden_size": 768, "num_hidden_layers": 12, "num_attention_heads": 12, "mlp_ratio": 4,
             "patch_size": 14, "image_size": 518, "layer_norm_eps": 1e-6, "layerscale_value": 1.0, "qkv_bias": True,
             "use_swiglu_ffn": False, "hidden_act": "gelu"}


def test_registered_specs_and_the_defaults_of_every_other_kind():
    want = {"vit_s_dinov2": (384, 12, 6, 1536), "vit_b_dinov2": (768, 12, 12, 3072), "vit_l_dinov2": (1024, 24, 16, 4096)}
    for name, (dim, depth, heads, mlp) in want.items():
        s = ENCODER_SPECS[name]
        assert (s.kind, s.dim, s.depth, s.heads, s.mlp, s.patch, s.img_size, s.pos_grid, s.head_dim) == \
            ("dinov2", dim, depth, heads, mlp, 14, 518, 37, 64)
        assert (s.prefix_tokens, s.layer_scale, s.key_bias, s.ln_eps) == (1, True, True, 1e-6)
    # existing specs mean what they meant
    assert ENCODER_SPECS["vit_b_mae"] == EncoderSpec("hf", 768, 12, 12, 3072, img_size=224)
    assert ENCODER_SPECS["vit_b_dinov3"].ln_eps == 1e-5 and ENCODER_SPECS["vit_b_dinov3"].patch == 16
    assert dinov2_spec_from_hf_config(HF_CONFIG) == ENCODER_SPECS["vit_b_dinov2"]
    # Dinov2Config has no intermediate_size: the MLP width is hidden_size * mlp_ratio
    assert dinov2_spec_from_hf_config({**HF_CONFIG, "hidden_size": 384, "num_attention_heads": 6}) == ENCODER_SPECS["vit_s_dinov2"]


def test_state_dict_layout_is_the_transformers_one():
    """Keys and shapes under image_encoder. in Dinov2Model's order and spelling; mask_token is held."""
    spec = ENCODER_SPECS["dinov2_tiny"]
    shapes = encoder_shapes(spec)
    pre = "image_encoder."
    keys = [k[len(pre):] for k in shapes]
    assert keys[:5] == ["embeddings.cls_token", "embeddings.mask_token", "embeddings.position_embeddings",
                        "embeddings.patch_embeddings.projection.weight", "embeddings.patch_embeddings.projection.bias"]
    layer0 = [k[len("encoder.layer.0."):] for k in keys if k.startswith("encoder.layer.0.")]
    assert layer0 == ["norm1.weight", "norm1.bias", "attention.attention.query.weight", "attention.attention.query.bias",
                      "attention.attention.key.weight", "attention.attention.key.bias", "attention.attention.value.weight",
                      "attention.attention.value.bias", "attention.output.dense.weight", "attention.output.dense.bias",
                      "layer_scale1.lambda1", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight",
                      "mlp.fc2.bias", "layer_scale2.lambda1"]
    assert keys[-2:] == ["layernorm.weight", "layernorm.bias"] and len(keys) == 5 + 18 * spec.depth + 2
    assert shapes[pre + "embeddings.position_embeddings"] == (1, 26, 128) and shapes[pre + "embeddings.mask_token"] == (1, 128)
    assert shapes[pre + "embeddings.patch_embeddings.projection.weight"] == (128, 3, 14, 14)
    for name in ENCODER_CASES:
        # what transformers itself listed when the fixture was made
        meta = json.load(open(os.path.join(os.path.dirname(__file__), "golden", f"dinov2_{name}.json")))
        s = encoder_shapes(ENCODER_SPECS[ENCODER_CASES[name]["encoder"]])
        assert meta["state_dict"] == [[k[len(pre):], list(v)] for k, v in s.items()]
    sd = init_state_dict(encoder_config(ENCODER_CASES["tiny"]), 0)
    lam1 = torch.cat([v for k, v in sd.items() if k.endswith("lambda1")])
    assert 0.05 <= float(lam1.min()) < 0.2 and 1.35 < float(lam1.max()) <= 1.5          # LayerScale is drawn, never the initial 1.0


def test_strict_load_reports_missing_and_unexpected_keys():
    case = ENCODER_CASES["tiny"]
    src = ImageEncoder(case["encoder"], image_size=case["side"], seed=5).state_dict()
    enc = ImageEncoder(case["encoder"], image_size=case["side"], seed=6)
    enc.load_state_dict(src)                                     # (the key mapping of other HF spellings leaves these keys alone)
    assert all(torch.equal(v, src[k]) for k, v in enc.state_dict().items()) and "embeddings.mask_token" in src
    assert "encoder.layer.1.mlp.fc2.weight" in src and "encoder.layer.0.layer_scale1.lambda1" in src
    with pytest.raises(RuntimeError, match="missing"):
        enc.load_state_dict({k: v for k, v in src.items() if "layer_scale2" not in k})
    with pytest.raises(RuntimeError, match="unexpected"):
        enc.load_state_dict({**src, "encoder.layer.0.layernorm_before.weight": torch.zeros(128)})
    # the whole model, strictly, through Lam.load_state_dict
    mcase = MODEL_CASES["model_tiny_1w1s"]
    full = init_state_dict(mcase["cfg"], 7)
    lam = Lam(mcase["cfg"], seed=8)
    lam.load_state_dict(full)
    assert all(torch.equal(v, full[k]) for k, v in lam.state_dict().items())


def test_unbuilt_variants_are_refused_by_name():
    with pytest.raises(NotImplementedError, match="use_swiglu_ffn"):
        dinov2_spec_from_hf_config({**HF_CONFIG, "use_swiglu_ffn": True})
    with pytest.raises(NotImplementedError, match="hidden_act"):
        dinov2_spec_from_hf_config({**HF_CONFIG, "hidden_act": "silu"})
    with pytest.raises(NotImplementedError, match="qkv_bias"):
        dinov2_spec_from_hf_config({**HF_CONFIG, "qkv_bias": False})
    with pytest.raises(NotImplementedError, match="register variant"):
        dinov2_spec_from_hf_config({**HF_CONFIG, "model_type": "dinov2_with_registers", "num_register_tokens": 4})
    with pytest.raises(NotImplementedError, match="128"):
        dinov2_spec_from_hf_config({**HF_CONFIG, "hidden_size": 1536, "num_attention_heads": 8})
    with pytest.raises(ValueError, match="model_type"):
        dinov2_spec_from_hf_config({**HF_CONFIG, "model_type": "vit"})


@pytest.mark.parametrize("change,match", [({"use_swiglu_ffn": True, "hidden_size": 1536, "num_attention_heads": 24}, "use_swiglu_ffn"),
                                          ({"model_type": "dinov2_with_registers", "num_register_tokens": 4}, "register variant")],
                         ids=["swiglu", "with_registers"])
def test_cli_entry_refuses_from_config_json_alone(tmp_path, change, match):
    """Before any weight is read or a device touched: model.safetensors here is not even a model."""
    from label_anything.preprocess import preprocess_images_to_embeddings_huggingface
    d = tmp_path / "model"
    os.makedirs(d)
    json.dump({**HF_CONFIG, **change}, open(d / "config.json", "w"))
    save_file({"layernorm.weight": torch.ones(8)}, str(d / "model.safetensors"))
    with pytest.raises(NotImplementedError, match=match):
        preprocess_images_to_embeddings_huggingface(str(d), str(tmp_path), outfolder=str(tmp_path / "out"))


def test_training_through_the_encoder_is_refused_by_name():
    from labelanything_amd.train import LamTrainer
    lam = Lam(MODEL_CASES["model_tiny_1w1s"]["cfg"], seed=1)
    with pytest.raises(NotImplementedError, match="dinov2.*LayerScale.*padded patch"):
        LamTrainer(lam, train_encoder=True)


def test_binding_declares_the_kernel_and_the_builders_know_the_kind():
    from labelanything_amd import _lib
    from labelanything_amd.engine import DINOV2_BLOCK, patch_kp
    from labelanything_amd.models import ENCODERS
    assert _lib.SIGNATURES["la_im2col_patch_pad"] == "piiiipis" and "la_im2col_patch_pad" in _lib.EXPORTS
    with pytest.raises(ValueError, match="even"):                # the wrapper's own checks come before the library
        _lib.im2col_patch_pad(torch.zeros(1, 3, 28, 28), 7, 192, torch.zeros(16, 192))
    assert (patch_kp(14), patch_kp(16), patch_kp(8), patch_kp(6), patch_kp(10)) == (640, 768, 192, 128, 320)
    assert DINOV2_BLOCK.norm1 == "norm1" and DINOV2_BLOCK.proj.endswith("output.ls") and DINOV2_BLOCK.lin2 == "mlp.fc2_ls"
    assert "vit_b_dinov2" in ENCODERS
