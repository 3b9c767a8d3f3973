"""CPU: the DINOv3 ViT encoder's configuration, weights layout, refusals and rotary table (no device code runs)."""
import json
import math
import os

import pytest
import torch
from safetensors.torch import save_file

from labelanything_amd.config import ENCODER_SPECS, EncoderSpec, LamConfig, dinov3_spec_from_hf_config
from labelanything_amd.engine import rope_table
from labelanything_amd.models import ImageEncoder, Lam
from labelanything_amd.weights import encoder_shapes, init_state_dict
from tests.cases_dinov3 import ENCODER_CASES, MODEL_CASES, encoder_config

HF_CONFIG = {"model_type": "dinov3_vit", "hidden_size": 768, "num_hidden_layers": 12, "num_attention_heads": 12, "intermediate_size": 3072,
             "patch_size": 16, "image_size": 224, "num_register_tokens": 4, "rope_theta": 100.0, "layer_norm_eps": 1e-5, "key_bias": False,
             "use_gated_mlp": False, "hidden_act": "gelu"}


def test_registered_specs_and_the_defaults_of_every_other_kind():
    want = {"vit_s_dinov3": (384, 12, 6, 1536), "vit_b_dinov3": (768, 12, 12, 3072), "vit_l_dinov3": (1024, 24, 16, 4096)}
    for name, (dim, depth, heads, mlp) in want.items():
        s = ENCODER_SPECS[name]
        assert (s.kind, s.dim, s.depth, s.heads, s.mlp, s.patch, s.head_dim) == ("dinov3", dim, depth, heads, mlp, 16, 64)
        assert (s.prefix_tokens, s.rope_theta, s.layer_scale, s.key_bias, s.ln_eps) == (5, 100.0, True, False, 1e-5)
    # the new fields are defaulted: an existing construction means what it meant
    old = EncoderSpec("hf", 768, 12, 12, 3072, img_size=224)
    assert old == ENCODER_SPECS["vit_b_mae"] and (old.prefix_tokens, old.layer_scale, old.key_bias) == (1, False, True)
    assert dinov3_spec_from_hf_config(HF_CONFIG) == ENCODER_SPECS["vit_b_dinov3"]


def test_state_dict_layout_is_the_transformers_one():
    """Keys and shapes under image_encoder. in DINOv3ViTModel's order (``layer.N.`` spelling): k_proj has no bias, mask_token is held."""
    spec = ENCODER_SPECS["dinov3_tiny"]
    shapes = encoder_shapes(spec)
    pre = "image_encoder."
    keys = [k[len(pre):] for k in shapes]
    assert keys[:5] == ["embeddings.cls_token", "embeddings.mask_token", "embeddings.register_tokens", "embeddings.patch_embeddings.weight",
                        "embeddings.patch_embeddings.bias"]
    layer0 = [k[len("layer.0."):] for k in keys if k.startswith("layer.0.")]
    assert layer0 == ["norm1.weight", "norm1.bias", "attention.k_proj.weight", "attention.v_proj.weight", "attention.v_proj.bias",
                      "attention.q_proj.weight", "attention.q_proj.bias", "attention.o_proj.weight", "attention.o_proj.bias",
                      "layer_scale1.lambda1", "norm2.weight", "norm2.bias", "mlp.up_proj.weight", "mlp.up_proj.bias",
                      "mlp.down_proj.weight", "mlp.down_proj.bias", "layer_scale2.lambda1"]
    assert keys[-2:] == ["norm.weight", "norm.bias"] and len(keys) == 5 + 17 * spec.depth + 2
    assert shapes[pre + "embeddings.register_tokens"] == (1, 4, 128) and shapes[pre + "layer.1.mlp.up_proj.weight"] == (512, 128)
    meta = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "dinov3_tiny.json")))
    # what transformers itself listed when the fixture was made (its 5.x spelling: model.layer.N.)
    assert [[k.replace("model.layer.", "layer."), s] for k, s in meta["state_dict"]] == [[k, list(shapes[pre + k])] for k in keys]
    sd = init_state_dict(encoder_config(ENCODER_CASES["tiny"]), 0)
    lam1 = torch.cat([v for k, v in sd.items() if k.endswith("lambda1")])
    assert 0.05 <= float(lam1.min()) < 0.2 and 1.35 < float(lam1.max()) <= 1.5          # LayerScale is drawn, never the initial 1.0


@pytest.mark.parametrize("spelling", ["layer.", "model.layer."])
def test_strict_load_in_both_key_spellings(spelling):
    case = ENCODER_CASES["tiny"]
    src = ImageEncoder(case["encoder"], image_size=case["side"], seed=5).state_dict()
    sd = {(spelling + k[len("layer."):] if k.startswith("layer.") else k): v for k, v in src.items()}
    enc = ImageEncoder(case["encoder"], image_size=case["side"], seed=6)
    enc.load_state_dict(sd)
    assert all(torch.equal(v, src[k]) for k, v in enc.state_dict().items()) and "embeddings.mask_token" in src
    with pytest.raises(RuntimeError, match="missing"):
        enc.load_state_dict({k: v for k, v in sd.items() if "layer_scale2" not in k})
    with pytest.raises(RuntimeError, match="unexpected"):
        enc.load_state_dict({**sd, spelling + "0.attention.k_proj.bias": torch.zeros(128)})
    # the whole model, strictly, through Lam.load_state_dict
    mcase = MODEL_CASES["model_tiny_1w1s"]
    full = init_state_dict(mcase["cfg"], 7)
    pre = "image_encoder."
    lam = Lam(mcase["cfg"], seed=8)
    lam.load_state_dict({(pre + spelling + k[len(pre + "layer."):] if k.startswith(pre + "layer.") else k): v for k, v in full.items()})
    assert all(torch.equal(v, full[k]) for k, v in lam.state_dict().items())


def test_gated_mlp_and_other_unbuilt_variants_are_refused(tmp_path):
    with pytest.raises(NotImplementedError, match="use_gated_mlp"):
        dinov3_spec_from_hf_config({**HF_CONFIG, "use_gated_mlp": True})
    with pytest.raises(NotImplementedError, match="hidden_act"):
        dinov3_spec_from_hf_config({**HF_CONFIG, "hidden_act": "silu"})
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        dinov3_spec_from_hf_config({**HF_CONFIG, "hidden_size": 120, "num_attention_heads": 5})
    with pytest.raises(ValueError, match="model_type"):
        dinov3_spec_from_hf_config({**HF_CONFIG, "model_type": "vit"})
    # the CLI's entry refuses an S+ / H+ directory from its config.json alone, before it reads weights or touches a device
    from label_anything.preprocess import preprocess_images_to_embeddings_huggingface
    d = tmp_path / "splus"
    os.makedirs(d)
    json.dump({**HF_CONFIG, "hidden_size": 384, "num_attention_heads": 6, "intermediate_size": 1536, "use_gated_mlp": True},
              open(d / "config.json", "w"))
    save_file({"norm.weight": torch.ones(384)}, str(d / "model.safetensors"))
    with pytest.raises(NotImplementedError, match="S\\+ and H\\+"):
        preprocess_images_to_embeddings_huggingface(str(d), str(tmp_path), outfolder=str(tmp_path / "out"))


@pytest.mark.parametrize("g,hd,theta", [(3, 64, 100.0), (4, 32, 100.0), (30, 64, 100.0), (5, 16, 10000.0)])
def test_rope_table_against_a_literal_restatement(g, hd, theta):
    """Patch centres (i + 0.5) / g mapped to [-1, 1], row-major (y, x); inv_freq = theta^(-arange(0, 1, 4 / hd)); angles 2 pi coord x
    inv_freq, the y block then the x block (hd / 2 columns), tiled twice - restated in fp64 with loops.  The table's angles are fp32
    (|angle| <= 2 pi: spacing 4.8e-7, a few roundings on the way), so cos and sin agree within 2e-6."""
    cos, sin = rope_table(g, hd, theta)
    assert cos.shape == sin.shape == (g * g, hd) and cos.dtype == sin.dtype == torch.float32
    nf = hd // 4
    inv_freq = [theta ** -(j * 4.0 / hd) for j in range(nf)]
    want_c, want_s = torch.empty(g * g, hd, dtype=torch.float64), torch.empty(g * g, hd, dtype=torch.float64)
    for y in range(g):
        for x in range(g):
            cy, cx = 2.0 * (y + 0.5) / g - 1.0, 2.0 * (x + 0.5) / g - 1.0
            ang = [2 * math.pi * cy * f for f in inv_freq] + [2 * math.pi * cx * f for f in inv_freq]
            ang = ang + ang
            want_c[y * g + x] = torch.tensor([math.cos(a) for a in ang], dtype=torch.float64)
            want_s[y * g + x] = torch.tensor([math.sin(a) for a in ang], dtype=torch.float64)
    assert float((cos.double() - want_c).abs().max()) <= 2e-6 and float((sin.double() - want_s).abs().max()) <= 2e-6
    assert torch.equal(cos[:, : hd // 2], cos[:, hd // 2:]) and torch.equal(sin[:, : hd // 2], sin[:, hd // 2:])


def test_training_through_the_encoder_is_refused_by_name():
    from labelanything_amd.train import LamTrainer
    lam = Lam(MODEL_CASES["model_tiny_1w1s"]["cfg"], seed=1)
    with pytest.raises(NotImplementedError, match="dinov3"):
        LamTrainer(lam, train_encoder=True)


def test_binding_declares_the_kernel():
    from labelanything_amd import _lib
    assert _lib.SIGNATURES["la_rope_qk"] == "pliiiiiippis" and "la_rope_qk" in _lib.EXPORTS
    cos, sin = rope_table(3, 64, 100.0)
    with pytest.raises(ValueError, match="tokens - prefix"):         # the wrapper's own checks come before the library
        _lib.rope_qk(torch.zeros(14, 384, dtype=torch.float16), 14, 4, 2, 64, 64, cos, sin)
