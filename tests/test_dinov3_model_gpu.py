"""GPU: the DINOv3 ViT encoder (kind "dinov3": la_rope_qk between the q | k | v GEMM and attention, register tokens, LayerScale folded into
o_proj / down_proj) against transformers' ``DINOv3ViTModel`` - the fixtures tests/golden/dinov3_* (tools/make_golden_dinov3.py; cases in
tests/cases_dinov3.py).

Bounds: 1e-3 max-norm, the project's stage bound for fp16 encoder stages, on the encoder output of every case and on the model case's
logits; argmax exact outside the 2e-3 margin band, whose share of the reference's own pixels the generator recorded (at most 5 %,
re-asserted here from the json).  The 99.9th percentile of the element-wise relative error is printed beside every max-norm figure.
"""
import json
import os

import pytest
import torch
from click.testing import CliRunner
from safetensors.torch import load_file, save_file

from labelanything_amd.models import ImageEncoder
from labelanything_amd.weights import init_state_dict
from tests import encoder_checks as EC
from tests.cases_dinov3 import ENCODER_CASES, MARGIN, MAX_BAND_SHARE, MODEL_CASES, encoder_config, encoder_images
from tests.encoder_checks import TOL, tokens
from tests.helpers import load_golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(ENCODER_CASES))
def test_encoder_matches_the_transformers_fixture(name):
    """la_rope_qk inside both block drivers: every case on the driver the engine chooses for it, which is asserted."""
    EC.check_encoder_case("dinov3", ENCODER_CASES, name)


def test_fold_case_on_the_plain_block_driver():
    """The ViT-B-wide case with the LayerNorm kernels (``norm_fold = False``): la_rope_qk behind the plain q | k | v GEMM, token-mean
    corrections pending in rvec - against the fixture, and against the folded driver."""
    EC.check_fold_case_on_the_plain_driver("dinov3", ENCODER_CASES)


def test_rotary_table_and_layer_scale_are_not_no_ops(monkeypatch):
    """Without la_rope_qk, and with LayerScale left at 1, the tiny case is far outside the bound: the fixture can tell."""
    from labelanything_amd import _lib
    case = ENCODER_CASES["tiny"]
    gold, _ = load_golden("dinov3_tiny")
    images = encoder_images(case)
    enc = ImageEncoder(case["encoder"], image_size=case["side"], seed=case["weight_seed"]).cuda()
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "rope_qk", lambda *a, **kw: None)
        no_rope = tokens(enc, images).clone()
    sd = enc.state_dict()
    enc.load_state_dict({k: (torch.ones_like(v) if k.endswith("lambda1") else v) for k, v in sd.items()})
    no_scale = tokens(enc, images)
    torch.cuda.synchronize()
    assert rel_err(no_rope, gold["patch_tokens"]) > 10 * TOL and rel_err(no_scale, gold["patch_tokens"]) > 10 * TOL


def test_model_case_logits_argmax_and_graph_replay():
    EC.check_model_case("dinov3", MODEL_CASES, "model_tiny_1w1s", MARGIN, MAX_BAND_SHARE)


@pytest.mark.parametrize("spelling", ["layer.", "model.layer."])
def test_generate_embeddings_from_a_dinov3_directory(tmp_path, spelling):
    """generate_embeddings --huggingface on a directory this test writes: config.json with model_type dinov3_vit and the tiny case's
    weights in the key spelling of the published checkpoints and in the one transformers 5.x prints.  The files hold what the encoder
    (whose parity the fixture cases establish) gives on the CLI's own preprocessing: ImageNet mean / std, square resize.  (96 px: one image's 36 patch rows are enough for the patch embedding's plane-pair operand.)"""
    from label_anything.cli import main
    from label_anything.preprocess import load_image, IMAGENET_DEFAULT
    from labelanything_amd.config import ENCODER_SPECS
    case = ENCODER_CASES["tiny"]
    spec = ENCODER_SPECS[case["encoder"]]
    sd = init_state_dict(encoder_config(case), case["weight_seed"])
    enc_sd = {k[len("image_encoder."):]: v for k, v in sd.items() if k.startswith("image_encoder.")}
    model_dir = tmp_path / "dinov3"
    os.makedirs(model_dir)
    with open(model_dir / "config.json", "w") as fh:
        json.dump({"model_type": "dinov3_vit", "hidden_size": spec.dim, "num_hidden_layers": spec.depth, "num_attention_heads": spec.heads,
                   "intermediate_size": spec.mlp, "patch_size": 16, "image_size": 224, "num_register_tokens": 4, "rope_theta": 100.0,
                   "layer_norm_eps": 1e-5, "key_bias": False, "use_gated_mlp": False, "hidden_act": "gelu"}, fh)
    save_file({(spelling + k[len("layer."):] if k.startswith("layer.") else k): v for k, v in enc_sd.items()},
              str(model_dir / "model.safetensors"))
    imgs, out = str(tmp_path / "imgs"), str(tmp_path / "emb")
    EC.write_images(imgs, [(100, 70)])
    r = CliRunner().invoke(main, ["generate_embeddings", "--huggingface", "--model_name", str(model_dir), "--directory", imgs,
                                  "--outfolder", out, "--image_resolution", "96", "--mean_std", "standard"])
    assert r.exit_code == 0, r.output + str(r.exception)
    got = load_file(os.path.join(out, "000000000000.safetensors"))["embedding"]
    assert got.shape == (spec.dim, 6, 6) and got.dtype == torch.float32
    x = load_image(os.path.join(imgs, "000000000000.png"), 96, False, *IMAGENET_DEFAULT, square=True).unsqueeze(0)
    enc = ImageEncoder(case["encoder"], image_size=96, seed=case["weight_seed"]).cuda()
    want = enc(x)[0]
    torch.cuda.synchronize()
    assert rel_err(got, want) <= 1e-6
