"""GPU: the DINOv2 ViT encoder (kind "dinov2": la_im2col_patch_pad in front of the patch GEMM, the position table resampled bicubically,
LayerScale folded into attention.output.dense / mlp.fc2) against transformers' ``Dinov2Model`` - the fixtures tests/golden/dinov2_*
(tools/make_golden_dinov2.py; cases in tests/cases_dinov2.py).

Bounds: 1e-3 max-norm, the project's stage bound for fp16 encoder stages, on the encoder output of every case and on the model case's
logits; argmax exact outside the 2e-3 margin band, whose share of the reference's own pixels the generator recorded (at most 5 %,
re-asserted here from the json).  The 99.9th percentile of the element-wise relative error is printed beside every max-norm figure.

Measured on one MI355X (max-norm): tiny 4.03e-4, resample 4.65e-4, hd32 3.68e-4, fold 3.92e-4 (plain driver 4.05e-4), model case logits
2.95e-4 and low-res logits 2.96e-4 (profiles/r15_dinov2.md).  The fold case's last bits differ from process to process (3.92e-4 - 3.99e-4
seen): its 16 x 16 position table is resampled by la_gemm_tn, which splits the 256 input positions over workgroups and accumulates with
float atomics, once per engine; every other case gives the same bits in every process (profiles/encoder_kinds.md).
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
from tests.cases_dinov2 import ENCODER_CASES, MARGIN, MAX_BAND_SHARE, MODEL_CASES, encoder_config, encoder_images
from tests.encoder_checks import TOL, tokens
from tests.helpers import load_golden, rel_err

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(ENCODER_CASES))
def test_encoder_matches_the_transformers_fixture(name):
    """Every case on the driver the engine chooses for it, which is asserted."""
    EC.check_encoder_case("dinov2", ENCODER_CASES, name)


def test_fold_case_on_the_plain_block_driver():
    """The ViT-B-wide case with the LayerNorm kernels (``norm_fold = False``) - against the fixture, and against the folded driver."""
    EC.check_fold_case_on_the_plain_driver("dinov2", ENCODER_CASES)


def test_layer_scale_position_table_and_the_tail_chunk_are_not_no_ops():
    """With LayerScale left at 1, and with the position table zeroed, the tiny case is far outside the bound: the fixture can tell.  With
    the patch weight's last four real columns (584 .. 587: the data half of the chunk that is half padding) zeroed, the output moves."""
    case = ENCODER_CASES["tiny"]
    gold, _ = load_golden("dinov2_tiny")
    images = encoder_images(case)
    enc = ImageEncoder(case["encoder"], image_size=case["side"], seed=case["weight_seed"]).cuda()
    sd = {k: v.clone() for k, v in enc.state_dict().items()}        # (copies: load_state_dict writes through the live tensors)
    base = tokens(enc, images).clone()
    enc.load_state_dict({k: (torch.ones_like(v) if k.endswith("lambda1") else v) for k, v in sd.items()})
    no_scale = tokens(enc, images).clone()
    enc.load_state_dict({k: (torch.zeros_like(v) if k.endswith("position_embeddings") else v) for k, v in sd.items()})
    no_pos = tokens(enc, images).clone()
    pw = sd["embeddings.patch_embeddings.projection.weight"].clone()
    assert pw.flatten(1).shape[1] == 588
    pw.view(pw.shape[0], -1)[:, 584:] = 0
    enc.load_state_dict({**sd, "embeddings.patch_embeddings.projection.weight": pw})
    no_tail = tokens(enc, images).clone()
    torch.cuda.synchronize()
    e_scale, e_pos, moved = rel_err(no_scale, gold["patch_tokens"]), rel_err(no_pos, gold["patch_tokens"]), rel_err(no_tail, base)
    print(f"[dinov2 tiny] LayerScale = 1: {e_scale:.3e}; position table zeroed: {e_pos:.3e}; patch columns 584..587 zeroed moves the "
          f"output by {moved:.3e}")
    assert rel_err(base, gold["patch_tokens"]) <= TOL
    assert e_scale > 10 * TOL and e_pos > 10 * TOL
    assert moved > 0


def test_model_case_logits_argmax_and_graph_replay():
    EC.check_model_case("dinov2", MODEL_CASES, "model_tiny_1w1s", MARGIN, MAX_BAND_SHARE)


def test_generate_embeddings_from_a_dinov2_directory(tmp_path):
    """generate_embeddings --huggingface on a directory this test writes: config.json with model_type dinov2 (mlp_ratio, no
    intermediate_size; image_size 70) and the tiny case's weights under Dinov2Model's keys, mask_token among them.  The file holds what
    the encoder (whose parity the fixture cases establish) gives on the CLI's own preprocessing: ImageNet mean / std whatever --mean_std
    says, square resize.  (84 px: one image's 36 patch rows are enough for the patch embedding's plane-pair operand.)"""
    from label_anything.cli import main
    from label_anything.preprocess import load_image, IMAGENET_DEFAULT
    from labelanything_amd.config import ENCODER_SPECS
    case = ENCODER_CASES["tiny"]
    spec = ENCODER_SPECS[case["encoder"]]
    sd = init_state_dict(encoder_config(case), case["weight_seed"])
    enc_sd = {k[len("image_encoder."):]: v for k, v in sd.items() if k.startswith("image_encoder.")}
    assert "embeddings.mask_token" in enc_sd
    model_dir = tmp_path / "dinov2"
    os.makedirs(model_dir)
    with open(model_dir / "config.json", "w") as fh:
        json.dump({"model_type": "dinov2", "hidden_size": spec.dim, "num_hidden_layers": spec.depth, "num_attention_heads": spec.heads,
                   "mlp_ratio": 4, "patch_size": 14, "image_size": 70, "layer_norm_eps": 1e-6, "qkv_bias": True, "use_swiglu_ffn": False,
                   "hidden_act": "gelu"}, fh)
    save_file(enc_sd, str(model_dir / "model.safetensors"))
    imgs, out = str(tmp_path / "imgs"), str(tmp_path / "emb")
    EC.write_images(imgs, [(100, 70)])
    r = CliRunner().invoke(main, ["generate_embeddings", "--huggingface", "--model_name", str(model_dir), "--directory", imgs,
                                  "--outfolder", out, "--image_resolution", "84", "--mean_std", "standard"])
    assert r.exit_code == 0, r.output + str(r.exception)
    got = load_file(os.path.join(out, "000000000000.safetensors"))["embedding"]
    assert got.shape == (spec.dim, 6, 6) and got.dtype == torch.float32
    x = load_image(os.path.join(imgs, "000000000000.png"), 84, False, *IMAGENET_DEFAULT, square=True).unsqueeze(0)
    enc = ImageEncoder(case["encoder"], image_size=84, seed=case["weight_seed"]).cuda()
    want = enc(x)[0]
    torch.cuda.synchronize()
    assert rel_err(got, want) <= 1e-6
