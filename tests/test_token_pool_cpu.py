"""CPU: configuration surface and weights of ``prompt_encoder="TokenPool"`` and the torch restatement (tests/token_pool_ref.py) against the
reference's fixtures (tests/golden/token_pool_*; tools/make_golden_token_pool.py)."""
import dataclasses
import json
import os
import re
import tempfile

import pytest
import torch
from safetensors.torch import load_file

from labelanything_amd import _lib
from labelanything_amd.config import LamConfig, config_from_kwargs
from labelanything_amd.episodes import make_episode
from labelanything_amd.weights import init_state_dict, model_shapes
from tests import token_pool_ref as R
from tests.cases import geometry_for
from tests.cases_token_pool import SRC_STRIDE, TP_CASES, TP_TRAIN, TP_TRAIN_FULL
from tests.helpers import GOLDEN, argmax_disagreement, load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(image_size=64, embed_dim=64, image_embed_dim=64)
TP = dict(prompt_encoder="TokenPool")
ORACLE_PIN = 2e-6                         # the project's pin of a torch restatement against the reference's fp32 (max-norm)
FINAL = ("prompt_encoder.transformer.final_attn_token_to_image.", "prompt_encoder.transformer.norm_final_attn.")


def cfg_of(**kw):
    return config_from_kwargs(encoder=None, use_vit=False, **SMALL, **kw)


# ---- the validator --------------------------------------------------------------------------------------------------------------------
def test_accepted_values_and_defaults():
    assert LamConfig().prompt_encoder is None and cfg_of().prompt_encoder is None
    assert cfg_of(prompt_encoder=None) == cfg_of()
    c = cfg_of(**TP)
    assert c.prompt_encoder == "TokenPool" and not c.segment_example_logits and c.pool_side == 1
    assert dataclasses.replace(c, prompt_encoder=None) == cfg_of()


@pytest.mark.parametrize("value", ["tokenpool", "Pool", "", 1, True])
def test_every_other_value_is_a_value_error(value):
    from labelanything_amd.models import Lam
    with pytest.raises(ValueError, match="prompt_encoder"):
        cfg_of(prompt_encoder=value)
    with pytest.raises(ValueError, match="prompt_encoder"):
        Lam(cfg_of(), prompt_encoder=value)


@pytest.mark.parametrize("kw,match", [
    (dict(segment_example_logits=True), "segment_example_logits"), (dict(embeddings_per_example=4), "embeddings_per_example"),
    (dict(embedding_extraction="cross_attention", embeddings_per_example=4), "embedding_extraction"),
    (dict(classification_levels=2), "classification_levels"), (dict(conv_classification=True), "conv_classification"),
    (dict(conv_classification=True, classification_layer_downsample_rate=1), "conv_classification")])
def test_combinations_that_are_not_built_name_the_pair(kw, match):
    from labelanything_amd.models import Lam
    with pytest.raises(NotImplementedError, match=match) as e:
        cfg_of(**TP, **kw)
    assert "TokenPool" in str(e.value)
    with pytest.raises(NotImplementedError, match=match) as e:
        Lam(cfg_of(**kw), **TP)
    assert "TokenPool" in str(e.value)


def test_the_pair_with_extraction_is_named_before_the_missing_number_of_queries():
    with pytest.raises(NotImplementedError, match="embedding_extraction") as e:
        cfg_of(embedding_extraction="cross_attention", **TP)
    assert "TokenPool" in str(e.value)


def test_use_support_features_false_stays_refused():
    with pytest.raises(NotImplementedError, match="use_support_features_in_prompt_encoder"):
        cfg_of(use_support_features_in_prompt_encoder=False, **TP)
    assert cfg_of(use_support_features_in_prompt_encoder=True, **TP).prompt_encoder == "TokenPool"


def test_public_constructors():
    from labelanything_amd.models import LabelAnything, Lam, build_lam, build_lam_no_vit
    assert build_lam_no_vit(**TP, **SMALL).cfg.prompt_encoder == "TokenPool"
    assert build_lam(encoder=None, use_vit=False, **TP, **SMALL).cfg.prompt_encoder == "TokenPool"
    base = cfg_of()
    lam = Lam(base, **TP)
    assert lam.cfg.prompt_encoder == "TokenPool" and base.prompt_encoder is None and Lam(base).cfg == base
    assert Lam(cfg_of(**TP)).cfg.prompt_encoder == "TokenPool"
    m = LabelAnything(encoder=None, use_vit=False, **TP, **SMALL)
    assert m.model.cfg.prompt_encoder == "TokenPool" and m.config["prompt_encoder"] == "TokenPool"
    assert LabelAnything(encoder=None, use_vit=False, **SMALL).model.cfg.prompt_encoder is None
    from label_anything.models import build_lam_no_vit as shim, model_registry
    assert shim(**TP, **SMALL).cfg.prompt_encoder == "TokenPool"
    assert model_registry["lam_no_vit"](**TP, **SMALL).cfg.prompt_encoder == "TokenPool"
    # the constructor call of the recipe (the model section of parameters/trainval/pascal/mae_pool.yaml)
    full = build_lam_no_vit(image_size=480, image_embed_dim=768, embed_dim=256, spatial_convs=3, prompt_encoder="TokenPool",
                            class_attention=False, example_attention=False, example_class_attention=True,
                            class_encoder={"name": "RandomMatrixEncoder", "bank_size": 100, "embed_dim": 256})
    assert full.cfg.grid == 30 and full.cfg.prompt_encoder == "TokenPool" and full.cfg.lam_neck


def test_config_json_round_trip():
    from labelanything_amd.models import LabelAnything, build_lam
    m = LabelAnything(encoder=None, use_vit=False, **TP, **SMALL)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    with tempfile.TemporaryDirectory() as d:
        m.save_local(d)
        with open(os.path.join(d, "config.json")) as fh:
            assert json.load(fh)["prompt_encoder"] == "TokenPool"
        m2 = LabelAnything.from_local(d)
        assert m2.model.cfg == m.model.cfg and m2.config == m.config and m2.model.cfg.prompt_encoder == "TokenPool"
        assert all(torch.equal(v, want[k]) for k, v in m2.state_dict().items()) and list(m2.state_dict()) == list(want)
    lam = build_lam(encoder=None, use_vit=False, **TP, **SMALL)
    assert config_from_kwargs(**json.loads(json.dumps(dataclasses.asdict(lam.cfg)))) == lam.cfg


# ---- shapes and weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TP_CASES))
def test_no_tensor_is_added_and_the_initialisation_is_the_plain_model_s(name):
    cfg = TP_CASES[name]["cfg"]
    plain = dataclasses.replace(cfg, prompt_encoder=None)
    assert list(model_shapes(cfg).items()) == list(model_shapes(plain).items())
    a, b = init_state_dict(cfg, 13), init_state_dict(plain, 13)
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in b)
    assert any(k.startswith(FINAL) for k in a)
    _, meta = load_golden(f"token_pool_{name}")
    assert meta["state_dict_keys_equal_plain"] is True           # the reference's two models, compared by the generator


def test_state_dict_is_strict_in_both_directions():
    from labelanything_amd.models import Lam
    on, off = Lam(cfg_of(**TP), seed=3), Lam(cfg_of(), seed=4)
    sd = on.state_dict()
    off.load_state_dict(sd)                                       # strict: same keys, same shapes
    assert all(torch.equal(v, sd[k]) for k, v in off.state_dict().items()) and list(off.state_dict()) == list(sd)
    on.load_state_dict(Lam(cfg_of(), seed=5).state_dict())
    with pytest.raises(RuntimeError):
        on.load_state_dict({k: v for k, v in sd.items() if not k.startswith(FINAL)})


# ---- the torch restatement ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    out = {}
    for name, case in TP_CASES.items():
        gold, meta = load_golden(f"token_pool_{name}")
        batch = make_episode(**case["episode"])
        with torch.no_grad():
            out[name] = (R.lam_forward(init_state_dict(case["cfg"], case["weight_seed"]), geometry_for(case["cfg"]), batch,
                                       gold.get("selected_rows")), gold, meta, batch)
    return out


@pytest.mark.parametrize("name", list(TP_CASES))
def test_restatement_reproduces_the_reference(restated, name):
    """fp32 restatement of the whole forward against what the reference returned, every stored quantity at the oracle pin."""
    got, gold, meta, batch = restated[name]
    cfg = TP_CASES[name]["cfg"]
    b, m, c = batch["flag_examples"].shape
    g, d, st = cfg.grid, cfg.embed_dim, SRC_STRIDE
    assert got["class_examples_src"].shape == (b * m, g * g, d) and meta["full_src_shape"] == [b * m, g * g, d]
    sample = got["class_examples_src"].view(b * m, g, g, d)[:, ::st, ::st, ::st].flatten(1, 2)
    errs = {"class_examples_src": rel_err(sample, gold["class_examples_src_sample"]),
            "class_examples_embeddings": rel_err(got["class_examples_embeddings"], gold["class_examples_embeddings"]),
            "class_embeddings": rel_err(got["class_embeddings"], gold["class_embeddings"]),
            "low_res_logits": rel_err(got["low_res_logits"], gold["low_res_logits"]),
            "logits": rel_err(got["logits"], gold["logits"])}
    print(f"[{name}] restatement vs reference: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (pin {ORACLE_PIN:.0e})")
    assert got["class_embeddings"].dtype == torch.float32
    assert max(errs.values()) <= ORACLE_PIN, errs
    assert argmax_disagreement(got["logits"], gold["argmax"], gold["logits"], 2e-3)[1] == 0


def test_restatement_takes_float64_and_the_fp32_reference_is_its_rounding():
    name = "tp_d64"
    case = TP_CASES[name]
    gold, _ = load_golden(f"token_pool_{name}")
    batch = R.to_dtype(make_episode(**case["episode"]), torch.float64)
    w = R.to_dtype(init_state_dict(case["cfg"], case["weight_seed"]), torch.float64)
    with torch.no_grad():
        got = R.lam_forward(w, geometry_for(case["cfg"]), batch, gold["selected_rows"])
    assert got["class_embeddings"].dtype == torch.float64 and got["low_res_logits"].dtype == torch.float64
    assert rel_err(got["low_res_logits"], gold["low_res_logits"]) <= 2e-5
    assert rel_err(got["class_examples_embeddings"], gold["class_examples_embeddings"]) <= 2e-5


def test_the_cases_cover_what_they_are_there_for():
    ep = {n: make_episode(**c["episode"]) for n, c in TP_CASES.items()}
    assert tuple(ep["tp_d256"]["flag_examples"].shape) == (1, 6, 3) and int((ep["tp_d256"]["flag_masks"] == 0).sum()) >= 1
    assert tuple(ep["tp_d64"]["flag_examples"].shape) == (2, 4, 3) and "prompt_bboxes" in ep["tp_d64"] and TP_CASES["tp_d64"]["cfg"].lam_neck
    masks = TP_CASES["tp_masks"]
    assert masks["episode"]["prompts"] == ("mask",) and masks["cfg"].class_encoder is None and not masks["cfg"].example_class_attention
    assert "prompt_points" not in ep["tp_masks"] or not bool((ep["tp_masks"]["flag_points"] != 0).any())
    for n in TP_CASES:
        assert os.path.getsize(os.path.join(GOLDEN, f"token_pool_{n}.safetensors")) < 1 << 20


def test_stored_training_step_has_live_final_attention():
    name = TP_TRAIN["case"]
    gold = load_file(os.path.join(GOLDEN, f"token_pool_{name}_train.safetensors"))
    with open(os.path.join(GOLDEN, f"token_pool_{name}_train.json")) as fh:
        meta = json.load(fh)
    assert not any(k.startswith(FINAL) for k in meta["dead"])
    finals = [k for k in meta["keys"] if k.startswith(FINAL)]
    assert len(finals) == 10 and all(float(gold["grad_norm"][meta["keys"].index(k)]) > 0 for k in finals)
    assert "grad.prompt_encoder.transformer.final_attn_token_to_image.out_proj.weight" in gold
    assert any(k.startswith("grad.prompt_encoder.mask_downscaling.") for k in gold)
    assert sorted("grad." + k for k in TP_TRAIN_FULL) == sorted(k for k in gold if k.startswith("grad."))
    assert 0 < meta["e_ref32"] < 3e-4 and abs(meta["loss"] - meta["loss_fp64"]) <= 2e-5 * abs(meta["loss_fp64"])
    shapes = model_shapes(TP_CASES[name]["cfg"])
    assert sorted(meta["keys"] + meta["dead"]) == sorted(k for k in shapes if not k.endswith("positional_encoding_gaussian_matrix"))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_new_entry_point_is_exported_and_declared():
    with open(os.path.join(ROOT, "include", "la_hip.h")) as fh:
        header = fh.read()
    assert "la_mask_embed_pooled" in _lib.EXPORTS
    assert re.search(r"\bint la_mask_embed_pooled\(", header)
    assert "prompt_encoder.py:880-896" in header
    assert callable(_lib.mask_embed_pooled)
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"C ABI ({len(_lib.EXPORTS) + 2} entry points" in fh.read()          # + la_last_error, la_version
