"""CPU: configuration surface and weights of ``fusion_transformer="OneWayTransformer"`` and the torch restatement (tests/oneway_ref.py)
against the reference's fixtures (tests/golden/oneway_*; tools/make_golden_oneway.py)."""
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
from tests import oneway_ref as R
from tests.cases import geometry_for
from tests.cases_oneway import KINK_BAND, MARGIN, MAX_BAND_SHARE, OW_CASES, OW_TRAIN, OW_TRAIN_FULL, SRC_STRIDE
from tests.helpers import GOLDEN, argmax_disagreement, load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(image_size=64, embed_dim=64, image_embed_dim=64)
OW = dict(fusion_transformer="OneWayTransformer")
ORACLE_PIN = 2e-6                         # the project's pin of a torch restatement against the reference's fp32 (max-norm)
TR = "mask_decoder.transformer."
NORM3 = tuple(f"{TR}layers.{l}.norm3." for l in range(2))


def cfg_of(**kw):
    return config_from_kwargs(encoder=None, use_vit=False, **SMALL, **kw)


# ---- the validator --------------------------------------------------------------------------------------------------------------------
def test_accepted_values_and_defaults():
    assert LamConfig().fusion_transformer == "TwoWayTransformer" and cfg_of().fusion_transformer == "TwoWayTransformer"
    assert cfg_of(fusion_transformer="TwoWayTransformer") == cfg_of() and not cfg_of().one_way
    c = cfg_of(**OW)
    assert c.fusion_transformer == "OneWayTransformer" and c.one_way
    assert dataclasses.replace(c, fusion_transformer="TwoWayTransformer") == cfg_of()


def test_a_model_with_an_image_encoder_keeps_raising():
    from labelanything_amd.models import Lam
    for enc in ("vit_b", "vit_b_mae"):
        with pytest.raises(NotImplementedError, match="image encoder"):
            config_from_kwargs(encoder=enc, **OW)
    with pytest.raises(NotImplementedError, match="image encoder"):
        Lam(config_from_kwargs(encoder="vit_b_mae", image_size=224), **OW)
    assert config_from_kwargs(encoder="vit_b", use_vit=False, **OW).one_way          # (lam_no_vit ignores the encoder's name)


@pytest.mark.parametrize("value", ["IdentityTransformer", "onewaytransformer", "AffinityTransformer", "", None])
def test_every_other_value_stays_refused(value):
    from labelanything_amd.models import Lam
    with pytest.raises(NotImplementedError, match="fusion_transformer"):
        cfg_of(fusion_transformer=value)
    if value is not None:               # (None leaves what cfg says)
        with pytest.raises(NotImplementedError, match="fusion_transformer"):
            Lam(cfg_of(), fusion_transformer=value)


@pytest.mark.parametrize("kw,match", [
    (dict(segment_example_logits=True), "segment_example_logits"), (dict(embeddings_per_example=4), "embeddings_per_example"),
    (dict(embedding_extraction="cross_attention", embeddings_per_example=4), "segment_example_logits|embedding_extraction"),
    (dict(classification_levels=2), "classification_levels"), (dict(conv_classification=True), "conv_classification"),
    (dict(classification_layer_downsample_rate=1), "classification_layer_downsample_rate"),
    (dict(prompt_encoder="TokenPool"), "TokenPool")])
def test_combinations_that_are_not_built_name_the_pair(kw, match):
    from labelanything_amd.models import Lam
    with pytest.raises(NotImplementedError, match=match) as e:
        cfg_of(**OW, **kw)
    assert "OneWayTransformer" in str(e.value)
    with pytest.raises(NotImplementedError, match=match) as e:
        Lam(cfg_of(**kw), **OW)
    assert "OneWayTransformer" in str(e.value)


def test_public_constructors():
    from labelanything_amd.models import LabelAnything, Lam, build_lam, build_lam_no_vit
    assert build_lam_no_vit(**OW, **SMALL).cfg.one_way
    assert build_lam(encoder=None, use_vit=False, **OW, **SMALL).cfg.one_way
    base = cfg_of()
    lam = Lam(base, **OW)
    assert lam.cfg.one_way and not base.one_way and Lam(base).cfg == base
    m = LabelAnything(encoder=None, use_vit=False, **OW, **SMALL)
    assert m.model.cfg.one_way and m.config["fusion_transformer"] == "OneWayTransformer"
    assert not LabelAnything(encoder=None, use_vit=False, **SMALL).model.cfg.one_way
    from label_anything.models import build_lam_no_vit as shim, model_registry
    assert shim(**OW, **SMALL).cfg.one_way
    assert model_registry["lam_no_vit"](**OW, **SMALL).cfg.one_way
    # the constructor call of the recipe (the model section of parameters/trainval/Ablations/mae_transformer.yaml)
    full = build_lam_no_vit(image_size=480, image_embed_dim=768, embed_dim=256, spatial_convs=3, fusion_transformer="OneWayTransformer",
                            class_attention=False, example_attention=False, example_class_attention=False)
    assert full.cfg.grid == 30 and full.cfg.one_way and full.cfg.lam_neck


def test_config_json_round_trip():
    from labelanything_amd.models import LabelAnything, build_lam
    m = LabelAnything(encoder=None, use_vit=False, **OW, **SMALL)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    with tempfile.TemporaryDirectory() as d:
        m.save_local(d)
        with open(os.path.join(d, "config.json")) as fh:
            assert json.load(fh)["fusion_transformer"] == "OneWayTransformer"
        m2 = LabelAnything.from_local(d)
        assert m2.model.cfg == m.model.cfg and m2.config == m.config and m2.model.cfg.one_way
        assert all(torch.equal(v, want[k]) for k, v in m2.state_dict().items()) and list(m2.state_dict()) == list(want)
    lam = build_lam(encoder=None, use_vit=False, **OW, **SMALL)
    assert config_from_kwargs(**json.loads(json.dumps(dataclasses.asdict(lam.cfg)))) == lam.cfg


# ---- shapes and weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OW_CASES))
def test_state_dict_is_the_reference_s(name):
    """Keys and shapes equal the reference's; mask_decoder.transformer.* is 36 tensors in the reference's order."""
    cfg = OW_CASES[name]["cfg"]
    _, meta = load_golden(f"oneway_{name}")
    ref = [(k, tuple(s)) for k, s in meta["state_dict"]]
    own = list(model_shapes(cfg).items())
    assert sorted(own) == sorted(ref)
    tr_own, tr_ref = [kv for kv in own if kv[0].startswith(TR)], [kv for kv in ref if kv[0].startswith(TR)]
    assert tr_own == tr_ref and len(tr_own) == 36
    sd = init_state_dict(cfg, 3)
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == own
    d, mlp = cfg.embed_dim, cfg.dec_mlp
    assert tuple(sd[TR + "layers.1.mlp.lin1.weight"].shape) == (mlp, d) and tuple(sd[TR + "layers.0.mlp.lin2.weight"].shape) == (d, mlp)
    assert tuple(sd[TR + "layers.0.cross_attn_image_to_token.out_proj.weight"].shape) == (d, d // 2)
    assert all(any(k.startswith(p) for k in sd) for p in NORM3)
    if name == "ow_d256":
        assert len(own) == 188


def test_existing_configurations_keep_their_initialisation():
    """The two-way model's init_state_dict does not depend on the new field; the tensors ahead of the mask decoder's transformer are the
    same bits in both models (one generator, drawn in key order)."""
    cfg = cfg_of(class_encoder={"name": "RandomMatrixEncoder", "bank_size": 10, "embed_dim": 64})
    a = init_state_dict(cfg, 13)
    assert TR + "layers.0.self_attn.q_proj.weight" in a and TR + "final_attn_token_to_image.q_proj.weight" in a and len(a) == len(model_shapes(cfg))
    b = init_state_dict(dataclasses.replace(cfg, fusion_transformer="OneWayTransformer"), 13)
    for k in a:
        if k.startswith(TR):
            break
        assert torch.equal(a[k], b[k]), k


def test_cross_loading_fails_with_the_missing_and_unexpected_keys():
    from labelanything_amd.models import Lam
    one, two = Lam(cfg_of(**OW), seed=3), Lam(cfg_of(), seed=4)
    # (every tensor name of a one-way block also exists in a two-way block, so each direction reports one list)
    with pytest.raises(RuntimeError, match=r"(?s)Unexpected key.*mask_decoder\.transformer\.layers\.0\.self_attn") as e:
        one.load_state_dict(two.state_dict())
    assert "norm4" in str(e.value) and "final_attn_token_to_image" in str(e.value) and "Missing" not in str(e.value)
    with pytest.raises(RuntimeError, match=r"(?s)Missing key.*mask_decoder\.transformer\.layers\.0\.self_attn") as e:
        two.load_state_dict(one.state_dict())
    assert "norm4" in str(e.value) and "Unexpected" not in str(e.value)
    sd = one.state_dict()
    other = Lam(cfg_of(**OW), seed=5)
    other.load_state_dict(sd)                                     # strict
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    with pytest.raises(RuntimeError):
        other.load_state_dict({k: v for k, v in sd.items() if not k.startswith(NORM3)})      # norm3 is held and loaded


def test_sam_initialisation_of_a_one_way_model_raises():
    """Segment-Anything's mask-decoder transformer is two-way: the reference's strict load of it into the one-way module fails."""
    from labelanything_amd.models import Lam, init_pretrained_weights
    kw = dict(image_size=64, embed_dim=256, image_embed_dim=256)
    sam = Lam(config_from_kwargs(encoder=None, use_vit=False, **kw), seed=1).state_dict()
    lam = Lam(config_from_kwargs(encoder=None, use_vit=False, **kw, **OW), seed=2)
    with pytest.raises(RuntimeError, match=r"does not match mask_decoder\.transformer\.\*"):
        init_pretrained_weights(lam, sam)
    init_pretrained_weights(Lam(config_from_kwargs(encoder=None, use_vit=False, **kw), seed=2), sam)     # the two-way model takes it


# ---- the torch restatement ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def restated():
    out = {}
    for name, case in OW_CASES.items():
        gold, meta = load_golden(f"oneway_{name}")
        batch = make_episode(**case["episode"])
        with torch.no_grad():
            out[name] = (R.lam_forward(init_state_dict(case["cfg"], case["weight_seed"]), geometry_for(case["cfg"]), batch,
                                       gold.get("selected_rows")), gold, meta, batch)
    return out


@pytest.mark.parametrize("name", list(OW_CASES))
def test_restatement_reproduces_the_reference(restated, name):
    """fp32 restatement of the whole forward against what the reference returned, every stored quantity at the oracle pin."""
    got, gold, meta, batch = restated[name]
    cfg = OW_CASES[name]["cfg"]
    b = batch["flag_examples"].shape[0]
    g, d, st = cfg.grid, cfg.embed_dim, SRC_STRIDE
    assert tuple(got["transformer_image"].shape) == (b, g * g, d) and meta["full_image_shape"] == [b, g * g, d]
    sample = got["transformer_image"].view(b, g, g, d)[:, ::st, ::st, ::st].flatten(1, 2)
    errs = {"transformer_image": rel_err(sample, gold["transformer_image_sample"]),
            "class_embeddings": rel_err(got["class_embeddings"], gold["class_embeddings"]),
            "low_res_logits": rel_err(got["low_res_logits"], gold["low_res_logits"]),
            "logits": rel_err(got["logits"], gold["logits"])}
    print(f"[{name}] restatement vs reference: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (pin {ORACLE_PIN:.0e})")
    assert got["low_res_logits"].dtype == torch.float32
    assert max(errs.values()) <= ORACLE_PIN, errs
    assert argmax_disagreement(got["logits"], gold["argmax"], gold["logits"], MARGIN)[1] == 0


def test_restatement_takes_float64_and_the_fp32_reference_is_its_rounding():
    name = "ow_d64"
    case = OW_CASES[name]
    gold, _ = load_golden(f"oneway_{name}")
    batch = R.to_dtype(make_episode(**case["episode"]), torch.float64)
    w = R.to_dtype(init_state_dict(case["cfg"], case["weight_seed"]), torch.float64)
    with torch.no_grad():
        got = R.lam_forward(w, geometry_for(case["cfg"]), batch, gold["selected_rows"])
    assert got["low_res_logits"].dtype == torch.float64
    assert rel_err(got["low_res_logits"], gold["low_res_logits"]) <= 2e-5


def test_the_one_way_decoder_is_not_the_two_way_one(restated):
    from oracle import lam_oracle as O
    got, gold, _, batch = restated["ow_d64"]
    case = OW_CASES["ow_d64"]
    two = dataclasses.replace(case["cfg"], fusion_transformer="TwoWayTransformer")
    st = {}
    with torch.no_grad():
        O.lam_forward(init_state_dict(two, case["weight_seed"]), geometry_for(two), batch, gold["selected_rows"], stages=st)
    assert rel_err(st["class_embeddings"], got["class_embeddings"]) <= 1e-6          # same prompt encoder, same weights ahead of the decoder
    assert rel_err(st["low_res_logits"], got["low_res_logits"]) > 1e-2


def test_the_cases_cover_what_they_are_there_for():
    ep = {n: make_episode(**c["episode"]) for n, c in OW_CASES.items()}
    assert OW_CASES["ow_d256"]["cfg"].embed_dim == 256 and OW_CASES["ow_d256"]["cfg"].grid == 16 and ep["ow_d256"]["flag_examples"].shape[2] == 3
    assert OW_CASES["ow_d64"]["cfg"].embed_dim == 64 and OW_CASES["ow_d64"]["cfg"].lam_neck and ep["ow_d64"]["flag_examples"].shape[0] == 2
    masks = OW_CASES["ow_masks"]
    assert masks["episode"]["prompts"] == ("mask",) and masks["cfg"].class_encoder is None and not masks["cfg"].example_class_attention
    for n in OW_CASES:
        _, meta = load_golden(f"oneway_{n}")
        assert 0 <= meta["margin_band_share"] <= MAX_BAND_SHARE and meta["margin"] == MARGIN
        assert os.path.getsize(os.path.join(GOLDEN, f"oneway_{n}.safetensors")) < 1 << 20


def test_stored_training_step_leaves_norm3_dead():
    name = OW_TRAIN["case"]
    gold = load_file(os.path.join(GOLDEN, f"oneway_{name}_train.safetensors"))
    with open(os.path.join(GOLDEN, f"oneway_{name}_train.json")) as fh:
        meta = json.load(fh)
    assert sorted(k for k in meta["dead"] if k.startswith(TR)) == sorted(p + n for p in NORM3 for n in ("weight", "bias"))
    assert not any(k.startswith(NORM3) for k in meta["keys"])
    assert sorted("grad." + k for k in OW_TRAIN_FULL) == sorted(k for k in gold if k.startswith("grad."))
    assert "grad." + TR + "layers.1.mlp.lin1.weight" in gold and "grad." + TR + "layers.0.cross_attn_image_to_token.k_proj.weight" in gold
    assert all(float(gold["grad." + k].abs().max()) > 0 for k in OW_TRAIN_FULL)
    assert meta["relu_min_gap"] >= KINK_BAND and meta["weight_seed"] == OW_CASES[name]["weight_seed"]      # no ReLU sits on its kink
    assert 0 < meta["e_ref32"] < 3e-4 and abs(meta["loss"] - meta["loss_fp64"]) <= 2e-5 * abs(meta["loss_fp64"])
    shapes = model_shapes(OW_CASES[name]["cfg"])
    assert sorted(meta["keys"] + meta["dead"]) == sorted(k for k in shapes if not k.endswith("positional_encoding_gaussian_matrix"))
    assert os.path.getsize(os.path.join(GOLDEN, f"oneway_{name}_train.safetensors")) < 1 << 20


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_and_declared():
    with open(os.path.join(ROOT, "include", "la_hip.h")) as fh:
        header = fh.read()
    for sym in ("la_stream_mlp", "la_stream_mlp_ok"):
        assert sym in _lib.EXPORTS and re.search(rf"\bint {sym}\(", header)
    assert "transformer.py:149-152" in header and "common.py:19-37" in header
    assert callable(_lib.stream_mlp) and callable(_lib.stream_mlp_ok)
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"C ABI ({len(_lib.EXPORTS) + 2} entry points" in fh.read()          # + la_last_error, la_version
