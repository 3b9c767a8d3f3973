"""CPU: configuration surface and weights of ``embedding_extraction="cross_attention"`` and the two torch restatements of the extraction
(tests/cross_extract_ref.py: literal and folded) against the reference's fixtures (tests/golden/cross_extract_*;
tools/make_golden_cross_extract.py)."""
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
from labelanything_amd.weights import decoder_shapes, init_state_dict, model_shapes
from tests import cross_extract_ref as R
from tests.cases_cross_extract import XE_CASES
from tests.helpers import GOLDEN, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(image_size=64, embed_dim=64, image_embed_dim=64)
XA = dict(embedding_extraction="cross_attention")
PRE = "prompt_encoder.embedding_extraction."
NEW_EXPORTS = ["la_extract_pool_plan", "la_extract_pool", "la_extract_fold", "la_extract_unfold"]
ORACLE_PIN = 2e-6                         # the project's pin of a torch restatement against the reference's fp32 (max-norm)


def cfg_of(**kw):
    return config_from_kwargs(encoder=None, use_vit=False, **SMALL, **kw)


def stream_of(name):
    case = XE_CASES[name]
    gold, meta = load_golden(f"cross_extract_{name}")
    ops = load_file(os.path.join(GOLDEN, f"cross_extract_{name}_stream.safetensors"))
    b, m, c = ops["flag_examples_in"].shape
    return case, gold, meta, ops, (b, m, c), init_state_dict(case["cfg"], case["weight_seed"])


# ---- the validator --------------------------------------------------------------------------------------------------------------------
def test_accepted_values_and_defaults():
    assert LamConfig().embedding_extraction is None and cfg_of().embedding_extraction is None
    assert cfg_of(embedding_extraction=None) == cfg_of()
    c4 = cfg_of(embeddings_per_example=4, **XA)
    assert c4.embedding_extraction == "cross_attention" and c4.segment_example_logits and c4.embeddings_per_example == 4
    assert c4.pool_side == 1                                        # the learned queries replace the pooling
    c1 = cfg_of(segment_example_logits=True, **XA)                  # the flag alone resolves to one query, as for the family
    assert c1.embeddings_per_example == 1 and c1.segment_example_logits


def test_five_queries_are_allowed_and_the_pool_check_does_not_apply():
    c5 = cfg_of(embeddings_per_example=5, **XA)
    assert c5.embeddings_per_example == 5 and c5.pool_side == 1
    # 16 queries on a 2 x 2 grid: the pooled family would refuse (4 x 4 bins from a 2 x 2 grid), the learned queries do not pool
    tiny = dict(image_size=32, embed_dim=64, image_embed_dim=64)
    with pytest.raises(ValueError, match="embeddings_per_example"):
        config_from_kwargs(encoder=None, use_vit=False, embeddings_per_example=16, **tiny)
    assert config_from_kwargs(encoder=None, use_vit=False, embeddings_per_example=16, **tiny, **XA).embeddings_per_example == 16


def test_without_a_number_of_queries_it_is_a_value_error():
    with pytest.raises(ValueError, match="embeddings_per_example"):
        cfg_of(**XA)
    with pytest.raises(ValueError, match="embeddings_per_example"):
        cfg_of(embeddings_per_example=0, **XA)
    from labelanything_amd.models import Lam
    with pytest.raises(ValueError, match="embeddings_per_example"):
        Lam(cfg_of(), segment_example_logits=False, embeddings_per_example=0, **XA)


@pytest.mark.parametrize("value", ["pooler", "GuidedPooler", "Cross_Attention", "", 1])
def test_every_other_value_is_not_built(value):
    from labelanything_amd.models import Lam
    with pytest.raises(NotImplementedError, match="embedding_extraction"):
        cfg_of(embeddings_per_example=4, embedding_extraction=value)
    with pytest.raises(NotImplementedError, match="embedding_extraction"):
        Lam(cfg_of(embeddings_per_example=4), embedding_extraction=value)


@pytest.mark.parametrize("kw,match", [(dict(classification_levels=2), "classification_levels"), (dict(conv_classification=True), "conv_classification"),
                                      (dict(classification_layer_downsample_rate=1), "classification_layer_downsample_rate")])
def test_refusals_of_the_per_example_family_stay(kw, match):
    with pytest.raises(NotImplementedError, match=match):
        cfg_of(embeddings_per_example=4, **XA, **kw)
    with pytest.raises(NotImplementedError, match=match):
        cfg_of(segment_example_logits=True, **XA, **kw)


def test_sizes_the_kernel_does_not_take_are_refused():
    with pytest.raises(NotImplementedError, match="16"):
        cfg_of(embeddings_per_example=17, **XA)
    with pytest.raises(NotImplementedError, match="embed_dim"):
        config_from_kwargs(encoder=None, use_vit=False, image_size=64, embed_dim=512, image_embed_dim=512, embeddings_per_example=4, **XA)


def test_public_constructors():
    from labelanything_amd.models import LabelAnything, Lam, build_lam, build_lam_no_vit
    kw = dict(embeddings_per_example=4, **XA)
    assert build_lam_no_vit(**kw, **SMALL).cfg.embedding_extraction == "cross_attention"
    assert build_lam(encoder=None, use_vit=False, **kw, **SMALL).cfg.embeddings_per_example == 4
    base = cfg_of()
    lam = Lam(base, **kw)
    assert lam.cfg.embedding_extraction == "cross_attention" and lam.cfg.embeddings_per_example == 4 and base.embedding_extraction is None
    assert Lam(base).cfg == base
    assert Lam(base, segment_example_logits=True, **XA).cfg.embeddings_per_example == 1
    m = LabelAnything(encoder=None, use_vit=False, segment_example_logits=True, **XA, **SMALL)
    assert m.model.cfg.embedding_extraction == "cross_attention" and m.config["embedding_extraction"] == "cross_attention"
    assert LabelAnything(encoder=None, use_vit=False, **SMALL).model.cfg.embedding_extraction is None
    from label_anything.models import build_lam_no_vit as shim, model_registry
    assert shim(**kw, **SMALL).cfg.embedding_extraction == "cross_attention"
    assert model_registry["lam_no_vit"](**kw, **SMALL).cfg.embeddings_per_example == 4
    # the constructor call of the recipe (parameters/validation/Pascal/mae_cross.yaml)
    full = build_lam_no_vit(image_size=480, image_embed_dim=768, embed_dim=256, spatial_convs=3, embeddings_per_example=4,
                            embedding_extraction="cross_attention", class_attention=False, example_attention=False, example_class_attention=False)
    assert full.cfg.grid == 30 and sum(k.startswith(PRE) for k in full.state_dict()) == 37


# ---- shapes and weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(XE_CASES))
def test_key_names_and_shapes_are_the_fixture_s(name):
    _, meta = load_golden(f"cross_extract_{name}")
    cfg = XE_CASES[name]["cfg"]
    ours = decoder_shapes(cfg)
    added = [k for k in ours if k.startswith(PRE)]
    assert len(added) == 37 and added == meta["added_keys"]
    assert {k: list(ours[k]) for k in added} == meta["added_shapes"]
    d, n = cfg.embed_dim, cfg.embeddings_per_example
    assert ours[PRE + "embeddings.weight"] == (n, d)
    for l in range(2):
        ca = f"{PRE}layers.{l}.cross_attn_image_to_token."
        assert ours[ca + "q_proj.weight"] == ours[ca + "k_proj.weight"] == ours[ca + "v_proj.weight"] == (d // 2, d)
        assert ours[ca + "out_proj.weight"] == (d, d // 2) and ours[f"{PRE}layers.{l}.mlp.lin1.weight"] == (2048, d)
        assert ours[f"{PRE}layers.{l}.norm3.weight"] == (d,)          # held and saved, never applied


def test_added_tensors_come_last_and_the_others_are_the_plain_model_s():
    cfg = XE_CASES["x4"]["cfg"]
    plain = dataclasses.replace(cfg, embedding_extraction=None, segment_example_logits=False, embeddings_per_example=None)
    s2, s1 = model_shapes(cfg), model_shapes(plain)
    assert list(s2)[:-37] == list(s1) and all(k.startswith(PRE) for k in list(s2)[-37:])
    a, b = init_state_dict(cfg, 13), init_state_dict(plain, 13)
    assert list(a)[:-37] == list(b) and all(torch.equal(a[k], b[k]) for k in b)
    emb = a[PRE + "embeddings.weight"]
    assert abs(float(emb.std()) - 1.0) < 0.1 and abs(float(emb.mean())) < 0.1            # N(0, 1) per entry, like nn.Embedding
    w = a[PRE + "layers.0.cross_attn_image_to_token.q_proj.weight"]
    assert abs(float(w.std()) * 256 ** 0.5 - 1.0) < 0.05                                 # the fan-in rule
    assert abs(float(a[PRE + "layers.1.norm3.weight"].mean()) - 1.0) < 0.05              # the norm rule
    # the merge attentions keep their parameters for strict-load parity (they are not run)
    with_attn = dataclasses.replace(cfg, example_class_attention=True)
    assert any(k.startswith("prompt_encoder.class_example_attention.") for k in model_shapes(with_attn))


def test_state_dict_is_strict():
    from labelanything_amd.models import Lam
    on, off = Lam(cfg_of(embeddings_per_example=3, **XA), seed=3), Lam(cfg_of(embeddings_per_example=3), seed=3)
    sd = on.state_dict()
    assert sum(k.startswith(PRE) for k in sd) == 37 and {k for k, _ in on.named_parameters()} >= {k for k in sd if k.startswith(PRE)}
    other = Lam(cfg_of(embeddings_per_example=3, **XA), seed=4)
    other.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    with pytest.raises(RuntimeError, match="embedding_extraction"):
        off.load_state_dict(sd)
    with pytest.raises(RuntimeError, match="embedding_extraction"):
        on.load_state_dict(off.state_dict())
    with pytest.raises(RuntimeError, match="size mismatch"):
        Lam(cfg_of(embeddings_per_example=4, **XA), seed=1).load_state_dict(sd)


def test_config_json_round_trip():
    from labelanything_amd.models import LabelAnything, build_lam
    kw = dict(encoder=None, use_vit=False, segment_example_logits=True, **XA, **SMALL)
    m = LabelAnything(**kw)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    assert "model." + PRE + "embeddings.weight" in want
    with tempfile.TemporaryDirectory() as d:
        m.save_local(d)
        with open(os.path.join(d, "config.json")) as fh:
            assert json.load(fh)["embedding_extraction"] == "cross_attention"
        m2 = LabelAnything.from_local(d)
        assert m2.model.cfg == m.model.cfg and m2.config == m.config
        assert all(torch.equal(v, want[k]) for k, v in m2.state_dict().items()) and list(m2.state_dict()) == list(want)
    lam = build_lam(encoder=None, use_vit=False, embeddings_per_example=4, **XA, **SMALL)
    assert config_from_kwargs(**json.loads(json.dumps(dataclasses.asdict(lam.cfg)))) == lam.cfg


def test_trainer_refuses_the_configuration():
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    with pytest.raises(NotImplementedError, match="embedding_extraction"):
        LamTrainer(Lam(cfg_of(embeddings_per_example=4, **XA), seed=1))


# ---- the torch restatements -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["literal", "folded"])
@pytest.mark.parametrize("name", list(XE_CASES))
def test_restatement_reproduces_the_reference_module(name, form):
    """fp32 restatement on the fixture's stream rows against what the reference's module returned for exactly those rows."""
    case, gold, meta, ops, (b, m, c), sd = stream_of(name)
    got = R.extract(ops["stream"], b, m, c, sd, form)
    want = ops["sub_embeddings"]
    assert got.dtype == torch.float32 and got.shape == want.shape == (b, case["cfg"].embeddings_per_example, c, case["cfg"].embed_dim)
    err = float((got - want).abs().max() / want.abs().max())
    print(f"[{name}] {form} restatement vs the reference's module: rel err {err:.3e} (pin {ORACLE_PIN:.0e})")
    assert err <= ORACLE_PIN
    if meta["stream_stride"] == 1:                                    # the whole stream is stored: these are the model's embeddings
        assert torch.equal(want, gold["class_examples_embeddings"])


@pytest.mark.parametrize("name", list(XE_CASES))
def test_the_two_forms_agree_in_float64(name):
    case, gold, meta, ops, (b, m, c), sd = stream_of(name)
    x = ops["stream"].double()
    lit, fold = R.extract(x, b, m, c, sd, "literal"), R.extract(x, b, m, c, sd, "folded")
    err = float((lit - fold).abs().max())
    print(f"[{name}] literal vs folded in float64: {err:.3e} (scale {float(lit.abs().max()):.2f})")
    assert err <= 1e-13 * float(lit.abs().max())
    # and the fp32 module output is the fp32 rounding of that
    assert float((lit.float() - ops["sub_embeddings"]).abs().max() / ops["sub_embeddings"].abs().max()) <= ORACLE_PIN


@pytest.mark.parametrize("name", list(XE_CASES))
def test_the_key_mask_is_a_no_op(name):
    case, gold, meta, ops, (b, m, c), sd = stream_of(name)
    flags = ops["flag_examples_in"]
    assert meta["key_mask_is_a_no_op"] is True                       # measured on the reference: real flags vs all-ones flags, bit-identical
    if name != "x5_d64":
        assert int((flags == 0).sum()) > 0                            # the episode does have a padded support
    for form in ("literal", "folded"):
        assert torch.equal(R.extract(ops["stream"], b, m, c, sd, form, flag_examples=flags), R.extract(ops["stream"], b, m, c, sd, form))
    assert torch.equal(gold["flag_examples"], R.example_flags(flags, case["cfg"].embeddings_per_example))


@pytest.mark.parametrize("name", list(XE_CASES))
def test_fixture_condition_on_the_score_spread(name):
    _, meta = load_golden(f"cross_extract_{name}")
    assert meta["min_spread_required"] == XE_CASES[name]["min_spread"] and (name == "x5_d64" or meta["min_spread_required"] == 1.5)
    for layer in meta["score_spread"]:
        assert layer["min"] >= meta["min_spread_required"] and layer["max"] >= 5.0
        assert layer["rows"] == 8 * meta["queries"] * gold_pairs(name)


def gold_pairs(name):
    ops = load_file(os.path.join(GOLDEN, f"cross_extract_{name}_stream.safetensors"))
    b, _, c = ops["flag_examples_in"].shape
    return b * c


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_and_declared():
    with open(os.path.join(ROOT, "include", "la_hip.h")) as fh:
        header = fh.read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(rf"\bint {name}\(", header), name
    for cite in ("prompt_encoder.py:289-298", "transformer.py:140-147", "common.py:105-146", "common.py:120-124"):
        assert cite in header, cite
    with open(os.path.join(ROOT, "labelanything_amd", "csrc", "extract.hip")) as fh:
        src = fh.read()
    assert "NO KEY IS MASKED" in src and "common.py:120-124" in src
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"C ABI ({len(_lib.EXPORTS) + 2} entry points" in fh.read()          # + la_last_error, la_version
