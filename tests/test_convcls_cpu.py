"""CPU: configuration surface and weights of ``conv_classification`` / ``classification_layer_downsample_rate`` and the torch restatement
of the two steps (tests/convcls_ref.py) against torch's own operators and the reference's fixtures (tests/golden/convcls_*, nodown_r1;
tools/make_golden_convcls.py)."""
import dataclasses
import json
import os
import re
import tempfile

import pytest
import torch
import torch.nn.functional as F

from labelanything_amd import _lib
from labelanything_amd.config import LamConfig, config_from_kwargs
from labelanything_amd.weights import decoder_shapes, init_state_dict, model_shapes
from tests import convcls_ref as R
from tests.cases_convcls import CC_CASES, CC_TCONV, CC_TCONV_ROWS, CC_TRAIN, CC_TRAIN_FULL
from safetensors.torch import load_file
from tests.helpers import GOLDEN, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(image_size=64, embed_dim=64, image_embed_dim=64)
NEW_KEYS = CC_TCONV
NEW_EXPORTS = ["la_proto_kernels", "la_proto_kernels_bwd", "la_classify_conv", "la_classify_conv_bwd"]


def cfg_of(**kw):
    return config_from_kwargs(encoder=None, use_vit=False, **SMALL, **kw)


# ---- the validator --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [1, 8])
@pytest.mark.parametrize("conv", [True, False])
def test_the_four_built_combinations_are_accepted(rate, conv):
    cfg = cfg_of(classification_layer_downsample_rate=rate, conv_classification=conv)
    assert cfg.classification_layer_downsample_rate == rate and cfg.conv_classification is conv
    assert (cfg.up_mid, cfg.class_width) == ((64, 64) if rate == 1 else (16, 8))


def test_defaults():
    assert LamConfig().classification_layer_downsample_rate == 8 and LamConfig().conv_classification is False
    assert cfg_of() == cfg_of(classification_layer_downsample_rate=8, conv_classification=False)


@pytest.mark.parametrize("rate", [3, 0, 16, True])
def test_rates_that_are_no_power_of_two_up_to_8_are_a_value_error(rate):
    with pytest.raises(ValueError, match="classification_layer_downsample_rate"):
        cfg_of(classification_layer_downsample_rate=rate)


@pytest.mark.parametrize("rate", [2, 4])
def test_rates_2_and_4_are_not_built(rate):
    with pytest.raises(NotImplementedError, match="classification_layer_downsample_rate"):
        cfg_of(classification_layer_downsample_rate=rate)


@pytest.mark.parametrize("kw", [dict(embeddings_per_example=4), dict(segment_example_logits=True)])
def test_combination_with_the_per_example_family_is_refused(kw):
    from labelanything_amd.models import Lam
    with pytest.raises(NotImplementedError, match="conv_classification"):
        cfg_of(conv_classification=True, **kw)
    with pytest.raises(NotImplementedError, match="conv_classification"):
        Lam(cfg_of(conv_classification=True), **kw)
    with pytest.raises(NotImplementedError, match="classification_layer_downsample_rate"):   # la_classify_max stops at 64 channels
        cfg_of(classification_layer_downsample_rate=1, **kw)
    with pytest.raises(NotImplementedError, match="classification_layer_downsample_rate"):
        Lam(cfg_of(classification_layer_downsample_rate=1), **kw)


@pytest.mark.parametrize("kw", [dict(conv_classification=True), dict(classification_layer_downsample_rate=1)])
def test_combination_with_two_levels_is_refused(kw):
    from labelanything_amd.models import Lam
    with pytest.raises(NotImplementedError, match="classification_levels"):
        cfg_of(classification_levels=2, **kw)
    with pytest.raises(NotImplementedError, match="classification_levels"):
        Lam(cfg_of(classification_levels=2), **kw)


def test_public_constructors():
    from labelanything_amd.models import LabelAnything, Lam, build_lam, build_lam_no_vit
    kw = dict(classification_layer_downsample_rate=1, conv_classification=True)
    m = LabelAnything(encoder=None, use_vit=False, **kw, **SMALL)
    assert m.model.cfg.conv_classification and m.model.cfg.classification_layer_downsample_rate == 1
    assert m.config["conv_classification"] is True and m.config["classification_layer_downsample_rate"] == 1
    assert not LabelAnything(encoder=None, use_vit=False, **SMALL).model.cfg.conv_classification
    assert build_lam_no_vit(**kw, **SMALL).cfg.class_width == 64
    assert build_lam(encoder=None, use_vit=False, **kw, **SMALL).cfg.conv_classification
    base = cfg_of()
    lam = Lam(base, **kw)
    assert lam.cfg.conv_classification and lam.cfg.class_width == 64 and not base.conv_classification
    assert Lam(base).cfg == base
    for bad in (3, True, 16):
        with pytest.raises(ValueError, match="classification_layer_downsample_rate"):
            Lam(base, classification_layer_downsample_rate=bad)
    with pytest.raises(NotImplementedError):
        Lam(base, classification_layer_downsample_rate=4)
    from label_anything.models import build_lam_no_vit as shim, model_registry
    assert shim(**kw, **SMALL).cfg.conv_classification
    assert model_registry["lam_no_vit"](**kw, **SMALL).cfg.class_width == 64


# ---- shapes and weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC_CASES))
def test_shapes_are_the_reference_s(name):
    _, meta = load_golden(name)
    ours = model_shapes(CC_CASES[name]["cfg"])
    ref = meta["reference_shapes"]
    assert sorted(ours) == sorted(ref)
    assert {k: list(v) for k, v in ours.items()} == ref
    if name == "convcls_r1":
        assert ours["mask_decoder.output_upscaling.0.weight"] == (256, 256, 2, 2) and ours["mask_decoder.output_upscaling.3.weight"] == (256, 256, 2, 2)
        assert ours["mask_decoder.class_mlp.layers.2.weight"] == (256, 256) and ours["mask_decoder.spatial_convs.6.weight"] == (256, 256, 3, 3)
        assert ours[NEW_KEYS[0]] == ours[NEW_KEYS[1]] == (256, 256, 3, 3)


def test_the_two_tensors_come_last_and_the_default_model_is_unchanged():
    base = CC_CASES["convcls_r8"]["cfg"]
    plain = dataclasses.replace(base, conv_classification=False)
    s2, s1 = model_shapes(base), model_shapes(plain)
    assert list(s2)[:-2] == list(s1) and list(s2)[-2:] == NEW_KEYS and list(decoder_shapes(base))[-2:] == NEW_KEYS
    a, b = init_state_dict(base, 13), init_state_dict(plain, 13)
    assert list(a)[:-2] == list(b) and all(torch.equal(a[k], b[k]) for k in b)
    # the default configuration: the key list, the shapes and the seeded values of a config that never heard of the two fields
    fields = {f.name: getattr(plain, f.name) for f in dataclasses.fields(plain)
              if f.name not in ("classification_layer_downsample_rate", "conv_classification")}
    again = LamConfig(**fields)
    assert again == plain and model_shapes(again) == s1
    d = again.embed_dim
    assert s1["mask_decoder.output_upscaling.0.weight"] == (d, d // 4, 2, 2) and s1["mask_decoder.output_upscaling.3.weight"] == (d // 4, d // 8, 2, 2)
    assert s1["mask_decoder.class_mlp.layers.2.weight"] == (d // 8, d) and s1["mask_decoder.spatial_convs.0.weight"] == (d // 8, d // 8, 3, 3)
    c = init_state_dict(again, 13)
    assert list(c) == list(b) and all(torch.equal(c[k], b[k]) for k in b)


def test_initialisation_scale_is_the_one_the_fixture_records():
    _, meta = load_golden("convcls_r1")
    sd = init_state_dict(CC_CASES["convcls_r1"]["cfg"], 13)
    init = meta["prototype_tconv_init"]
    assert init["fan"] == 9 * 256 and abs(init["std"] - (9 * 256) ** -0.5) < 1e-12
    for k in NEW_KEYS:
        assert abs(float(sd[k].std()) / init["std"] - 1) < 0.01
    assert 1.0 <= meta["scale"]["low_res_logits_rms"] <= 10.0 and meta["scale"]["low_res_logits"] < 40.0


def test_state_dict_is_strict():
    from labelanything_amd.models import Lam
    on, off = Lam(cfg_of(conv_classification=True), seed=3), Lam(cfg_of(), seed=3)
    sd = on.state_dict()
    assert list(sd)[-2:] == NEW_KEYS and list(sd)[:-2] == list(off.state_dict())
    assert {k for k, _ in on.named_parameters()} >= set(NEW_KEYS)
    other = Lam(cfg_of(conv_classification=True), seed=4)
    other.load_state_dict(sd)
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())
    with pytest.raises(RuntimeError, match="prototype_tconv"):
        off.load_state_dict(sd)                                      # unexpected keys
    with pytest.raises(RuntimeError, match="prototype_tconv"):
        on.load_state_dict(off.state_dict())                         # missing keys
    with pytest.raises(RuntimeError, match="size mismatch"):
        Lam(cfg_of(classification_layer_downsample_rate=1), seed=1).load_state_dict(off.state_dict())


def test_hub_round_trip():
    from labelanything_amd.models import LabelAnything, build_lam
    kw = dict(encoder=None, use_vit=False, classification_layer_downsample_rate=1, conv_classification=True, **SMALL)
    m = LabelAnything(**kw)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    assert "model.mask_decoder.prototype_tconv.1.weight" in want
    with tempfile.TemporaryDirectory() as d:
        m.save_local(d)
        with open(os.path.join(d, "config.json")) as fh:
            saved = json.load(fh)
        assert saved["conv_classification"] is True and saved["classification_layer_downsample_rate"] == 1
        m2 = LabelAnything.from_local(d)
        assert m2.model.cfg == m.model.cfg and m2.config == m.config
        assert all(torch.equal(v, want[k]) for k, v in m2.state_dict().items()) and list(m2.state_dict()) == list(want)
    lam = build_lam(**json.loads(json.dumps(kw)))
    assert config_from_kwargs(**json.loads(json.dumps(dataclasses.asdict(lam.cfg)))) == lam.cfg


# ---- the torch restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_is_conv_transpose_and_conv2d():
    g = torch.Generator().manual_seed(5)
    cf, b, c, h, w = 8, 2, 3, 7, 4
    e = torch.randn(b, c, cf, dtype=torch.float64, generator=g)
    w1, w2 = (torch.randn(cf, cf, 3, 3, dtype=torch.float64, generator=g) for _ in range(2))
    feat = torch.randn(b, cf, h, w, dtype=torch.float64, generator=g)
    k = R.compose_kernels(e.reshape(b * c, cf), w1, w2)
    want_k = F.conv_transpose2d(F.conv_transpose2d(e.reshape(b * c, cf, 1, 1), w1), w2)
    assert float((k - want_k).abs().max()) <= 1e-14 * float(want_k.abs().max())
    assert torch.equal(R.from_tap_major(R.tap_major(k)), k)
    want = torch.cat([F.conv2d(feat[i:i + 1], want_k.view(b, c, cf, 5, 5)[i], padding=2) for i in range(b)])
    got = R.conv_classify(feat, e, w1, w2)
    assert got.shape == (b, c, h, w) and float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())


@pytest.mark.parametrize("name", [n for n, c in CC_CASES.items() if c["cfg"].conv_classification])
def test_restatement_reproduces_the_fixtures(name):
    """fp32 restatement on the fixture's stored feature rows and prototypes against the reference's low_res_logits, on the logit rows that
    the stored rows determine: 1e-6 of the logit scale (max-norm)."""
    case = CC_CASES[name]
    gold, meta = load_golden(name)
    ops = load_file(os.path.join(GOLDEN, name + "_feat.safetensors"))
    sd = init_state_dict(case["cfg"], case["weight_seed"])
    rows = meta["feature_rows"]
    feat = ops["feature_rows"].permute(0, 3, 1, 2).contiguous()            # (B, cf, rows, W)
    assert feat.dtype == torch.float32 and feat.shape[1] == meta["class_width"] and feat.shape[2] == rows
    want = gold["low_res_logits"]
    full = rows == want.shape[2]
    valid = rows if full else rows - 2
    assert valid >= 10
    if not full:                          # rows below the stored ones are missing, not zero: only rows 0 .. rows - 3 are determined
        feat = F.pad(feat, (0, 0, 0, 2))
    seg = R.conv_classify(feat, ops["prototypes"], sd[NEW_KEYS[0]], sd[NEW_KEYS[1]])[:, :, :valid]
    assert seg.dtype == torch.float32
    err = float((seg - want[:, :, :valid]).abs().max() / want.abs().max())
    print(f"{name}: restated low_res_logits rel err {err:.3e} on {valid} rows")
    assert err <= 1e-6


def test_training_fixture_holds_the_new_gradients():
    gold, meta = load_golden(f"{CC_TRAIN['case']}_train")
    assert set(NEW_KEYS) <= set(meta["keys"]) and meta["sliced"] == {k: CC_TCONV_ROWS for k in NEW_KEYS}
    for k in CC_TRAIN_FULL + NEW_KEYS:
        assert "grad." + k in gold
    assert "mask_decoder.class_mlp.layers.2.weight" in CC_TRAIN_FULL
    for k in NEW_KEYS:
        assert tuple(gold["grad." + k].shape) == (CC_TCONV_ROWS, 256, 3, 3) and float(gold["grad." + k].abs().max()) > 0
    assert len(gold["grad_norm"]) == len(meta["keys"]) and 0 < meta["e_kink"] < 1e-2


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_and_declared():
    with open(os.path.join(ROOT, "include", "la_hip.h")) as fh:
        header = fh.read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(rf"\bint {name}\(", header), name
    assert "mask_decoder.py:257-271" in header and "mask_decoder.py:305-307" in header
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert f"C ABI ({len(_lib.EXPORTS) + 2} entry points" in fh.read()          # + la_last_error, la_version
