"""CPU: configuration surface and weights of the two-level classification head (``classification_levels=2``) and the torch restatement of
its two steps (tests/levels_ref.py) against the reference's fixtures (tests/golden/levels_*, tools/make_golden_levels.py)."""
import dataclasses
import json
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

from labelanything_amd.config import LamConfig, config_from_kwargs
from labelanything_amd.weights import decoder_shapes, init_state_dict, model_shapes
from tests import levels_ref as R
from tests.cases_levels import LV_CASES, LV_TRAIN, LV_TRAIN_FULL
from tests.helpers import load_golden

SMALL = dict(image_size=64, embed_dim=64, image_embed_dim=64)
NEW_KEYS = ["mask_decoder.level_reducer.weight", "mask_decoder.level_reducer.bias"]


def test_switch_is_accepted():
    assert LamConfig().classification_levels == 1
    assert config_from_kwargs(encoder=None, use_vit=False, **SMALL).classification_levels == 1
    assert config_from_kwargs(encoder=None, use_vit=False, classification_levels=1, **SMALL).classification_levels == 1
    assert config_from_kwargs(encoder=None, use_vit=False, classification_levels=2, **SMALL).classification_levels == 2


@pytest.mark.parametrize("value", [0, 3, -1, 2.5, "2", None, True])
def test_other_values_are_refused(value):
    """mask_decoder.py:360 stacks exactly two levels: nothing but 1 and 2 can run in the reference."""
    with pytest.raises(ValueError, match="classification_levels"):
        config_from_kwargs(encoder=None, use_vit=False, classification_levels=value, **SMALL)


@pytest.mark.parametrize("kw", [dict(embeddings_per_example=4), dict(segment_example_logits=True),
                                dict(segment_example_logits=True, embeddings_per_example=9)])
def test_combination_with_the_per_example_family_is_refused(kw):
    from labelanything_amd.models import Lam
    with pytest.raises(NotImplementedError, match="mae_chooser"):
        config_from_kwargs(encoder=None, use_vit=False, classification_levels=2, **SMALL, **kw)
    base = config_from_kwargs(encoder=None, use_vit=False, classification_levels=2, **SMALL)
    with pytest.raises(NotImplementedError, match="mae_chooser"):
        Lam(base, **kw)


def test_public_constructors():
    from labelanything_amd.models import LabelAnything, Lam, build_lam, build_lam_no_vit
    m = LabelAnything(encoder=None, use_vit=False, classification_levels=2, **SMALL)
    assert m.model.cfg.classification_levels == 2 and m.config["classification_levels"] == 2
    assert LabelAnything(encoder=None, use_vit=False, **SMALL).model.cfg.classification_levels == 1
    assert build_lam_no_vit(classification_levels=2, **SMALL).cfg.classification_levels == 2
    assert build_lam(encoder=None, use_vit=False, classification_levels=2, **SMALL).cfg.classification_levels == 2
    base = config_from_kwargs(encoder=None, use_vit=False, **SMALL)
    lam = Lam(base, classification_levels=2)
    assert lam.cfg.classification_levels == 2 and base.classification_levels == 1
    assert Lam(base).cfg == base
    for bad in (3, True, 1.0, 2.0, "2"):                                # the same check as config_from_kwargs
        with pytest.raises(ValueError, match="classification_levels"):
            Lam(base, classification_levels=bad)
    with pytest.raises(ValueError, match="classification_levels"):
        build_lam_no_vit(classification_levels=3, **SMALL)
    # the re-exported surface of the reference's package name, and its builder registry
    from label_anything.models import build_lam_no_vit as shim, model_registry
    assert shim(classification_levels=2, **SMALL).cfg.classification_levels == 2
    assert model_registry["lam_no_vit"](classification_levels=2, **SMALL).cfg.classification_levels == 2


def test_exactly_two_tensors_are_added_and_they_come_last():
    for case in LV_CASES.values():
        cfg = case["cfg"]
        plain = dataclasses.replace(cfg, classification_levels=1)
        s2, s1 = model_shapes(cfg), model_shapes(plain)
        assert list(s2)[:-2] == list(s1) and list(s2)[-2:] == NEW_KEYS
        assert s2[NEW_KEYS[0]] == (1, 2, 3, 3) and s2[NEW_KEYS[1]] == (1,)
        assert list(decoder_shapes(cfg))[-2:] == NEW_KEYS
        assert all(s2[k] == s1[k] for k in s1)


def test_common_tensors_are_bit_equal_to_the_one_level_model():
    for case in LV_CASES.values():
        cfg = case["cfg"]
        a = init_state_dict(cfg, case["weight_seed"])
        b = init_state_dict(dataclasses.replace(cfg, classification_levels=1), case["weight_seed"])
        assert list(a)[:-2] == list(b) and all(torch.equal(a[k], b[k]) for k in b)
        w = a[NEW_KEYS[0]]
        assert 0.1 < float(w.abs().mean()) < 0.6 and float(w.abs().max()) < 1.5          # of order 0.3


def test_state_dict_is_strict():
    from labelanything_amd.models import Lam
    cfg2 = config_from_kwargs(encoder=None, use_vit=False, classification_levels=2, **SMALL)
    cfg1 = config_from_kwargs(encoder=None, use_vit=False, **SMALL)
    two, one = Lam(cfg2, seed=3), Lam(cfg1, seed=3)
    sd2 = two.state_dict()
    assert list(sd2)[-2:] == NEW_KEYS and list(sd2)[:-2] == list(one.state_dict())
    assert {k for k, _ in two.named_parameters()} >= set(NEW_KEYS)
    other = Lam(cfg2, seed=4)
    other.load_state_dict(sd2)
    assert all(torch.equal(v, sd2[k]) for k, v in other.state_dict().items())
    with pytest.raises(RuntimeError, match="level_reducer"):
        one.load_state_dict(sd2)                                     # unexpected keys
    with pytest.raises(RuntimeError, match="level_reducer"):
        two.load_state_dict(one.state_dict())                        # missing keys


def test_hub_round_trip():
    from labelanything_amd.models import LabelAnything, build_lam
    m = LabelAnything(encoder=None, use_vit=False, classification_levels=2, **SMALL)
    with torch.no_grad():
        m.model.mask_decoder.level_reducer.weight.copy_(torch.arange(18.0).view(1, 2, 3, 3) / 7)
        m.model.mask_decoder.level_reducer.bias.fill_(-0.375)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    assert "model.mask_decoder.level_reducer.weight" in want
    with tempfile.TemporaryDirectory() as d:
        m.save_local(d)
        with open(os.path.join(d, "config.json")) as fh:
            assert json.load(fh)["classification_levels"] == 2
        m2 = LabelAnything.from_local(d)
        assert m2.model.cfg == m.model.cfg and m2.config == m.config
        assert all(torch.equal(v, want[k]) for k, v in m2.state_dict().items()) and list(m2.state_dict()) == list(want)
    with tempfile.TemporaryDirectory() as d:
        m.save_pretrained(d)
        m3 = LabelAnything.from_pretrained(d)
        assert m3.model.cfg.classification_levels == 2
        assert all(torch.equal(v, want[k]) for k, v in m3.state_dict().items()) and list(m3.state_dict()) == list(want)
    kw = dict(encoder=None, use_vit=False, classification_levels=2, **SMALL)
    lam = build_lam(**json.loads(json.dumps(kw)))
    assert config_from_kwargs(**json.loads(json.dumps(dataclasses.asdict(lam.cfg)))) == lam.cfg


# ---- the torch restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (5, 7), (16, 16)])
def test_enlarge4_is_torch_bilinear(h, w):
    x = torch.randn(2, 3, h, w, dtype=torch.float64, generator=torch.Generator().manual_seed(h * 31 + w))
    want = F.interpolate(x, size=(4 * h, 4 * w), mode="bilinear", align_corners=False)
    assert float((R.enlarge4(x) - want).abs().max()) <= 1e-14


def test_phase_weights_are_eighths():
    ramp = torch.arange(4, dtype=torch.float64).view(1, 1, 1, 4)
    got = R.enlarge4(ramp.expand(1, 1, 1, 4))[0, 0, 0]
    want = torch.tensor([0, 0, 1 / 8, 3 / 8, 5 / 8, 7 / 8, 9 / 8, 11 / 8, 13 / 8, 15 / 8, 17 / 8, 19 / 8, 21 / 8, 23 / 8, 3, 3], dtype=torch.float64)
    assert torch.equal(got, want)


@pytest.mark.parametrize("name", list(LV_CASES))
def test_restatement_reproduces_the_fixtures(name):
    """fp32 restatement on the fixture's operands (tokens, image stream, fine logits, the case's level_reducer) against the reference's
    low_res_logits: 2e-6 of the logit scale (max-norm), the project's oracle pin."""
    case = LV_CASES[name]
    gold, meta = load_golden(f"levels_{name}")
    sd = init_state_dict(case["cfg"], case["weight_seed"])
    w, bias = sd[NEW_KEYS[0]], sd[NEW_KEYS[1]]
    g = meta["grid"]
    b, c, _ = gold["tokens"].shape
    assert gold["tokens"].dtype == torch.float32
    cls1 = R.coarse_classify(gold["tokens"], gold["image_rows"]).view(b, c, g, g)
    e1 = float((cls1 - gold["cls1"]).abs().max() / gold["cls1"].abs().max())
    seg = R.level_reduce(gold["cls0"], cls1, w, bias)
    want = gold["low_res_logits"]
    assert seg.dtype == torch.float32 and seg.shape == want.shape
    err = float((seg - want).abs().max() / want.abs().max())
    err64 = float((R.level_reduce(gold["cls0"].double(), R.coarse_classify(gold["tokens"].double(), gold["image_rows"].double())
                                  .view(b, c, g, g), w.double(), bias.double()) - want.double()).abs().max() / want.abs().max())
    print(f"{name}: restated cls1 rel err {e1:.3e}, low_res_logits rel err fp32 {err:.3e} fp64 {err64:.3e}")
    assert e1 <= 2e-6 and err <= 2e-6


def test_training_fixture_holds_the_new_gradients():
    """The weight's gradient carries signal.  The bias is inert under the step's softmax objective (it shifts every class alike): the
    reference's fp32 value is rounding noise, below what summing the stored number of terms can leave, and it is not part of e_kink."""
    gold, meta = load_golden(f"levels_{LV_TRAIN['case']}_train")
    assert NEW_KEYS[0] in meta["keys"] and meta["inert"] == [NEW_KEYS[1]] and NEW_KEYS[1] not in meta["keys"]
    assert set(NEW_KEYS) <= set(LV_TRAIN_FULL)
    for k in LV_TRAIN_FULL:
        assert "grad." + k in gold
    assert float(gold["grad." + NEW_KEYS[0]].abs().min()) > 0
    assert tuple(gold["grad." + NEW_KEYS[0]].shape) == (1, 2, 3, 3)
    noise = (meta["dseg_numel"] + 2) * 2.0 ** -24 * meta["dseg_abs_sum"]
    assert float(gold["grad." + NEW_KEYS[1]].abs().max()) == meta["inert_reference_fp32"] <= noise
    assert meta["inert_reference_fp64"] <= 1e-12 * float(gold["grad." + NEW_KEYS[0]].abs().max())
    assert meta["e_kink_worst_tensor"] != NEW_KEYS[1] and 0 < meta["e_kink"] < 1e-2
