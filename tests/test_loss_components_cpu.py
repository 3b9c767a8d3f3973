"""CPU: the device LabelAnythingLoss's construction and bookkeeping (reference loss/__init__.py) and the fp64 restatement
(tests/loss_components_ref.py) against the reference's own outputs (tests/golden/loss_components.safetensors and
train_loss_components.*, written by tools/make_golden_loss_components.py from the imported reference)."""
import json
import math
import os

import pytest
import torch
from safetensors.torch import load_file

from labelanything_amd.loss import LabelAnythingLoss
from tests import loss_components_ref as R
from tests.helpers import GOLDEN

# loss sections of parameters/trainval/other/*.yaml and the fine-tuning configs (weights only, class_weighting True)
CONFIGS = {
    "1_NewTraining": {"focal": {"weight": 0.725}, "dice": {"weight": 0.025}, "prompt_contrastive": {"weight": 0.25}},
    "2.5_NewTraining_NoDice": {"focal": {"weight": 0.75}, "prompt_contrastive": {"weight": 0.25}},
    "2.6_NewTraining_FP": {"focal": {"weight": 0.8}, "prompt_contrastive": {"weight": 0.1}, "fp": {"weight": 0.1}},
    "test_weed": {"focal": {"weight": 0.9}, "prompt_contrastive": {"weight": 0.1}},
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_constructs_from_the_reference_config_sections(name):
    comps = CONFIGS[name]
    crit = LabelAnythingLoss(comps, class_weighting=True)
    assert crit.weights == {k: v["weight"] for k, v in comps.items()}
    assert comps[next(iter(comps))]["weight"]                     # the caller's dicts are not consumed
    assert crit.logits_components == [k for k in comps if k != "prompt_contrastive"]
    keys = ["prompt_components.prompt_contrastive.t_prime", "prompt_components.prompt_contrastive.bias"]
    assert list(crit.state_dict()) == keys and [k for k, _ in crit.named_parameters()] == keys
    assert len(list(crit.parameters())) == 2
    sd = crit.state_dict()
    assert abs(float(sd[keys[0]]) - math.log(10.0)) < 1e-6 and float(sd[keys[1]]) == -10.0
    assert sd[keys[0]].shape == (1,) and sd[keys[1]].shape == (1,)
    crit.load_state_dict({keys[0]: torch.tensor([math.log(50.0)]), keys[1]: torch.tensor([-3.0])})
    assert abs(float(crit.prompt_components["prompt_contrastive"].t_prime) - math.log(50.0)) < 1e-6


def test_unknown_and_unbuilt_components_raise():
    with pytest.raises(ValueError, match="Unknown loss components"):
        LabelAnythingLoss({"focal": {"weight": 1.0}, "tversky": {"weight": 1.0}})
    for k in ("rmi", "emb_contrastive", "masks"):
        with pytest.raises(NotImplementedError, match=k):
            LabelAnythingLoss({"focal": {"weight": 1.0}, k: {"weight": 0.1}})
    with pytest.raises(NotImplementedError, match="average"):
        LabelAnythingLoss({"dice": {"weight": 1.0, "average": "micro"}})
    with pytest.raises(NotImplementedError, match="reduction"):
        LabelAnythingLoss({"dice": {"weight": 1.0, "reduction": "sum"}})
    with pytest.raises(KeyError):
        LabelAnythingLoss({"focal": {"gamma": 2.0}})
    assert LabelAnythingLoss({"focal": {"weight": 1.0, "gamma": 3.0}}).gamma == 3.0
    assert list(LabelAnythingLoss({"focal": {"weight": 1.0}, "fp": {"weight": 0.1}}).parameters()) == []


def test_weight_bookkeeping_of_the_fixtures():
    """A logits component adds w^2 L and reports w L; prompt_contrastive adds w L and reports L (loss/__init__.py:78,87,101)."""
    with open(os.path.join(GOLDEN, "loss_components.json")) as fh:
        meta = json.load(fh)
    for name, m in meta["cases"].items():
        total = 0.0
        for k, rep in m["reported"].items():
            w = m["components"][k]["weight"]
            total += w * rep          # logits: w^2 L = w * (w L); prompt: w L = w * L
        assert abs(total - m["value"]) <= 1e-6 * max(1.0, abs(m["value"])), name
    a = meta["cases"]["a"]["reported"]
    assert abs(0.725 * a["focal"] + 0.025 * a["dice"] + 0.25 * a["prompt_contrastive"] - meta["cases"]["a"]["value"]) < 1e-5


def test_restatement_matches_the_reference_fixtures():
    t = load_file(os.path.join(GOLDEN, "loss_components.safetensors"))
    with open(os.path.join(GOLDEN, "loss_components.json")) as fh:
        meta = json.load(fh)
    names = meta["component_order"]
    for name, m in meta["cases"].items():
        x = t[f"{name}.logits"].double().requires_grad_(True)
        e = t[f"{name}.emb"].double().requires_grad_(True)
        tp = t[f"{name}.t_prime"].double().requires_grad_(True)
        bs = t[f"{name}.bias"].double().requires_grad_(True)
        val, comps = R.objective(m["components"], m["class_weighting"], x, t[f"{name}.target"], e, t[f"{name}.flags"], tp, bs)
        val.backward()
        assert abs(float(val) - float(t[f"{name}.value"])) <= 2e-6 * max(1.0, abs(float(t[f"{name}.value"]))), name
        for k, v in comps.items():
            r = float(t[f"{name}.components"][names.index(k)])
            assert abs(float(v) - r) <= 2e-6 * max(1.0, abs(r)), (name, k)
        rg = t[f"{name}.grad_logits"]
        assert float((x.grad - rg).abs().max()) <= 1e-5 * float(rg.abs().max()), name
        if "prompt_contrastive" in comps:
            for mine, k in ((e.grad, "grad_emb"), (tp.grad, "grad_t_prime"), (bs.grad, "grad_bias")):
                assert float((mine - t[f"{name}.{k}"]).abs().max()) <= 1e-5 * max(1.0, float(t[f"{name}.{k}"].abs().max())), (name, k)


def test_quirks_pinned_by_the_fixtures():
    t = load_file(os.path.join(GOLDEN, "loss_components.safetensors"))
    # (e): the class plane at -inf gives a zero dice term and no NaN anywhere
    assert torch.isfinite(t["e.grad_logits"]).all() and float(t["e.value"]) == float(t["e.value"])
    x = t["e.logits"].double()
    assert float(R.dice(x[1:], t["e.target"][1:], torch.ones(4, dtype=torch.float64))) >= 0
    # (d): image 1 has no flagged row - it contributes nothing (the stored gradient there is zero)
    assert int(t["d.flags"][1].sum()) == 0 and float(t["d.grad_emb"][1].abs().max()) == 0.0
    # (b): background counts as present in the image with ignored pixels, so fp looks at classes absent after ignore -> 0
    tz = torch.where(t["b.target"][2] == -100, 0, t["b.target"][2])
    assert bool((tz == 0).any())


def test_training_fixture_is_consistent():
    gold = load_file(os.path.join(GOLDEN, "train_loss_components.safetensors"))
    with open(os.path.join(GOLDEN, "train_loss_components.json")) as fh:
        meta = json.load(fh)
    assert "loss.prompt_components.prompt_contrastive.t_prime" in meta["keys"]
    comps = gold["components"]
    value = 0.725 * comps[:, 0] + 0.025 * comps[:, 1] + 0.25 * comps[:, 3]
    assert torch.allclose(value, gold["loss"], rtol=1e-6)
    assert gold["t_prime"].shape == (4,) and float(gold["t_prime"][0]) == pytest.approx(math.log(10.0))
