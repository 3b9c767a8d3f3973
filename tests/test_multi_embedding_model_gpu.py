"""GPU: the per-example family (``segment_example_logits`` / ``embeddings_per_example``) through the model - inference engine, HIP graph
replay, the embedding cache and one training step - against the REFERENCE's fixtures tests/golden/multi_embedding_*
(tools/make_golden_multi_embedding.py; cases in tests/cases_multi_embedding.py).

Bounds: 2e-5 max-norm for decoder-only forward quantities (the bound of tools/make_golden.py and test_train_gpu.py for decoder-only
cases); argmax exact outside the project's 2e-3 margin band; gradients within max(3e-4, 4 e_kink) of the tensor's scale, 3e-4 being the
decoder-only bound of test_gradients_match_oracle_autograd and e_kink what the generator measured between the reference's OWN fp32 and
fp64 gradients (the maximum over examples is a kink: where two examples tie to rounding, fp32 and fp64 pick different winners).
"""
import dataclasses

import pytest
import torch

from labelanything_amd.episodes import make_episode
from labelanything_amd.models import Lam
from tests import model_checks as MC
from tests.cases_multi_embedding import ME_CASES, ME_TRAIN
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
ARGMAX_MARGIN = 2e-3


def model_for(name):
    return MC.load_model(ME_CASES, name, "multi_embedding_")


@pytest.mark.parametrize("name", list(ME_CASES))
def test_forward_matches_the_reference_fixture(name):
    lam, case, gold, meta = model_for(name)
    batch = make_episode(**case["episode"])
    seg, pe = lam._forward(batch)
    out = lam.forward_argmax(batch)
    torch.cuda.synchronize()
    assert tuple(pe["class_examples_embeddings"].shape) == tuple(gold["class_examples_embeddings"].shape)
    assert torch.equal(lam.engine().h2d(pe["flag_examples"]).cpu().to(torch.uint8), gold["flag_examples"])
    errs = {"class_examples_embeddings": rel_err(pe["class_examples_embeddings"], gold["class_examples_embeddings"]),
            "low_res_logits": rel_err(seg, gold["low_res_logits"]), "logits": rel_err(out["logits"], gold["logits"])}
    print(f"[{name}] {meta['decoder_tokens']} decoder tokens: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {TOL:.0e})")
    assert all(v <= TOL for v in errs.values()), errs
    MC.check_argmax(name, out, gold, ARGMAX_MARGIN)
    assert torch.equal(out["class_examples_embeddings"], pe["class_examples_embeddings"])


@pytest.mark.parametrize("name", ["e4", "e9_attn"])
def test_graph_replay_is_bit_identical_and_tracks_new_inputs(name):
    lam, case, _, _ = model_for(name)
    MC.check_graph_replay(lam, case, keys=("logits", "argmax", "class_examples_embeddings"))


@pytest.mark.parametrize("name", ["e4", "e1"])
def test_predict_from_cached_example_embeddings_matches_forward(name):
    """generate_class_embeddings keeps the per-example embeddings and the (repeated) flags; predict decodes against them."""
    lam, case, gold, _ = model_for(name)
    ce, _ = MC.check_cached_predict(lam, case)
    assert tuple(ce["class_examples_embeddings"].shape) == tuple(gold["class_examples_embeddings"].shape)
    assert tuple(ce["flag_examples"].shape) == tuple(gold["flag_examples"].shape)


def test_state_dict_of_the_one_prototype_model_loads():
    """No parameter is added: the state dict of the default (one prototype per class) model strict-loads and decodes per example."""
    lam, case, gold, _ = model_for("e4")
    plain = Lam(dataclasses.replace(case["cfg"], segment_example_logits=False, embeddings_per_example=None), seed=case["weight_seed"] + 50)
    res = lam.load_state_dict(plain.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    batch = make_episode(**case["episode"])
    moved = lam(batch)["logits"]
    assert torch.isfinite(moved[:, :, :8, :8]).all()
    assert rel_err(moved, gold["logits"]) > 1e-2                  # other weights: another result
    lam.load_state_dict(Lam(case["cfg"], seed=case["weight_seed"]).state_dict())
    assert rel_err(lam(batch)["logits"], gold["logits"]) <= TOL


def test_class_without_a_valid_example_is_minus_infinity():
    """Deliberate difference from the reference: its full-resolution plane of a class without any valid example is NaN
    (bilinear resampling of -inf) unless flag_gts overwrites it; here it is -inf at both resolutions, with and without flag_gts."""
    lam, case, _, _ = model_for("e4")
    batch = make_episode(**case["episode"])
    batch["flag_examples"] = batch["flag_examples"].clone()
    batch["flag_examples"][:, :, 2] = 0
    for with_gts in (True, False):
        b = dict(batch)
        if not with_gts:
            b.pop("flag_gts")
        seg, _ = lam._forward(b)
        out = lam.forward_argmax(b)
        torch.cuda.synchronize()
        assert bool((seg[:, 2] == float("-inf")).all()) and bool(torch.isfinite(seg[:, :2]).all())
        assert not bool(torch.isnan(out["logits"]).any())
        assert bool((out["logits"][:, 2] == float("-inf")).all())
        assert bool((out["argmax"] != 2).all())


def test_one_training_step_matches_the_reference():
    name = ME_TRAIN["case"]
    lam, case, gold_fwd, _ = model_for(name)
    gold, meta = MC.load_train_fixture(f"multi_embedding_{name}")
    tr, _, grads = MC.run_training_step(lam, case, gold_fwd, gold, meta, TOL, label=name)
    e_kink = float(meta["e_kink"])
    tol = max(3e-4, 4 * e_kink)
    print(f"[train {name}] gradient bound max(3e-4, 4 * e_kink = {4 * e_kink:.3e}) = {tol:.3e}")
    assert "grad.mask_decoder.class_mlp.layers.2.weight" in gold
    MC.compare_gradients(tr.names, grads, gold, meta, tol, label=name)


def test_trainer_refuses_prompt_contrastive_with_region_embeddings():
    from labelanything_amd.loss import LabelAnythingLoss
    from labelanything_amd.train import LamTrainer
    lam, _, _, _ = model_for("e4")
    with pytest.raises(NotImplementedError, match="prompt_contrastive"):
        LamTrainer(lam, loss=LabelAnythingLoss({"focal": {"weight": 1.0}, "prompt_contrastive": {"weight": 0.1}}))
    lam1, _, _, _ = model_for("e1")                                  # one embedding per example: the component is built
    LamTrainer(lam1, loss=LabelAnythingLoss({"focal": {"weight": 1.0}, "prompt_contrastive": {"weight": 0.1}}))
