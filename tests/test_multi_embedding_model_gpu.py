"""GPU: the per-example family (``segment_example_logits`` / ``embeddings_per_example``) through the model - inference engine, HIP graph
replay, the embedding cache and one training step - against the REFERENCE's fixtures tests/golden/multi_embedding_*
(tools/make_golden_multi_embedding.py; cases in tests/cases_multi_embedding.py).

Bounds: 2e-5 max-norm for decoder-only forward quantities (the bound of tools/make_golden.py and test_train_gpu.py for decoder-only
cases); argmax exact outside the project's 2e-3 margin band; gradients within max(3e-4, 4 e_kink) of the tensor's scale, 3e-4 being the
decoder-only bound of test_gradients_match_oracle_autograd and e_kink what the generator measured between the reference's OWN fp32 and
fp64 gradients (the maximum over examples is a kink: where two examples tie to rounding, fp32 and fp64 pick different winners).
"""
import dataclasses
import json
import os

import pytest
import torch

from labelanything_amd.episodes import make_episode
from labelanything_amd.models import Lam
from tests.cases_multi_embedding import ME_CASES, ME_TRAIN
from tests.helpers import GOLDEN, argmax_disagreement, load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
ARGMAX_MARGIN = 2e-3


def model_for(name):
    case = ME_CASES[name]
    gold, meta = load_golden(f"multi_embedding_{name}")
    lam = Lam(case["cfg"], seed=case["weight_seed"]).cuda()
    lam.selected_rows = gold.get("selected_rows")
    return lam, case, gold, meta


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
    assert torch.equal(out["logits"].argmax(dim=1).cpu(), out["argmax"].cpu())
    n_diff, n_real = argmax_disagreement(out["logits"], gold["argmax"].long(), gold["logits"], margin_rel=ARGMAX_MARGIN)
    print(f"[{name}] argmax differs on {n_diff} pixels, {n_real} outside the {ARGMAX_MARGIN:.0e} margin band")
    assert n_real == 0
    assert torch.equal(out["class_examples_embeddings"], pe["class_examples_embeddings"])


@pytest.mark.parametrize("name", ["e4", "e9_attn"])
def test_graph_replay_is_bit_identical_and_tracks_new_inputs(name):
    lam, case, gold, _ = model_for(name)
    b1 = make_episode(**case["episode"])
    b2 = make_episode(**{**case["episode"], "seed": 778})
    e1, e2 = lam.forward_argmax(b1), lam.forward_argmax(b2)
    lam.use_graphs = True
    g1 = lam.forward_argmax(b1)       # capture
    g2 = lam.forward_argmax(b2)       # replay with new inputs
    g1b = lam.forward_argmax(b1)
    torch.cuda.synchronize()
    for k in ("logits", "argmax", "class_examples_embeddings"):
        assert torch.equal(e1[k], g1[k]) and torch.equal(e2[k], g2[k]) and torch.equal(e1[k], g1b[k]), k
    assert len(lam._graphs) == 1
    assert not torch.equal(e1["logits"], e2["logits"])


@pytest.mark.parametrize("name", ["e4", "e1"])
def test_predict_from_cached_example_embeddings_matches_forward(name):
    """generate_class_embeddings keeps the per-example embeddings and the (repeated) flags; predict decodes against them."""
    from labelanything_amd.cache import set_class_embeddings
    lam, case, gold, meta = model_for(name)
    batch = make_episode(**case["episode"])
    full = lam(batch)["logits"]
    examples = {k: (v[:, 1:] if k in ("embeddings", "dims") else v) for k, v in batch.items()}
    ce = lam.generate_class_embeddings(examples)
    assert tuple(ce["class_examples_embeddings"].shape) == tuple(gold["class_examples_embeddings"].shape)
    assert tuple(ce["flag_examples"].shape) == tuple(gold["flag_examples"].shape)
    q = {"embeddings": batch["embeddings"][:, :1], "dims": batch["dims"][:, 0]}
    pred = lam.predict(q, ce)
    torch.cuda.synchronize()
    assert rel_err(pred, full) <= 1e-6
    # the test-time prototype cache (experiment/utils.py:210-249) serves the same
    set_class_embeddings(lam, {k: v[0] for k, v in examples.items()})
    assert rel_err(lam.predict(q), full) <= 1e-6


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
    from labelanything_amd.train import LamTrainer
    from tests.test_train_gpu import make_gt
    name = ME_TRAIN["case"]
    lam, case, gold_fwd, _ = model_for(name)
    from safetensors.torch import load_file
    gold = load_file(os.path.join(GOLDEN, f"multi_embedding_{name}_train.safetensors"))
    with open(os.path.join(GOLDEN, f"multi_embedding_{name}_train.json")) as fh:
        meta = json.load(fh)
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=meta["seed_gt"])
    tr = LamTrainer(lam)
    tr.zero_grad()
    res = tr.forward_backward(batch, gt)
    torch.cuda.synchronize()
    assert rel_err(res["logits"], gold_fwd["logits"]) <= TOL
    loss = float(res["loss"])
    print(f"[train {name}] loss {loss:.8f} reference {meta['loss']:.8f}")
    assert abs(loss - meta["loss"]) <= TOL * max(1.0, abs(meta["loss"]))
    e_kink = float(meta["e_kink"])
    tol = max(3e-4, 4 * e_kink)
    print(f"[train {name}] gradient bound max(3e-4, 4 * e_kink = {4 * e_kink:.3e}) = {tol:.3e}")
    grads = dict(zip(tr.names, tr.opt.grad_views))
    keys = meta["keys"]
    assert set(keys) <= set(tr.names)
    for k in meta["dead"]:                                           # never reached by the reference's forward either
        assert float(grads[k].abs().max()) == 0.0, k
    # every tensor by its norm: | ||g|| - ||ref|| | <= ||g - ref||, relative to the tensor's own norm floored at 1e-2 of the largest
    gn = torch.stack([grads[k].norm() for k in keys]).cpu()
    floor = 1e-2 * float(gold["grad_norm"].max())
    rel_n = (gn - gold["grad_norm"]).abs() / gold["grad_norm"].clamp_min(floor)
    print(f"[train {name}] worst gradient-norm difference {float(rel_n.max()):.3e} at {keys[int(rel_n.argmax())]}")
    assert float(rel_n.max()) <= tol
    # the stored tensors entry by entry, relative to the tensor's scale floored at 1e-2 of the largest stored gradient
    full = {k[5:]: v for k, v in gold.items() if k.startswith("grad.")}
    assert "mask_decoder.class_mlp.layers.2.weight" in full
    gmax = max(float(v.abs().max()) for v in full.values())
    worst = {k: float((grads[k].cpu() - v).abs().max()) / max(float(v.abs().max()), 1e-2 * gmax) for k, v in full.items()}
    print(f"[train {name}] worst entry-wise gradient difference {max(worst.values()):.3e} at {max(worst, key=worst.get)}")
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, bad


def test_trainer_refuses_prompt_contrastive_with_region_embeddings():
    from labelanything_amd.loss import LabelAnythingLoss
    from labelanything_amd.train import LamTrainer
    lam, _, _, _ = model_for("e4")
    with pytest.raises(NotImplementedError, match="prompt_contrastive"):
        LamTrainer(lam, loss=LabelAnythingLoss({"focal": {"weight": 1.0}, "prompt_contrastive": {"weight": 0.1}}))
    lam1, _, _, _ = model_for("e1")                                  # one embedding per example: the component is built
    LamTrainer(lam1, loss=LabelAnythingLoss({"focal": {"weight": 1.0}, "prompt_contrastive": {"weight": 0.1}}))
