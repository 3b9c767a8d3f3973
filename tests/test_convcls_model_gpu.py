"""GPU: ``conv_classification`` and ``classification_layer_downsample_rate=1`` through the model - inference engine, HIP graph replay, the
embedding cache and one training step - against the REFERENCE's fixtures tests/golden/convcls_r1, convcls_r8, nodown_r1
(tools/make_golden_convcls.py; cases in tests/cases_convcls.py).

Bounds (those of tests/test_levels_model_gpu.py): 2e-5 max-norm for decoder-only forward quantities; argmax exact outside the project's
2e-3 margin band; gradients within max(3e-4, 4 e_kink) of the tensor's scale, e_kink being what the generator measured between the
reference's OWN fp32 and fp64 gradients.
"""
import dataclasses

import pytest
import torch

from labelanything_amd.episodes import make_episode
from labelanything_amd.models import Lam
from tests import model_checks as MC
from tests.cases_convcls import CC_CASES, CC_TCONV, CC_TRAIN, CC_TRAIN_PLAIN
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
ARGMAX_MARGIN = 2e-3
NEW_KEYS = CC_TCONV
NEW_WRAPPERS = ("proto_kernels", "proto_kernels_bwd", "classify_conv", "classify_conv_bwd")


def model_for(name):
    return MC.load_model(CC_CASES, name)


def default_twin(case, gold):
    """The default-configuration model (rate 8, no prototype_tconv) of the convcls_r8 weights, minus the two keys."""
    sd = {k: v for k, v in Lam(case["cfg"], seed=case["weight_seed"]).state_dict().items() if k not in NEW_KEYS}
    plain = Lam(dataclasses.replace(case["cfg"], conv_classification=False), seed=case["weight_seed"] + 9)
    plain.load_state_dict(sd, strict=True)
    plain = plain.cuda()
    plain.selected_rows = gold.get("selected_rows")
    return plain


def test_default_model_is_untouched_by_the_new_code(monkeypatch):
    """With both switches at their defaults no new kernel is launched (nor the wide classify), and the logits are the same bits before and
    after the new kernels (forward and backward) have run in the process."""
    lam, case, gold, _ = model_for("convcls_r8")
    MC.check_default_model_untouched(monkeypatch, lam, case, lambda: default_twin(case, gold),
                                     NEW_WRAPPERS + ("classify_wide", "classify_wide_bwd"), "prototype_tconv",
                                     "a kernel of conv_classification / the wide classify was launched by a default model")


@pytest.mark.parametrize("name", list(CC_CASES))
def test_forward_matches_the_reference_fixture(name):
    lam, case, gold, meta = model_for(name)
    batch = make_episode(**case["episode"])
    seg, pe = lam._forward(batch)
    out = lam.forward_argmax(batch)
    torch.cuda.synchronize()
    errs = {"low_res_logits": rel_err(seg, gold["low_res_logits"]), "logits": rel_err(out["logits"], gold["logits"])}
    print(f"[{name}] " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {TOL:.0e}); scales {meta['scale']}")
    assert all(v <= TOL for v in errs.values()), errs
    MC.check_argmax(name, out, gold, ARGMAX_MARGIN)


@pytest.mark.parametrize("name", list(CC_CASES))
def test_graph_replay_is_bit_identical_and_tracks_new_inputs(name):
    lam, case, _, _ = model_for(name)
    MC.check_graph_replay(lam, case)


@pytest.mark.parametrize("name", list(CC_CASES))
def test_predict_from_cached_embeddings_matches_forward(name):
    lam, case, gold, _ = model_for(name)
    _, full = MC.check_cached_predict(lam, case)
    assert rel_err(full, gold["logits"]) <= TOL


def test_other_prototype_tconv_weights_change_the_logits():
    lam, case, gold, _ = model_for("convcls_r1")
    batch = make_episode(**case["episode"])
    sd = {k: v.clone() for k, v in lam.state_dict().items()}
    assert list(sd)[-2:] == NEW_KEYS
    moved = dict(sd)
    moved[NEW_KEYS[1]] = sd[NEW_KEYS[1]].flip(2)                                # the second layer's rows swap top and bottom
    res = lam.load_state_dict(moved, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert rel_err(lam(batch)["logits"], gold["logits"]) > 1e-2
    lam.load_state_dict(sd, strict=True)
    assert rel_err(lam(batch)["logits"], gold["logits"]) <= TOL


@pytest.mark.parametrize("name", [CC_TRAIN["case"], CC_TRAIN_PLAIN["case"]])
def test_one_training_step_matches_the_reference(name):
    """convcls_r1: the two new autograd nodes (la_proto_kernels_bwd, la_classify_conv_bwd).  nodown_r1: the training graph's branch for a
    map wider than 64 channels without the prototype kernels, la_classify_wide / la_classify_wide_bwd on the 256-channel features."""
    lam, case, gold_fwd, _ = model_for(name)
    new_keys = NEW_KEYS if case["cfg"].conv_classification else []
    gold, meta = MC.load_train_fixture(name)
    tr, _, grads = MC.run_training_step(lam, case, gold_fwd, gold, meta, TOL, label=name)
    # live parameters of the decoder span: in the trainer's names, in front of the dead tail, inside the decoder bucket of the flat buffer
    dead = [i for i, k in enumerate(tr.names) if k.startswith(("prompt_encoder.transformer.final_attn_token_to_image.",
                                                                "prompt_encoder.transformer.norm_final_attn."))]
    where = [tr.names.index(k) for k in new_keys]
    assert dead and all(i < min(dead) for i in where) and not (set(NEW_KEYS) - set(new_keys)) & set(tr.names)
    lo, hi = tr.reducer.bounds[tr._dec_bucket]
    for i in where:
        off = sum(p.numel() for p in tr.opt.grad_views[:i])
        assert lo <= off and off + tr.opt.grad_views[i].numel() <= hi
    e_kink = float(meta["e_kink"])
    tol = max(3e-4, 4 * e_kink)
    print(f"[train {name}] gradient bound max(3e-4, 4 * e_kink = {4 * e_kink:.3e}) = {tol:.3e}")
    assert set(new_keys) <= set(meta["keys"])
    for k in new_keys:
        assert tr._touched[tr.names.index(k)], k
        assert float(grads[k].abs().max()) > 0
    assert {"grad." + k for k in new_keys} <= set(gold) and "grad.mask_decoder.class_mlp.layers.2.weight" in gold
    MC.compare_gradients(tr.names, grads, gold, meta, tol, label=name)       # (meta["sliced"]: the first input channels of a 2.4 MB tensor)
    # the optimizer moves them
    moving = new_keys or ["mask_decoder.class_mlp.layers.2.weight"]
    before = {k: lam.state_dict()[k].clone() for k in moving}
    tr.apply_update()
    torch.cuda.synchronize()
    assert all(not torch.equal(lam.state_dict()[k], before[k]) for k in moving)
