"""GPU: ``conv_classification`` and ``classification_layer_downsample_rate=1`` through the model - inference engine, HIP graph replay, the
embedding cache and one training step - against the REFERENCE's fixtures tests/golden/convcls_r1, convcls_r8, nodown_r1
(tools/make_golden_convcls.py; cases in tests/cases_convcls.py).

Bounds (those of tests/test_levels_model_gpu.py): 2e-5 max-norm for decoder-only forward quantities; argmax exact outside the project's
2e-3 margin band; gradients within max(3e-4, 4 e_kink) of the tensor's scale, e_kink being what the generator measured between the
reference's OWN fp32 and fp64 gradients.
"""
import dataclasses
import json
import os

import pytest
import torch

from labelanything_amd.episodes import make_episode
from labelanything_amd.models import Lam
from tests.cases_convcls import CC_CASES, CC_TCONV, CC_TRAIN, CC_TRAIN_PLAIN
from tests.helpers import GOLDEN, argmax_disagreement, load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
ARGMAX_MARGIN = 2e-3
NEW_KEYS = CC_TCONV
NEW_WRAPPERS = ("proto_kernels", "proto_kernels_bwd", "classify_conv", "classify_conv_bwd")


def model_for(name):
    case = CC_CASES[name]
    gold, meta = load_golden(name)
    lam = Lam(case["cfg"], seed=case["weight_seed"]).cuda()
    lam.selected_rows = gold.get("selected_rows")
    return lam, case, gold, meta


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
    from labelanything_amd import _lib as L
    from labelanything_amd.train import LamTrainer
    from tests.test_train_gpu import make_gt
    lam, case, gold, _ = model_for("convcls_r8")
    batch = make_episode(**case["episode"])
    plain = default_twin(case, gold)

    def forbidden(*a, **kw):
        raise AssertionError("a kernel of conv_classification / the wide classify was launched by a default model")

    with monkeypatch.context() as mp:
        for fn in NEW_WRAPPERS + ("classify_wide", "classify_wide_bwd"):
            mp.setattr(L, fn, forbidden)
        before = plain.forward_argmax(batch)
        before = {k: before[k].clone() for k in ("logits", "argmax")}
        tr = LamTrainer(default_twin(case, gold))
        tr.zero_grad()
        tr.forward_backward(batch, make_gt(batch, batch["flag_examples"].shape[2], seed=3))
        torch.cuda.synchronize()
        assert not any("prototype_tconv" in k for k in tr.names)
    conv = lam.forward_argmax(batch)
    tr2 = LamTrainer(lam)
    tr2.zero_grad()
    tr2.forward_backward(batch, make_gt(batch, batch["flag_examples"].shape[2], seed=3))
    after = default_twin(case, gold).forward_argmax(batch)
    torch.cuda.synchronize()
    assert torch.equal(after["logits"], before["logits"]) and torch.equal(after["argmax"], before["argmax"])
    assert rel_err(conv["logits"], before["logits"]) > 1e-2                      # the head is not a no-op


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
    assert torch.equal(out["logits"].argmax(dim=1).cpu(), out["argmax"].cpu())
    n_diff, n_real = argmax_disagreement(out["logits"], gold["argmax"].long(), gold["logits"], margin_rel=ARGMAX_MARGIN)
    print(f"[{name}] argmax differs on {n_diff} pixels, {n_real} outside the {ARGMAX_MARGIN:.0e} margin band")
    assert n_real == 0


@pytest.mark.parametrize("name", list(CC_CASES))
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
    for k in ("logits", "argmax"):
        assert torch.equal(e1[k], g1[k]) and torch.equal(e2[k], g2[k]) and torch.equal(e1[k], g1b[k]), k
    assert len(lam._graphs) == 1
    assert not torch.equal(e1["logits"], e2["logits"])


@pytest.mark.parametrize("name", list(CC_CASES))
def test_predict_from_cached_embeddings_matches_forward(name):
    from labelanything_amd.cache import set_class_embeddings
    lam, case, gold, meta = model_for(name)
    batch = make_episode(**case["episode"])
    full = lam(batch)["logits"]
    examples = {k: (v[:, 1:] if k in ("embeddings", "dims") else v) for k, v in batch.items()}
    ce = lam.generate_class_embeddings(examples)
    q = {"embeddings": batch["embeddings"][:, :1], "dims": batch["dims"][:, 0]}
    pred = lam.predict(q, ce)
    torch.cuda.synchronize()
    assert rel_err(pred, full) <= 1e-6
    assert rel_err(full, gold["logits"]) <= TOL
    set_class_embeddings(lam, {k: v[0] for k, v in examples.items()})
    assert rel_err(lam.predict(q), full) <= 1e-6


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
    from labelanything_amd.train import LamTrainer
    from tests.test_train_gpu import make_gt
    lam, case, gold_fwd, _ = model_for(name)
    new_keys = NEW_KEYS if case["cfg"].conv_classification else []
    from safetensors.torch import load_file
    gold = load_file(os.path.join(GOLDEN, f"{name}_train.safetensors"))
    with open(os.path.join(GOLDEN, f"{name}_train.json")) as fh:
        meta = json.load(fh)
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=meta["seed_gt"])
    tr = LamTrainer(lam)
    # live parameters of the decoder span: in the trainer's names, in front of the dead tail, inside the decoder bucket of the flat buffer
    dead = [i for i, k in enumerate(tr.names) if k.startswith(("prompt_encoder.transformer.final_attn_token_to_image.",
                                                                "prompt_encoder.transformer.norm_final_attn."))]
    where = [tr.names.index(k) for k in new_keys]
    assert dead and all(i < min(dead) for i in where) and not (set(NEW_KEYS) - set(new_keys)) & set(tr.names)
    lo, hi = tr.reducer.bounds[tr._dec_bucket]
    for i in where:
        off = sum(p.numel() for p in tr.opt.grad_views[:i])
        assert lo <= off and off + tr.opt.grad_views[i].numel() <= hi
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
    assert set(keys) <= set(tr.names) and set(new_keys) <= set(keys)
    for k in new_keys:
        assert tr._touched[tr.names.index(k)], k
        assert float(grads[k].abs().max()) > 0
    for k in meta["dead"]:                                           # never reached by the reference's forward either
        assert float(grads[k].abs().max()) == 0.0, k
    gn = torch.stack([grads[k].norm() for k in keys]).cpu()
    floor = 1e-2 * float(gold["grad_norm"].max())
    rel_n = (gn - gold["grad_norm"]).abs() / gold["grad_norm"].clamp_min(floor)
    print(f"[train {name}] worst gradient-norm difference {float(rel_n.max()):.3e} at {keys[int(rel_n.argmax())]}")
    assert float(rel_n.max()) <= tol
    full = {k[5:]: v for k, v in gold.items() if k.startswith("grad.")}
    assert set(new_keys) <= set(full) and "mask_decoder.class_mlp.layers.2.weight" in full
    gmax = max(float(v.abs().max()) for v in full.values())
    worst = {}
    for k, v in full.items():
        mine = grads[k].cpu()
        if k in meta["sliced"]:                                      # the first input channels of a 2.4 MB tensor
            mine = mine[:meta["sliced"][k]]
        assert mine.shape == v.shape, k
        worst[k] = float((mine - v).abs().max()) / max(float(v.abs().max()), 1e-2 * gmax)
    print(f"[train {name}] worst entry-wise gradient difference {max(worst.values()):.3e} at {max(worst, key=worst.get)}")
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, bad
    # the optimizer moves them
    moving = new_keys or ["mask_decoder.class_mlp.layers.2.weight"]
    before = {k: lam.state_dict()[k].clone() for k in moving}
    tr.apply_update()
    torch.cuda.synchronize()
    assert all(not torch.equal(lam.state_dict()[k], before[k]) for k in moving)
