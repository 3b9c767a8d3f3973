"""GPU: the two-level classification head (``classification_levels=2``) through the model - inference engine, HIP graph replay, the
embedding cache and one training step - against the REFERENCE's fixtures tests/golden/levels_* (tools/make_golden_levels.py; cases in
tests/cases_levels.py; one call of the fixture run, torchvision's ``resize``, is a stand-in - see the generator).

Bounds: 2e-5 max-norm for decoder-only forward quantities (the bound of tests/test_multi_embedding_model_gpu.py); argmax exact outside the
project's 2e-3 margin band; gradients within max(3e-4, 4 e_kink) of the tensor's scale, e_kink being what the generator measured between
the reference's OWN fp32 and fp64 gradients.

``level_reducer.bias`` is inert in the stored step: it shifts every class plane alike and the focal objective is a softmax cross-entropy,
so its gradient sum(d loss / d low_res_logits) is zero analytically (the reference gives 9e-8 in fp32, 2e-17 in fp64).  It is not part of
e_kink or of the relative comparisons; the test bounds it by what summing the ``dseg_numel`` terms in any fp32 order can leave,
(n + 2) 2^-24 sum|d loss / d low_res_logits| with the sum from the reference's fp64 run - a partial sum that misses a tile is larger.
"""
import dataclasses

import pytest
import torch

from labelanything_amd.episodes import make_episode
from labelanything_amd.models import Lam
from tests import model_checks as MC
from tests.cases_levels import LV_CASES, LV_TRAIN
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
ARGMAX_MARGIN = 2e-3
NEW_KEYS = ["mask_decoder.level_reducer.weight", "mask_decoder.level_reducer.bias"]


def model_for(name):
    return MC.load_model(LV_CASES, name, "levels_")


def one_level_twin(case, gold):
    """The classification_levels = 1 model of the same weights, minus the two keys."""
    lam2 = Lam(case["cfg"], seed=case["weight_seed"])
    sd = {k: v for k, v in lam2.state_dict().items() if k not in NEW_KEYS}
    plain = Lam(dataclasses.replace(case["cfg"], classification_levels=1), seed=case["weight_seed"] + 9)
    plain.load_state_dict(sd, strict=True)
    plain = plain.cuda()
    plain.selected_rows = gold.get("selected_rows")
    return plain


def test_one_level_model_is_untouched_by_the_new_code(monkeypatch):
    """With classification_levels = 1 no new kernel is launched, and the logits are the same bits before and after the new kernels (forward
    and backward) have run in the process."""
    lam, case, gold, _ = model_for("l2")
    MC.check_default_model_untouched(monkeypatch, lam, case, lambda: one_level_twin(case, gold),
                                     ("classify_wide", "classify_wide_bwd", "level_reduce", "level_reduce_bwd"), "level_reducer",
                                     "a kernel of the two-level head was launched by a classification_levels=1 model")


@pytest.mark.parametrize("name", list(LV_CASES))
def test_forward_matches_the_reference_fixture(name):
    lam, case, gold, meta = model_for(name)
    batch = make_episode(**case["episode"])
    seg, pe = lam._forward(batch)
    g = meta["grid"]
    b, c = seg.shape[:2]
    cls1 = lam.engine(validate=False).f32("md.cls1", (b, c, g, g)).clone()      # the arena buffer the forward wrote
    cls0 = lam.engine(validate=False).f32("md.cls0", (b, c, 4 * g, 4 * g)).clone()
    out = lam.forward_argmax(batch)
    torch.cuda.synchronize()
    errs = {"cls1": rel_err(cls1, gold["cls1"]), "cls0": rel_err(cls0, gold["cls0"]), "low_res_logits": rel_err(seg, gold["low_res_logits"]),
            "logits": rel_err(out["logits"], gold["logits"])}
    print(f"[{name}] " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {TOL:.0e}); scales {meta['scale']}")
    assert all(v <= TOL for v in errs.values()), errs
    MC.check_argmax(name, out, gold, ARGMAX_MARGIN)


@pytest.mark.parametrize("name", list(LV_CASES))
def test_graph_replay_is_bit_identical_and_tracks_new_inputs(name):
    lam, case, _, _ = model_for(name)
    MC.check_graph_replay(lam, case)


@pytest.mark.parametrize("name", list(LV_CASES))
def test_predict_from_cached_embeddings_matches_forward(name):
    lam, case, gold, _ = model_for(name)
    _, full = MC.check_cached_predict(lam, case)
    assert rel_err(full, gold["logits"]) <= TOL


def test_other_level_reducer_weights_change_the_logits():
    lam, case, gold, _ = model_for("l2")
    batch = make_episode(**case["episode"])
    sd = {k: v.clone() for k, v in lam.state_dict().items()}
    assert list(sd)[-2:] == NEW_KEYS
    moved = dict(sd)
    moved[NEW_KEYS[0]] = sd[NEW_KEYS[0]].flip(1)                                 # the two levels swap their taps
    res = lam.load_state_dict(moved, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert rel_err(lam(batch)["logits"], gold["logits"]) > 1e-2
    moved[NEW_KEYS[0]] = sd[NEW_KEYS[0]]
    moved[NEW_KEYS[1]] = sd[NEW_KEYS[1]] + 1.0
    lam.load_state_dict(moved, strict=True)
    seg, _ = lam._forward(batch)
    torch.cuda.synchronize()
    assert rel_err(seg - 1.0, gold["low_res_logits"]) <= TOL                     # the bias is added once per pixel
    lam.load_state_dict(sd, strict=True)
    assert rel_err(lam(batch)["logits"], gold["logits"]) <= TOL


def test_one_training_step_matches_the_reference():
    name = LV_TRAIN["case"]
    lam, case, gold_fwd, _ = model_for(name)
    gold, meta = MC.load_train_fixture(f"levels_{name}")
    tr, _, grads = MC.run_training_step(lam, case, gold_fwd, gold, meta, TOL, label=name)
    # live parameters of the decoder span: in the trainer's names, in front of the dead tail, inside the decoder bucket
    dead = [i for i, k in enumerate(tr.names) if k.startswith(("prompt_encoder.transformer.final_attn_token_to_image.",
                                                                "prompt_encoder.transformer.norm_final_attn."))]
    where = [tr.names.index(k) for k in NEW_KEYS]
    assert dead and max(where) < min(dead)
    lo, hi = tr.reducer.bounds[tr._dec_bucket]
    for i in where:
        off = sum(p.numel() for p in tr.opt.grad_views[:i])
        assert lo <= off and off + tr.opt.grad_views[i].numel() <= hi
    e_kink = float(meta["e_kink"])
    tol = max(3e-4, 4 * e_kink)
    print(f"[train {name}] gradient bound max(3e-4, 4 * e_kink = {4 * e_kink:.3e}) = {tol:.3e}")
    keys = meta["keys"]
    assert NEW_KEYS[0] in keys and meta["inert"] == [NEW_KEYS[1]] and NEW_KEYS[1] not in keys
    assert float(grads[NEW_KEYS[0]].abs().min()) > 0
    for k in NEW_KEYS:
        assert tr._touched[tr.names.index(k)], k
    noise = (meta["dseg_numel"] + 2) * 2.0 ** -24 * meta["dseg_abs_sum"]
    dbias = float(grads[NEW_KEYS[1]].abs().max())
    print(f"[train {name}] inert level_reducer.bias gradient {dbias:.3e} (reference fp32 {meta['inert_reference_fp32']:.3e}); "
          f"[derived] bound {noise:.3e}")
    assert dbias <= noise
    assert {"grad." + k for k in NEW_KEYS} <= set(gold)
    MC.compare_gradients(tr.names, grads, gold, meta, tol, label=name)       # (leaves the inert bias, bounded above, out of both comparisons)
    # the optimizer moves them
    before = {k: lam.state_dict()[k].clone() for k in NEW_KEYS}
    tr.apply_update()
    torch.cuda.synchronize()
    assert all(not torch.equal(lam.state_dict()[k], before[k]) for k in NEW_KEYS)
