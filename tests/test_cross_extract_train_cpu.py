"""CPU: the host side of training ``embedding_extraction="cross_attention"`` - the query-dropout rule (``draw_extraction_keep``), the
opt-in and refusal matrix of ``LamTrainer`` (the error paths that come before the device check) and the meta of the training fixtures
tests/golden/cross_extract_<case>_train.* (tools/make_golden_cross_extract_train.py; cases in tests/cases_cross_extract_train.py)."""
import os
import re

import pytest
import torch

from labelanything_amd import _lib
from labelanything_amd.config import config_from_kwargs
from labelanything_amd.models import Lam
from labelanything_amd.train import LamTrainer, draw_extraction_keep
from tests import model_checks as MC
from tests.cases_cross_extract import XE_CASES
from tests.cases_cross_extract_train import (EX, XE_FLOOR, XE_GRAD_TOL, XE_MIN_LIVE_EXTRACTION_ABOVE, XE_MIN_UPSTREAM_ABOVE, XE_MUST_BE_ABOVE,
                                             XE_TRAIN, XE_TRAIN_FULL, XE_TRAIN_SLICED, XE_TRAIN_SLICED_ROWS)
from tests.helpers import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(image_size=64, embed_dim=64, image_embed_dim=64)
XA = dict(embedding_extraction="cross_attention")
NORM3 = sorted(f"{EX}layers.{l}.norm3.{p}" for l in range(2) for p in ("weight", "bias"))
NEW_EXPORTS = ["la_extract_pool_lse", "la_extract_pool_bwd_plan", "la_extract_pool_bwd", "la_extract_fold_bwd", "la_extract_unfold_bwd"]


def cfg_of(**kw):
    return config_from_kwargs(encoder=None, use_vit=False, **SMALL, **kw)


# ---- the keep mask --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(4, 0.2), (5, 0.2), (16, 0.2), (4, 0.0), (3, 0.9)])
def test_draw_follows_the_reference_rule_over_seeds(n, p):
    """prompt_encoder.py:302-305 restated: torch.rand(n) > p, and if nothing survives one torch.randint(0, n, (1,)) - the same draws in the
    same order from the host generator, which is left in the same state."""
    fallbacks = 0
    for seed in range(200):
        torch.manual_seed(seed)
        want = torch.rand(n) > p
        if not want.any():
            fallbacks += 1
            want[torch.randint(0, n, (1,)).item()] = True
        state = torch.get_rng_state()
        torch.manual_seed(seed)
        got = draw_extraction_keep(n, p)
        assert got.dtype == torch.bool and tuple(got.shape) == (n,) and torch.equal(got, want) and bool(got.any())
        assert torch.equal(torch.get_rng_state(), state)
    assert (fallbacks > 0) == (p == 0.9)                     # at p = 0.9 and n = 3 the fallback is taken for 7 seeds in 10
    if p == 0.0:
        assert bool(draw_extraction_keep(n, 0.0).all())


def test_nothing_survives_with_one_query_and_the_fallback_picks_it():
    hits = 0
    for seed in range(100):
        torch.manual_seed(seed)
        lost = not bool((torch.rand(1) > 0.2).any())
        torch.manual_seed(seed)
        keep = draw_extraction_keep(1, 0.2)
        assert keep.tolist() == [True]
        hits += lost
    assert hits > 0                                          # about one seed in five goes through the fallback


def test_the_fixture_seeds_give_the_masks_the_fixtures_hold():
    want = {"x4": [True, True, False, False], "x5_d64": [True, True, True, True, False]}
    for spec in XE_TRAIN:
        torch.manual_seed(spec["keep_seed"])
        n = int(XE_CASES[spec["case"]]["cfg"].embeddings_per_example)
        assert draw_extraction_keep(n, 0.2).tolist() == want[spec["case"]]


# ---- LamTrainer: opt-in and refusals ---------------------------------------------------------------------------------------------------
def test_the_trainer_asks_for_the_dropout_by_name():
    lam = Lam(cfg_of(embeddings_per_example=4, **XA), seed=1)
    with pytest.raises(NotImplementedError, match=r"embedding_extraction.*embedding_dropout.*0\.2.*0\.0"):
        LamTrainer(lam)
    with pytest.raises(NotImplementedError, match="embedding_dropout"):
        LamTrainer(lam, embedding_dropout=None)
    assert lam.extraction_keep is None and Lam(cfg_of(), seed=1).extraction_keep is None


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5])
def test_a_dropout_outside_the_unit_interval_is_refused(p):
    with pytest.raises(ValueError, match="embedding_dropout"):
        LamTrainer(Lam(cfg_of(embeddings_per_example=4, **XA), seed=1), embedding_dropout=p)


def test_a_dropout_for_a_model_without_extraction_is_refused():
    for kw in (dict(), dict(embeddings_per_example=4)):
        with pytest.raises(ValueError, match="embedding_dropout"):
            LamTrainer(Lam(cfg_of(**kw), seed=1), embedding_dropout=0.2)


def test_with_the_dropout_the_next_refusal_is_the_device():
    """On the CPU a trainer that got past the configuration checks stops at the device check: the extraction is no longer what refuses."""
    for p in (0.0, 0.2):
        with pytest.raises(RuntimeError, match="MI355X"):
            LamTrainer(Lam(cfg_of(embeddings_per_example=4, **XA), seed=1), embedding_dropout=p)


def test_prompt_contrastive_with_extraction_stays_refused():
    from labelanything_amd.loss import LabelAnythingLoss
    loss = LabelAnythingLoss({"focal": {"weight": 1.0}, "prompt_contrastive": {"weight": 0.1}}, class_weighting=True)
    with pytest.raises(NotImplementedError, match="prompt_contrastive.*embedding_extraction"):
        LamTrainer(Lam(cfg_of(embeddings_per_example=4, **XA), seed=1), loss=loss, embedding_dropout=0.2)
    with pytest.raises(RuntimeError, match="MI355X"):      # the focal term alone gets through
        LamTrainer(Lam(cfg_of(embeddings_per_example=4, **XA), seed=1), loss=LabelAnythingLoss({"focal": {"weight": 1.0}}, class_weighting=True),
                   embedding_dropout=0.2)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", XE_TRAIN, ids=[s["case"] for s in XE_TRAIN])
def test_training_fixture_meta_and_conditions(spec):
    name = spec["case"]
    gold, meta = MC.load_train_fixture(f"cross_extract_{name}")
    cfg = XE_CASES[name]["cfg"]
    n = int(cfg.embeddings_per_example)
    assert meta["case"] == name and meta["seed_gt"] == spec["seed_gt"] == 17 and meta["keep_seed"] == spec["keep_seed"]
    assert meta["generated_by"] == "tools/make_golden_cross_extract_train.py" and meta["embedding_dropout"] == 0.2
    keep = gold["extraction_keep"].bool()
    assert keep.tolist() == meta["extraction_keep"] and keep.numel() == n and bool(keep.any()) and not bool(keep.all())
    # the returned flags: valid classes times the mask
    flags = gold["flag_examples"].bool()
    assert tuple(flags.shape)[1] == n and torch.equal(flags, flags.any(dim=1, keepdim=True) & keep.view(1, n, 1))
    # live and dead tensors: the four norm3 are the only extraction tensors without a gradient, and every model parameter is listed
    assert sorted(k for k in meta["dead"] if k.startswith(EX)) == NORM3
    lam = Lam(cfg, seed=XE_CASES[name]["weight_seed"])
    assert sorted(meta["keys"] + meta["dead"]) == sorted(k for k, _ in lam.named_parameters())
    assert len([k for k in meta["keys"] if k.startswith(EX)]) == meta["live_extraction_tensors"] == 33
    # the generator's conditions as it measured them
    assert 4 * meta["e_ref32"] <= XE_GRAD_TOL == 3e-4 and abs(meta["four_e_ref32"] - 4 * meta["e_ref32"]) < 1e-12
    assert meta["floor"] == XE_FLOOR == 1e-2 and sorted(meta["norm_over_largest"]) == sorted(XE_MUST_BE_ABOVE)
    assert all(v > XE_FLOOR for v in meta["norm_over_largest"].values())
    assert meta["live_extraction_above_floor"] >= XE_MIN_LIVE_EXTRACTION_ABOVE == 29
    assert (meta["upstream_tensors"], meta["upstream_above_floor"] >= XE_MIN_UPSTREAM_ABOVE[name][1]) == (XE_MIN_UPSTREAM_ABOVE[name][0], True)
    assert XE_MIN_UPSTREAM_ABOVE["x4"] == (101, 80)
    # the same figures from the stored norms
    norms = dict(zip(meta["keys"], gold["grad_norm"].tolist()))
    floor = XE_FLOOR * max(norms.values())
    assert sum(norms[k] > floor for k in meta["keys"] if k.startswith(EX)) == meta["live_extraction_above_floor"]
    assert all(norms[k] > floor for k in XE_MUST_BE_ABOVE)
    assert abs(float(gold["loss"]) - meta["loss"]) < 1e-7 and abs(meta["loss"] - meta["loss_fp64"]) <= 1e-6 * abs(meta["loss_fp64"])
    # stored gradients: the full list, and the first rows of the wide MLP weights
    shapes = dict((k, tuple(p.shape)) for k, p in lam.named_parameters())
    for k in XE_TRAIN_FULL:
        assert tuple(gold["grad." + k].shape) == shapes[k], k
    assert meta["sliced"] == {k: XE_TRAIN_SLICED_ROWS for k in XE_TRAIN_SLICED}
    for k in XE_TRAIN_SLICED:
        assert tuple(gold["grad." + k].shape) == (XE_TRAIN_SLICED_ROWS,) + shapes[k][1:], k
    for l in range(2):                                    # the reference's k_proj.bias gradient is rounding noise around an exact zero
        kb = f"{EX}layers.{l}.cross_attn_image_to_token.k_proj.bias"
        assert kb in meta["keys"] and norms[kb] <= 1e-5 * max(norms.values())
    # sizes: every committed file stays below 1 MiB, the logits in a file of their own
    from safetensors.torch import load_file
    logits = load_file(os.path.join(GOLDEN, f"cross_extract_{name}_train_logits.safetensors"))["logits"]
    eval_gold = load_file(os.path.join(GOLDEN, f"cross_extract_{name}.safetensors"))
    assert logits.shape == eval_gold["logits"].shape and not torch.equal(logits, eval_gold["logits"])       # a query is dropped
    assert torch.equal(gold["selected_rows"], eval_gold["selected_rows"])
    for stem in (f"cross_extract_{name}_train.safetensors", f"cross_extract_{name}_train_logits.safetensors", f"cross_extract_{name}_train.json"):
        assert os.path.getsize(os.path.join(GOLDEN, stem)) < (1 << 20), stem


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_with_their_citations():
    with open(os.path.join(ROOT, "include", "la_hip.h")) as fh:
        header = fh.read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS
        assert re.search(rf"\bint {name}\(", header), name
    for cite in ("prompt_encoder.py:289-313", "prompt_encoder.py:301-307"):
        assert cite in header, cite
    assert _lib.SIGNATURES["la_extract_pool_bwd_plan"] == _lib.SIGNATURES["la_extract_pool_plan"]
