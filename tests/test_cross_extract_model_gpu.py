"""GPU: ``embedding_extraction="cross_attention"`` through the model - inference engine, HIP graph replay and the embedding cache - against
the REFERENCE's fixtures tests/golden/cross_extract_* (tools/make_golden_cross_extract.py; cases in tests/cases_cross_extract.py).

Bounds, as in tests/test_multi_embedding_model_gpu.py: 2e-5 max-norm for decoder-only forward quantities (the bound of
tools/make_golden.py for decoder-only cases); argmax exact outside the project's 2e-3 margin band.
"""
import pytest
import torch

from labelanything_amd.episodes import make_episode
from tests import model_checks as MC
from tests.cases_cross_extract import XE_CASES
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
ARGMAX_MARGIN = 2e-3


def model_for(name):
    return MC.load_model(XE_CASES, name, "cross_extract_")


@pytest.mark.parametrize("name", list(XE_CASES))
def test_forward_matches_the_reference_fixture(name):
    lam, case, gold, meta = model_for(name)
    batch = make_episode(**case["episode"])
    seg, pe = lam._forward(batch)
    out = lam.forward_argmax(batch)
    torch.cuda.synchronize()
    assert tuple(pe["class_examples_embeddings"].shape) == tuple(gold["class_examples_embeddings"].shape)
    assert "class_embeddings" not in pe                                      # the reference's result has no class mean in this mode
    assert torch.equal(lam.engine().h2d(pe["flag_examples"]).cpu().to(torch.uint8), gold["flag_examples"])
    errs = {"class_examples_embeddings": rel_err(pe["class_examples_embeddings"], gold["class_examples_embeddings"]),
            "low_res_logits": rel_err(seg, gold["low_res_logits"]), "logits": rel_err(out["logits"], gold["logits"])}
    print(f"[{name}] {meta['folded_queries']} folded queries per pair: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {TOL:.0e})")
    assert all(v <= TOL for v in errs.values()), errs
    MC.check_argmax(name, out, gold, ARGMAX_MARGIN)
    assert set(out) == {"logits", "class_examples_embeddings", "argmax"}     # the reference's keys (+ the fused argmax)
    assert torch.equal(out["class_examples_embeddings"], pe["class_examples_embeddings"])


@pytest.mark.parametrize("name", list(XE_CASES))
def test_graph_replay_is_bit_identical_and_tracks_new_inputs(name):
    lam, case, _, _ = model_for(name)
    MC.check_graph_replay(lam, case, keys=("logits", "argmax", "class_examples_embeddings"))


@pytest.mark.parametrize("name", ["x4", "x1"])
def test_predict_from_cached_example_embeddings_matches_forward(name):
    """generate_class_embeddings keeps the extracted embeddings and their (B, n, C) flags; predict decodes against them.  (The cached path
    takes post-neck embeddings, lam.py:193-213: the two cases without a neck.)"""
    lam, case, gold, _ = model_for(name)
    ce, _ = MC.check_cached_predict(lam, case, exact=True)
    assert tuple(ce["class_examples_embeddings"].shape) == tuple(gold["class_examples_embeddings"].shape)
    assert tuple(ce["flag_examples"].shape) == tuple(gold["flag_examples"].shape) and "class_embeddings" not in ce


def test_padded_supports_take_part_like_the_reference_s():
    """The key mask is a no-op (common.py:120-124): clearing a support's flag for a class that another support still shows changes no
    embedding - only the (B, n, C) flags would change if no support showed the class at all."""
    lam, case, gold, _ = model_for("x4")
    batch = make_episode(**case["episode"])
    _, pe = lam._forward(batch)
    base = pe["class_examples_embeddings"].clone()
    fe = batch["flag_examples"].clone()
    assert int(fe[0, :, 1].sum()) >= 2
    first = int(fe[0, :, 1].nonzero()[0])
    fe[0, first, 1] = 0
    _, pe2 = lam._forward({**batch, "flag_examples": fe})
    torch.cuda.synchronize()
    assert torch.equal(pe2["class_examples_embeddings"], base)
    assert torch.equal(lam.engine().h2d(pe2["flag_examples"]).cpu().to(torch.uint8), gold["flag_examples"])


def test_class_without_a_valid_example_is_minus_infinity():
    """The documented behaviour of the per-example family: -inf planes at both resolutions, never NaN."""
    lam, case, _, _ = model_for("x4")
    batch = make_episode(**case["episode"])
    batch["flag_examples"] = batch["flag_examples"].clone()
    batch["flag_examples"][:, :, 2] = 0
    for with_gts in (True, False):
        b = dict(batch)
        if not with_gts:
            b.pop("flag_gts")
        seg, pe = lam._forward(b)
        out = lam.forward_argmax(b)
        torch.cuda.synchronize()
        assert bool((lam.engine().h2d(pe["flag_examples"])[:, :, 2] == 0).all())
        assert bool((seg[:, 2] == float("-inf")).all()) and bool(torch.isfinite(seg[:, :2]).all())
        assert not bool(torch.isnan(out["logits"]).any())
        assert bool((out["logits"][:, 2] == float("-inf")).all())
        assert bool((out["argmax"] != 2).all())


def test_the_recipe_constructs_strict_loads_and_runs():
    """The model section of parameters/validation/Pascal/mae_cross.yaml on its 30 x 30 grid: a state dict with the reference's key names
    strict-loads and an episode of precomputed 768-channel embeddings runs."""
    from labelanything_amd.models import build_lam_no_vit
    from labelanything_amd.weights import init_state_dict
    kw = dict(image_size=480, image_embed_dim=768, embed_dim=256, spatial_convs=3, embeddings_per_example=4,
              embedding_extraction="cross_attention", class_attention=False, example_attention=False, example_class_attention=False)
    lam = build_lam_no_vit(**kw)
    sd = init_state_dict(lam.cfg, 5)
    assert sum(k.startswith("prompt_encoder.embedding_extraction.") for k in sd) == 37
    res = lam.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    lam = lam.cuda()
    batch = make_episode(batch=1, n_ways=2, k_shots=1, image_size=480, seed=9, prompts=("mask",), embeddings_channels=768, grid=30)
    out = lam(batch)
    torch.cuda.synchronize()
    b, m, c = batch["flag_examples"].shape
    assert tuple(out["class_examples_embeddings"].shape) == (b, 4, c, 256)
    assert tuple(out["logits"].shape[:2]) == (b, c) and bool(torch.isfinite(out["logits"]).all())
