"""GPU: the TokenPool prompt encoder (``prompt_encoder="TokenPool"``) through the model - inference engine, HIP graph replay, the embedding
cache, the recipe's constructor call and one training step - against the REFERENCE's fixtures tests/golden/token_pool_*
(tools/make_golden_token_pool.py; cases in tests/cases_token_pool.py).

Bounds: 2e-5 max-norm for decoder-only forward quantities (the bound of tools/make_golden.py and test_train_gpu.py for decoder-only
cases); argmax exact outside the project's 2e-3 margin band; gradients within 3e-4 of the tensor's scale floored at 1e-2 of the largest
gradient, the decoder-only bound of test_gradients_match_oracle_autograd (there is no max-over-examples kink on this path).  The
reference's own fp32-vs-fp64 gradient error (``e_ref32`` of the fixture's json) is printed beside the measured figure.
"""
import pytest
import torch

from labelanything_amd.episodes import make_episode
from labelanything_amd.models import build_lam_no_vit
from tests import model_checks as MC
from tests.cases_token_pool import SRC_STRIDE, TP_CASES, TP_TRAIN
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
ARGMAX_MARGIN = 2e-3
GRAD_TOL = 3e-4
FINAL = ("prompt_encoder.transformer.final_attn_token_to_image.", "prompt_encoder.transformer.norm_final_attn.")


def model_for(name):
    return MC.load_model(TP_CASES, name, "token_pool_")


def forward_errors(lam, case, gold):
    batch = make_episode(**case["episode"])
    b, m, c = batch["flag_examples"].shape
    g, d, st = case["cfg"].grid, case["cfg"].embed_dim, SRC_STRIDE
    examples = {k: (v[:, 1:] if k in ("embeddings", "dims") else v) for k, v in batch.items()}
    seg, pe = lam._forward(batch)
    out = lam.forward_argmax(batch)
    torch.cuda.synchronize()
    errs = {"class_embeddings": rel_err(pe["class_embeddings"], gold["class_embeddings"]),
            "class_examples_embeddings": rel_err(pe["class_examples_embeddings"], gold["class_examples_embeddings"]),
            "low_res_logits": rel_err(seg, gold["low_res_logits"]), "logits": rel_err(out["logits"], gold["logits"])}
    if not case["cfg"].lam_neck:         # (generate_class_embeddings takes post-neck embeddings: the stream is read where there is no neck)
        src = lam.generate_class_embeddings(examples)["class_examples_src"]          # (B M, D, g, g): one slab per support image
        assert tuple(src.shape) == (b * m, d, g, g)
        errs["class_examples_src"] = rel_err(src[:, ::st, ::st, ::st].permute(0, 2, 3, 1).flatten(1, 2), gold["class_examples_src_sample"])
    return errs, out, pe


@pytest.mark.parametrize("name", list(TP_CASES))
def test_forward_matches_the_reference_fixture(name):
    """la_mask_embed_pooled, the two-way transformer over B M groups with its token output, the token mean, merge and class mean."""
    lam, case, gold, meta = model_for(name)
    errs, out, pe = forward_errors(lam, case, gold)
    print(f"[{name}] {meta['supports']} supports x {meta['classes']} classes: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items())
          + f" (bound {TOL:.0e})")
    assert tuple(pe["class_examples_embeddings"].shape) == tuple(gold["class_examples_embeddings"].shape)
    assert all(v <= TOL for v in errs.values()), errs
    MC.check_argmax(name, out, gold, ARGMAX_MARGIN)
    assert torch.equal(out["class_examples_embeddings"], pe["class_examples_embeddings"])


@pytest.mark.parametrize("name", ["tp_d256", "tp_masks"])
def test_fused_and_unfused_two_way_paths_agree(name):
    """The D = 256 cases take the fused two-way kernels (6 and 3 tokens a support); with the engine's switch off the same model runs the
    GEMM + attention + norm chain on the 16-bit operands la_mask_embed_pooled emits, within the forward bound of the reference."""
    from labelanything_amd.engine import LamEngine
    lam, case, gold, _ = model_for(name)
    fused = lam.engine()
    assert fused.fuse_twoway and fused.fused_ok(6)
    e_fused, out_fused, _ = forward_errors(lam, case, gold)
    lam._engine = LamEngine(lam.cfg, lam.state_dict(), lam._device(), lam.compute_dtype, lam.decoder_dtype, lam.precise, fuse_twoway=False)
    assert not lam.engine().fuse_twoway and not lam.engine().fused_ok(1)
    e_chain, out_chain, _ = forward_errors(lam, case, gold)
    between = rel_err(out_chain["logits"], out_fused["logits"])
    print(f"[{name}] fused {max(e_fused.values()):.2e}, unfused chain {max(e_chain.values()):.2e} against the reference; {between:.2e} between them")
    assert all(v <= TOL for v in e_chain.values()), e_chain
    assert between <= TOL


@pytest.mark.parametrize("name", ["tp_d256", "tp_d64"])
def test_graph_replay_is_bit_identical_and_tracks_new_inputs(name):
    lam, case, _, _ = model_for(name)
    MC.check_graph_replay(lam, case, keys=("logits", "argmax", "class_examples_embeddings"))


@pytest.mark.parametrize("name", ["tp_d256", "tp_masks"])
def test_predict_from_cached_class_embeddings_matches_forward(name):
    lam, case, gold, _ = model_for(name)
    ce, _ = MC.check_cached_predict(lam, case)
    assert tuple(ce["class_embeddings"].shape) == tuple(gold["class_embeddings"].shape)
    assert rel_err(ce["class_embeddings"], gold["class_embeddings"]) <= TOL


def test_the_recipe_builds_loads_and_runs():
    """The model section of parameters/trainval/pascal/mae_pool.yaml: 480 px, 768-channel precomputed embeddings behind the neck, D = 256,
    30 x 30 grid, class-encoder bank of 100, mask prompts.  A state dict with the reference's key names (the plain model's) strict-loads;
    one small episode runs, and TokenPool is what ran: the plain prompt encoder on the same weights gives other logits."""
    kw = dict(spatial_convs=3, class_attention=False, example_attention=False, example_class_attention=True,
              fusion_transformer="TwoWayTransformer", image_embed_dim=768, embed_dim=256, image_size=480,
              class_encoder={"name": "RandomMatrixEncoder", "bank_size": 100, "embed_dim": 256})
    lam = build_lam_no_vit(prompt_encoder="TokenPool", seed=5, **kw).cuda()
    plain = build_lam_no_vit(seed=6, **kw).cuda()
    res = lam.load_state_dict(plain.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys and lam.cfg.grid == 30 and lam.cfg.prompt_encoder == "TokenPool"
    batch = make_episode(batch=1, n_ways=2, k_shots=1, image_size=480, seed=31, prompts=("mask",), embeddings_channels=768, grid=30,
                         dims=[[480, 360]] * 3)
    lam.selected_rows = plain.selected_rows = torch.tensor([0, 17, 42])
    out, ref = lam.forward_argmax(batch), plain.forward_argmax(batch)
    torch.cuda.synchronize()
    assert tuple(out["logits"].shape) == (1, 3, 480, 360) and tuple(out["class_examples_embeddings"].shape) == (1, 2, 3, 256)
    assert bool(torch.isfinite(out["logits"]).all())
    assert rel_err(out["logits"], ref["logits"]) > 1e-2
    again = lam.forward_argmax(batch)
    assert torch.equal(again["logits"], out["logits"])


def test_one_training_step_matches_the_reference():
    name = TP_TRAIN["case"]
    lam, case, gold_fwd, _ = model_for(name)
    gold, meta = MC.load_train_fixture(f"token_pool_{name}")
    tr, _, grads = MC.run_training_step(lam, case, gold_fwd, gold, meta, TOL, label=name)
    e_ref = float(meta["e_ref32"])
    print(f"[train {name}] gradient bound {GRAD_TOL:.0e}; the reference's own fp32-vs-fp64 error {e_ref:.3e} (x4 = {4 * e_ref:.3e})")
    # the final attention of the prompt encoder's transformer is live here: inside the active span, in front of nothing dead
    assert not any(k.startswith(FINAL) for k in meta["dead"])
    for k in meta["keys"]:
        if k.startswith(FINAL):
            assert float(grads[k].abs().max()) > 0.0, k
    assert "grad.prompt_encoder.transformer.final_attn_token_to_image.out_proj.weight" in gold
    MC.compare_gradients(tr.names, grads, gold, meta, GRAD_TOL, label=name)
