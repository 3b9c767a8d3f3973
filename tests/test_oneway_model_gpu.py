"""GPU: the one-way mask decoder (``fusion_transformer="OneWayTransformer"``) through the model - inference engine (la_twoway_i2t +
la_stream_mlp per layer, and the unfused chain), HIP graph replay, the embedding cache, the recipe's constructor call and one training
step - against the REFERENCE's fixtures tests/golden/oneway_* (tools/make_golden_oneway.py; cases in tests/cases_oneway.py).

Bounds, those of tests/test_token_pool_model_gpu.py: 2e-5 max-norm for decoder-only forward quantities; argmax exact outside the project's
2e-3 margin band, whose share of the reference's own pixels the generator recorded (at most 5 %, re-asserted here from the json);
gradients within 3e-4 of the tensor's scale floored at 1e-2 of the largest gradient.  The reference's own fp32-vs-fp64 gradient error
(``e_ref32`` of the fixture's json) is printed beside the measured figure.
"""
import dataclasses

import pytest
import torch

from labelanything_amd.episodes import make_episode
from labelanything_amd.models import Lam, build_lam_no_vit
from tests import model_checks as MC
from tests.cases_oneway import MARGIN, MAX_BAND_SHARE, OW_CASES, OW_TRAIN, SRC_STRIDE
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
GRAD_TOL = 3e-4
NORM3 = tuple(f"mask_decoder.transformer.layers.{l}.norm3." for l in range(2))


def model_for(name):
    return MC.load_model(OW_CASES, name, "oneway_")


def engine_with(lam, **kw):
    from labelanything_amd.engine import LamEngine
    lam.engine()            # (sets the cache key that keeps a hand-built engine in place)
    lam._engine = LamEngine(lam.cfg, lam.state_dict(), lam._device(), lam.compute_dtype, lam.decoder_dtype, lam.precise, **kw)
    return lam._engine


def forward_errors(lam, case, gold):
    """Stage by stage: class embeddings, the transformer's image output (the engine's stream buffer), low-res logits, logits."""
    batch = make_episode(**case["episode"])
    b = batch["flag_examples"].shape[0]
    g, d, st = case["cfg"].grid, case["cfg"].embed_dim, SRC_STRIDE
    seg, pe = lam._forward(batch)
    torch.cuda.synchronize()
    img = lam.engine().f32("md.img32", (b * g * g, d)).clone()           # the stream after the transformer: nothing writes it afterwards
    out = lam.forward_argmax(batch)
    torch.cuda.synchronize()
    errs = {"class_embeddings": rel_err(pe["class_embeddings"], gold["class_embeddings"]),
            "transformer_image": rel_err(img.view(b, g, g, d)[:, ::st, ::st, ::st].flatten(1, 2), gold["transformer_image_sample"]),
            "low_res_logits": rel_err(seg, gold["low_res_logits"]), "logits": rel_err(out["logits"], gold["logits"])}
    return errs, out, pe


def check_argmax(name, out, gold, meta):
    MC.check_argmax(name, out, gold, MARGIN, band_share=(meta, MAX_BAND_SHARE))


@pytest.mark.parametrize("name", list(OW_CASES))
def test_forward_matches_the_reference_fixture(name):
    """la_stream_mlp and la_twoway_i2t inside the one-way mask decoder (D = 256 cases), the unfused chain (D = 64)."""
    lam, case, gold, meta = model_for(name)
    eng = lam.engine()
    eng.ONEWAY_MLP_MIN_ROWS = 0          # (the fixtures' streams are a few hundred rows: below the default threshold)
    c = meta["classes"]
    assert eng.oneway_fused(c) == (case["cfg"].embed_dim == 256) and eng.fuse_oneway == (case["cfg"].embed_dim == 256)
    assert eng.oneway_mlp_fused(c, case["cfg"].grid ** 2) == (case["cfg"].embed_dim == 256)
    errs, out, pe = forward_errors(lam, case, gold)
    print(f"[{name}] {c} classes, fused {eng.oneway_fused(c)}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {TOL:.0e})")
    assert all(v <= TOL for v in errs.values()), errs
    check_argmax(name, out, gold, meta)


@pytest.mark.parametrize("name", ["ow_d256", "ow_masks"])
def test_fused_and_unfused_paths_agree(name):
    """la_stream_mlp: the D = 256 cases with the fused MLP forced on, with the chain MLP behind the fused attention, and with the whole
    layer on the GEMM + attention + norm chain - each against the reference, and against each other."""
    lam, case, gold, meta = model_for(name)
    c = meta["classes"]
    outs, errs = {}, {}
    for mode, kw, min_rows in (("fused", {}, 0), ("chain_mlp", {}, 1 << 40), ("chain", dict(fuse_oneway=False), 0)):
        eng = engine_with(lam, **kw)
        eng.ONEWAY_MLP_MIN_ROWS = min_rows
        rows = case["cfg"].grid ** 2
        assert eng.oneway_fused(c) == (mode != "chain") and eng.oneway_mlp_fused(c, rows) == (mode == "fused")
        errs[mode], outs[mode], _ = forward_errors(lam, case, gold)
        assert lam.engine() is eng
        assert all(v <= TOL for v in errs[mode].values()), (mode, errs[mode])
        check_argmax(f"{name} {mode}", outs[mode], gold, meta)
    between = {m: rel_err(outs[m]["logits"], outs["fused"]["logits"]) for m in ("chain_mlp", "chain")}
    print(f"[{name}] against the reference: " + ", ".join(f"{m} {max(e.values()):.2e}" for m, e in errs.items())
          + "; against the fused path: " + ", ".join(f"{m} {v:.2e}" for m, v in between.items()))
    assert all(v <= TOL for v in between.values()), between


@pytest.mark.parametrize("decoder_dtype,bound", [("f16x2", TOL), (None, 1e-2)])
def test_chain_on_the_other_decoder_operand_types(decoder_dtype, bound):
    """The unfused chain with the image-side operands as fp16 plane pairs ("f16x2": fp32-class, the forward bound) and with a 16-bit
    decoder (None = the encoder's fp16: every GEMM operand carries 11 bits, 5e-4 a rounding, and a logit sits behind a few dozen of
    them - 1e-2 of the logit scale is the class, an order above what fp16 operands give elsewhere in the project), against the fixture."""
    lam, case, gold, meta = model_for("ow_d256")
    lam.decoder_dtype = decoder_dtype
    eng = engine_with(lam, fuse_oneway=False)
    assert not eng.oneway_fused(meta["classes"]) and eng.isplit == (decoder_dtype == "f16x2")
    errs, out, _ = forward_errors(lam, case, gold)
    assert lam.engine() is eng
    print(f"[ow_d256 decoder_dtype={decoder_dtype}] " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {bound:.0e})")
    assert all(v <= bound for v in errs.values()), errs


def test_more_than_32_classes_take_the_chain():
    lam, case, _, _ = model_for("ow_d256")
    eng = lam.engine()
    assert eng.oneway_fused(32) and not eng.oneway_fused(33) and not eng.oneway_mlp_fused(33, 1 << 20)
    assert eng.oneway_mlp_fused(3, eng.ONEWAY_MLP_MIN_ROWS) and not eng.oneway_mlp_fused(3, eng.ONEWAY_MLP_MIN_ROWS - 1)
    assert not engine_with(lam, fuse_twoway=False).oneway_fused(3)


@pytest.mark.parametrize("name", ["ow_d256", "ow_d64"])
def test_graph_replay_is_bit_identical_and_tracks_new_inputs(name):
    lam, case, _, _ = model_for(name)
    MC.check_graph_replay(lam, case)


@pytest.mark.parametrize("name", ["ow_d256", "ow_masks"])
def test_predict_from_cached_class_embeddings_matches_forward(name):
    lam, case, gold, _ = model_for(name)
    ce, _ = MC.check_cached_predict(lam, case)
    assert rel_err(ce["class_embeddings"], gold["class_embeddings"]) <= TOL


def test_classes_without_a_valid_support_are_treated_as_in_the_plain_model():
    """A class no support shows (flag_examples all zero) and a class the ground truth does not hold (flag_gts, whose planes are -inf):
    the finite / -inf pattern is the two-way model's on the same episode, and the argmax never picks a -inf plane."""
    lam, case, _, _ = model_for("ow_d256")
    batch = make_episode(**case["episode"])
    batch["flag_examples"] = batch["flag_examples"].clone()
    batch["flag_examples"][:, :, 2] = 0
    batch["flag_gts"] = batch["flag_gts"].clone()
    batch["flag_gts"][:, 1] = False
    plain = Lam(dataclasses.replace(case["cfg"], fusion_transformer="TwoWayTransformer"), seed=case["weight_seed"]).cuda()
    plain.selected_rows = lam.selected_rows
    out, ref = lam.forward_argmax(batch), plain.forward_argmax(batch)
    torch.cuda.synchronize()
    assert torch.equal(torch.isfinite(out["logits"]), torch.isfinite(ref["logits"]))
    assert bool(torch.isinf(out["logits"][:, 1]).all()) and bool((out["logits"][:, 1] < 0).all()) and bool(torch.isfinite(out["logits"][:, 0]).all())
    assert int((out["argmax"] == 1).sum()) == 0 and not bool(torch.isnan(out["logits"]).any())


def test_the_recipe_builds_loads_and_runs_and_is_not_the_two_way_decoder():
    """The model section of parameters/trainval/Ablations/mae_transformer.yaml: 480 px, 768-channel precomputed embeddings behind the neck,
    D = 256, 30 x 30 grid (900 stream rows an episode: la_stream_mlp with a 4-row tail), no class encoder, mask prompts.  A seeded state
    dict strict-loads; one small episode runs; a two-way model on the same episode gives other logits, so the switch is not a no-op."""
    kw = dict(spatial_convs=3, class_attention=False, example_attention=False, example_class_attention=False,
              image_embed_dim=768, embed_dim=256, image_size=480)
    lam = build_lam_no_vit(fusion_transformer="OneWayTransformer", seed=5, **kw).cuda()
    donor = build_lam_no_vit(fusion_transformer="OneWayTransformer", seed=6, **kw)
    res = lam.load_state_dict(donor.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys and lam.cfg.grid == 30 and lam.cfg.one_way
    two = build_lam_no_vit(fusion_transformer="TwoWayTransformer", seed=6, **kw).cuda()
    batch = make_episode(batch=1, n_ways=2, k_shots=1, image_size=480, seed=31, prompts=("mask",), embeddings_channels=768, grid=30,
                         dims=[[480, 360]] * 3)
    lam.engine().ONEWAY_MLP_MIN_ROWS = 0          # (one episode is below the default threshold: the fused MLP is what this test runs)
    assert lam.engine().oneway_mlp_fused(3, 900)
    out, ref = lam.forward_argmax(batch), two.forward_argmax(batch)
    torch.cuda.synchronize()
    assert tuple(out["logits"].shape) == (1, 3, 480, 360) and bool(torch.isfinite(out["logits"]).all())
    assert rel_err(out["logits"], ref["logits"]) > 1e-2
    again = lam.forward_argmax(batch)
    assert torch.equal(again["logits"], out["logits"])


def test_one_training_step_matches_the_reference():
    name = OW_TRAIN["case"]
    lam, case, gold_fwd, _ = model_for(name)
    gold, meta = MC.load_train_fixture(f"oneway_{name}")
    lin1 = "mask_decoder.transformer.layers.1.mlp.lin1.weight"
    before = {k: p.detach().clone() for k, p in lam.named_parameters() if k.startswith(NORM3) or k == lin1}
    tr, _, grads = MC.run_training_step(lam, case, gold_fwd, gold, meta, TOL, label=name)
    # norm3 sits in the dead tail of the flat buffer, with the plain prompt encoder's final attention
    tail = [k for k in tr.names if k.startswith(NORM3)]
    assert len(tail) == 4 and tr.names.index(tail[0]) > tr.names.index("mask_decoder.class_mlp.layers.2.bias")
    e_ref = float(meta["e_ref32"])
    print(f"[train {name}] gradient bound {GRAD_TOL:.0e}; the reference's own fp32-vs-fp64 error {e_ref:.3e} (x4 = {4 * e_ref:.3e})")
    assert all(any(k.startswith(p) for k in meta["dead"]) for p in NORM3)
    assert "grad." + lin1 in gold
    MC.compare_gradients(tr.names, grads, gold, meta, GRAD_TOL, label=name)
    # an optimizer step leaves norm3 where it was: no gradient, and the trainer skips tensors that never received one
    tr.apply_update()
    torch.cuda.synchronize()
    after = dict(lam.named_parameters())
    assert all(torch.equal(after[k].detach(), v) for k, v in before.items() if k != lin1)
    assert not torch.equal(after[lin1].detach(), before[lin1])
