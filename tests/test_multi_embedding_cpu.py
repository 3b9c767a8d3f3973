"""CPU: configuration surface of the per-example family (``segment_example_logits`` / ``embeddings_per_example``) and the torch
restatement of its three changed steps (tests/multi_embedding_ref.py) against the reference's fixtures
(tests/golden/multi_embedding_*, tools/make_golden_multi_embedding.py)."""
import json
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

from labelanything_amd.config import LamConfig, config_from_kwargs, resolve_examples
from labelanything_amd.weights import init_state_dict, model_shapes
from tests import multi_embedding_ref as R
from tests.cases_multi_embedding import ME_CASES
from tests.helpers import load_golden

SMALL = dict(image_size=64, embed_dim=64, image_embed_dim=64)


def test_resolution_follows_the_reference_builder():
    """build_lam.py:145-148: the flag alone -> 1 embedding per example; a truthy count turns the flag on; 0 / None leave it off."""
    assert resolve_examples(False, None) == (False, None)
    assert resolve_examples(True, None) == (True, 1)
    assert resolve_examples(False, 4) == (True, 4)
    assert resolve_examples(True, 9) == (True, 9)
    assert resolve_examples(False, 0) == (False, 0)
    cfg = config_from_kwargs(encoder=None, use_vit=False, segment_example_logits=True, **SMALL)
    assert (cfg.segment_example_logits, cfg.embeddings_per_example, cfg.pool_side) == (True, 1, 1)
    cfg = config_from_kwargs(encoder=None, use_vit=False, embeddings_per_example=4, **SMALL)
    assert (cfg.segment_example_logits, cfg.embeddings_per_example, cfg.pool_side) == (True, 4, 2)
    cfg = config_from_kwargs(encoder=None, use_vit=False, **SMALL)
    assert (cfg.segment_example_logits, cfg.embeddings_per_example, cfg.pool_side) == (False, None, 1)
    assert LamConfig().segment_example_logits is False and LamConfig().embeddings_per_example is None


@pytest.mark.parametrize("epe,k", [(1, 1), (2, 1), (3, 1), (4, 2), (5, 2), (8, 2), (9, 3), (15, 3), (16, 4)])
def test_pool_side_is_floor_sqrt(epe, k):
    """prompt_encoder.py:727: int(sqrt(embeddings_per_example)) - 5 gives 2 x 2."""
    assert config_from_kwargs(encoder=None, use_vit=False, embeddings_per_example=epe, **SMALL).pool_side == k
    assert R.pool_side(epe) == k
    assert int(torch.sqrt(torch.tensor(epe))) == k


def test_more_bins_than_grid_positions_is_refused():
    with pytest.raises(ValueError, match="grid"):
        config_from_kwargs(encoder=None, use_vit=False, embeddings_per_example=25, **SMALL)      # 5 x 5 bins from a 4 x 4 grid


def test_public_constructors():
    """LabelAnything takes segment_example_logits only (build_lam.py:470-498); the build_lam functions and Lam take both."""
    from labelanything_amd.models import LabelAnything, Lam, build_lam, build_lam_no_vit
    with pytest.raises(TypeError):
        LabelAnything(encoder=None, use_vit=False, embeddings_per_example=4, **SMALL)
    m = LabelAnything(encoder=None, use_vit=False, segment_example_logits=True, **SMALL)
    assert m.model.cfg.segment_example_logits and m.model.cfg.embeddings_per_example == 1
    lam = build_lam_no_vit(embeddings_per_example=4, **SMALL)
    assert lam.cfg.segment_example_logits and lam.cfg.pool_side == 2
    lam = build_lam(encoder=None, use_vit=False, segment_example_logits=True, embeddings_per_example=9, image_size=128, embed_dim=64,
                    image_embed_dim=64)
    assert lam.cfg.pool_side == 3
    base = config_from_kwargs(encoder=None, use_vit=False, **SMALL)
    lam = Lam(base, embeddings_per_example=5)
    assert lam.cfg.segment_example_logits and lam.cfg.pool_side == 2 and base.embeddings_per_example is None
    assert Lam(base, segment_example_logits=True).cfg.embeddings_per_example == 1
    assert Lam(base).cfg == base
    # the re-exported surface of the reference's package name
    from label_anything.models import build_lam_no_vit as shim
    assert shim(embeddings_per_example=4, **SMALL).cfg.pool_side == 2


@pytest.mark.parametrize("kw", [dict(embedding_extraction="GuidedPooler"), dict(prompt_encoder="TokenPool"), dict(conv_classification=True),
                                dict(classification_levels=2), dict(few_type="Affinity"), dict(fusion_transformer="OneWayTransformer")])
def test_out_of_scope_switches_still_raise(kw):
    with pytest.raises(NotImplementedError):
        config_from_kwargs(encoder=None, use_vit=False, embeddings_per_example=4, **SMALL, **kw)


def test_no_parameter_is_added():
    """The state dict is key-for-key (and shape-for-shape) that of the one-prototype model."""
    for case in ME_CASES.values():
        cfg = case["cfg"]
        import dataclasses
        plain = dataclasses.replace(cfg, segment_example_logits=False, embeddings_per_example=None)
        assert model_shapes(cfg) == model_shapes(plain)
        a, b = init_state_dict(cfg, 5), init_state_dict(plain, 5)
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_config_json_round_trip():
    from labelanything_amd.models import LabelAnything, build_lam
    m = LabelAnything(encoder=None, use_vit=False, segment_example_logits=True, **SMALL)
    with tempfile.TemporaryDirectory() as d:
        m.save_local(d)
        with open(os.path.join(d, "config.json")) as fh:
            assert json.load(fh)["segment_example_logits"] is True
        m2 = LabelAnything.from_local(d)
        assert m2.model.cfg == m.model.cfg and m2.config == m.config
    with tempfile.TemporaryDirectory() as d:
        m.save_pretrained(d)
        m3 = LabelAnything.from_pretrained(d)
        assert m3.model.cfg.segment_example_logits and m3.model.cfg.embeddings_per_example == 1
    # the builder's keyword set (what a parameters/*.yaml model section holds) through json: both arguments survive
    kw = dict(encoder=None, use_vit=False, embeddings_per_example=4, segment_example_logits=False, **SMALL)
    lam = build_lam(**json.loads(json.dumps(kw)))
    assert lam.cfg.segment_example_logits and lam.cfg.embeddings_per_example == 4
    import dataclasses
    again = config_from_kwargs(**json.loads(json.dumps(dataclasses.asdict(lam.cfg))))
    assert again == lam.cfg


def test_trainer_refuses_prompt_contrastive_with_region_embeddings():
    from labelanything_amd.loss import LabelAnythingLoss
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    lam = Lam(config_from_kwargs(encoder=None, use_vit=False, embeddings_per_example=4, **SMALL))
    with pytest.raises(NotImplementedError, match="prompt_contrastive"):
        LamTrainer(lam, loss=LabelAnythingLoss({"focal": {"weight": 1.0}, "prompt_contrastive": {"weight": 0.1}}))


# ---- the torch restatement against the reference's fixtures ---------------------------------------------------------------------
@pytest.mark.parametrize("g,k", [(16, 3), (5, 2), (30, 2), (4, 4), (16, 1), (7, 7)])
def test_bins_are_adaptive_avg_pool_bins(g, k):
    """The bin rule that la_region_mean documents is torch's: pooling an index ramp returns each bin's mean position."""
    ramp = torch.arange(g, dtype=torch.float64).view(1, 1, g)
    got = F.adaptive_avg_pool1d(ramp, k).flatten()
    want = torch.tensor([(lo + hi - 1) / 2 for lo, hi in R.bins(g, k)], dtype=torch.float64)
    assert torch.equal(got, want)
    assert all(hi > lo for lo, hi in R.bins(g, k))
    cover = torch.zeros(g)
    for lo, hi in R.bins(g, k):
        cover[lo:hi] += 1
    assert bool((cover >= 1).all()) and bool((cover <= 2).all())          # a position lies in one bin, or in two neighbours


def test_pool_layout_is_m_h_w_major():
    """out[b, m k k + i k + j, c] = mean of slab (b m c) over bin (i, j)."""
    b, m, c, g, k, d = 2, 2, 3, 5, 2, 4
    src = torch.randn(b * m * c, g * g, d, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    out = R.pool_examples(src, b, m, c, g, k)
    assert tuple(out.shape) == (b, m * k * k, c, d)
    by = R.bins(g, k)
    for bi in range(b):
        for mi in range(m):
            for ci in range(c):
                slab = src[(bi * m + mi) * c + ci].view(g, g, d)
                for i, (y0, y1) in enumerate(by):
                    for j, (x0, x1) in enumerate(by):
                        want = slab[y0:y1, x0:x1].reshape(-1, d).mean(dim=0)
                        assert torch.allclose(out[bi, mi * k * k + i * k + j, ci], want, atol=1e-14)


@pytest.mark.parametrize("name", list(ME_CASES))
def test_restatement_reproduces_the_fixtures(name):
    """Repeated flags and the (B, M k k, C, D) layout as the reference returns them, and low_res_logits = the masked maximum over the
    examples of the stored class_mlp output against the stored (strided) upscaled features, to 2e-5 of the logit scale."""
    from labelanything_amd.episodes import make_episode
    case = ME_CASES[name]
    gold, meta = load_golden(f"multi_embedding_{name}")
    batch = make_episode(**case["episode"])
    k = case["cfg"].pool_side
    b, m, c = batch["flag_examples"].shape
    assert meta["pool_side"] == k and meta["examples"] == m * k * k
    flags = R.repeat_flags(batch["flag_examples"], k)
    assert torch.equal(flags, gold["flag_examples"])
    assert tuple(gold["class_examples_embeddings"].shape) == (b, m * k * k, c, case["cfg"].embed_dim)
    if not (case["cfg"].class_attention or case["cfg"].example_attention or case["cfg"].example_class_attention):
        # no merge block: every bin of one (support, class) slab is a mean of the same rows, so the k k examples of a support are
        # distinct vectors laid out support-major - the m-th block of k k examples differs from the next one
        e = gold["class_examples_embeddings"].view(b, m, k * k, c, -1)
        assert float((e[:, 0] - e[:, 1]).abs().max()) > 0
    s = meta["feature_stride"]
    feat = gold["features_s2"]                                           # [b, f, h / s, w / s]
    cf = feat.shape[1]
    protos = gold["protos"].view(b, m * k * k, c, cf)
    seg, _ = R.classify_max(protos.double(), feat.flatten(2).transpose(1, 2).double(), flags)
    want = gold["low_res_logits"][:, :, ::s, ::s].flatten(2).double()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isfinite(seg), fin)
    err = float((seg[fin] - want[fin]).abs().max() / want[fin].abs().max())
    print(f"{name}: restated low_res_logits rel err {err:.3e}")
    assert err <= 2e-5
