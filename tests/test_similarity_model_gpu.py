"""GPU: the cosine-similarity segmenter against the reference's fixtures (tests/golden/similarity_*), its image path, the empty-class rule
and the refusal of a batch it cannot embed."""
import pytest
import torch

from labelanything_amd.models import ImageEncoder
from labelanything_amd.similarity import build_similarity
from tests import similarity_ref as R
from tests.cases_similarity import CASES, MARGIN, MAX_BAND_SHARE
from tests.helpers import argmax_disagreement, load_golden, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-3                  # the project's stage bound (README): max|a - b| / max|b|


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_matches_the_reference_fixture(name):
    """la_sim_prepare, la_sim_class_bits and la_sim_max inside the model: compare-grid logits and final logits within the stage bound,
    argmax equal wherever the reference's top-2 gap exceeds MARGIN of its largest logit."""
    gold, meta = load_golden(f"similarity_{name}")
    assert meta["margin"] == MARGIN and meta["margin_band_share"] <= MAX_BAND_SHARE
    model = build_similarity(**CASES[name]["model"])
    batch = {k: gold[k] for k in ("embeddings", "prompt_masks", "dims")}
    low = model.compare_logits(batch)
    out = model(batch)["logits"]
    torch.cuda.synchronize()
    assert low.is_cuda and out.is_cuda and low.shape == gold["compare_logits"].shape and out.shape == gold["logits"].shape
    e_low, e_out = rel_err(low, gold["compare_logits"]), rel_err(out, gold["logits"])
    n_diff, n_clear = argmax_disagreement(out, gold["argmax"], gold["logits"], MARGIN)
    print(f"{name}: compare-grid rel err {e_low:.3e}, final {e_out:.3e} (bound {TOL:.0e}); argmax differs on {n_diff} pixels, "
          f"{n_clear} outside the margin band")
    assert e_low <= TOL and e_out <= TOL
    assert n_clear == 0


def test_images_path_equals_the_embeddings_path_bit_for_bit():
    import tests.cases_dinov3  # noqa: F401  (registers dinov3_tiny)
    enc = ImageEncoder("dinov3_tiny", image_size=64, seed=31).cuda()
    gen = torch.Generator().manual_seed(77)
    images = torch.randn(1, 3, 3, 64, 64, generator=gen)
    masks = torch.zeros(1, 2, 2, 16, 16)
    masks[0, 0, 1, 2:9, 3:12] = 1.0
    masks[0, 1, 1, 8:14, 1:7] = 1.0
    dims = torch.tensor([[[50, 64], [64, 64], [64, 64]]])
    kw = dict(image_size=64, compare_size=8, custom_preprocess=True)
    via_images = build_similarity(encoder=enc, **kw)({"images": images.cuda(), "prompt_masks": masks, "dims": dims})["logits"]
    emb = enc(images.flatten(0, 1).cuda())
    assert tuple(emb.shape) == (3, 128, 4, 4)
    via_emb = build_similarity(**kw)({"embeddings": emb.view(1, 3, 128, 4, 4), "prompt_masks": masks, "dims": dims})["logits"]
    torch.cuda.synchronize()
    assert tuple(via_images.shape) == (1, 2, 64, 64) and bool(torch.isfinite(via_images[:, :, :50]).all())
    assert torch.equal(via_images, via_emb)


def test_a_class_without_a_support_pixel_is_minus_inf_everywhere():
    """The documented deviation: la_sim_max writes -inf, the model resamples a zero channel in its place and passes
    "has a support pixel" as la_post_final's flag - no NaN, and the other channels are what they are without the empty class."""
    gold, _ = load_golden("similarity_b2_cs16")
    model = build_similarity(**CASES["b2_cs16"]["model"])
    masks = gold["prompt_masks"].clone()
    masks[1, :, 2] = 0.0                                      # episode 1: class 2 has no support pixel
    batch = {"embeddings": gold["embeddings"], "prompt_masks": masks, "dims": gold["dims"]}
    low = model.compare_logits(batch).cpu()
    out = model(batch)["logits"].cpu()
    assert bool((low[1, 2] == float("-inf")).all()) and bool(torch.isfinite(low[0]).all()) and bool(torch.isfinite(low[1, :2]).all())
    assert not bool(torch.isnan(out).any())
    assert bool((out[1, 2] == float("-inf")).all()) and not bool((out.argmax(dim=1)[1] == 2).any())
    want = R.compare_logits(gold["embeddings"], masks, 16)
    assert rel_err(low[1, :2], want[1, :2]) <= TOL and rel_err(low[0], want[0]) <= TOL
    h, w = (int(v) for v in gold["dims"][1, 0])
    assert bool(torch.isfinite(out[1, :2, :h, :w]).all()) and bool(torch.isfinite(out[0, :, :50, :70]).all())


def test_a_batch_with_neither_embeddings_nor_an_encoder_is_refused():
    model = build_similarity(image_size=64, compare_size=8)
    with pytest.raises(ValueError, match="Encoder is None, but no embeddings provided in batch."):
        model({"images": torch.zeros(1, 2, 3, 64, 64), "prompt_masks": torch.zeros(1, 1, 2, 16, 16), "dims": torch.zeros(1, 2, 2)})


def test_registry_model_runs_a_recipe_shaped_episode():
    """parameters/validation/COCO/cosine.yaml: image_size 480, compare_size 128 on 30 x 30 DINOv3 embeddings (width cut to 128 here)."""
    from label_anything.models import model_registry
    model = model_registry["similarity"](image_size=480, compare_size=128)
    gen = torch.Generator().manual_seed(3)
    masks = torch.zeros(1, 1, 2, 256, 256)
    masks[0, 0, 1, 40:200, 60:180] = 1.0
    batch = {"embeddings": torch.randn(1, 2, 128, 30, 30, generator=gen), "prompt_masks": masks, "dims": torch.tensor([[[375, 500], [480, 480]]])}
    out = model(batch)["logits"]
    low = model.compare_logits(batch).cpu()
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, 2, 480, 500) and bool(torch.isfinite(out[:, :, :375]).all())
    # fp64 on every 61st query pixel (all of them would be a 2 GiB score matrix - the very thing the kernel avoids)
    rows = R.prepare(batch["embeddings"].flatten(0, 1), 128)
    sel = torch.arange(0, 128 * 128, 61)
    want = R.masked_max(rows[:1, sel], rows[1:], R.class_bits(masks.view(1, 2, 256, 256), 128), 2)
    assert rel_err(low.view(1, 2, -1)[:, :, sel], want) <= TOL
