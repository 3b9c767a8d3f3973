"""CPU: the cosine-similarity segmenter's restatement against the reference fixtures, torch's nearest index rule, the registry entry and
the bindings of its three kernels."""
import pytest
import torch
import torch.nn.functional as F

from labelanything_amd import _lib
from tests import similarity_ref as R
from tests.cases_similarity import CASES, MARGIN, MAX_BAND_SHARE, make_inputs
from tests.helpers import load_golden
from tests.test_lib_signatures_cpu import CountingLibrary


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_gives_the_references_compare_grid_logits(name):
    gold, meta = load_golden(f"similarity_{name}")
    batch = make_inputs(CASES[name])
    assert all(torch.equal(gold[k], batch[k]) for k in batch), "the fixture's inputs are not the case's"
    assert meta["model"] == CASES[name]["model"] and meta["margin"] == MARGIN and meta["margin_band_share"] <= MAX_BAND_SHARE
    got = R.compare_logits(gold["embeddings"], gold["prompt_masks"], CASES[name]["model"]["compare_size"])
    ref = gold["compare_logits"].double()
    assert got.shape == ref.shape and bool(torch.isfinite(ref).all())
    err = float((got - ref).abs().max())
    print(f"{name}: max |restatement - reference| = {err:.3e} (bound 1e-6)")
    assert err <= 1e-6


@pytest.mark.parametrize("src", [256, 37])
@pytest.mark.parametrize("cs", [6, 9, 16, 20, 24, 128])
def test_nearest_index_rule_is_torchs(src, cs):
    ramp = torch.arange(src, dtype=torch.float32).view(1, 1, src, 1).expand(1, 1, src, src).contiguous()
    want = F.interpolate(ramp, size=(cs, cs), mode="nearest")[0, 0, :, 0].long()
    assert torch.equal(R.nearest_index(src, cs), want)


def test_class_bits_restatement_follows_the_reference_membership():
    """similarity.py:149-181 on non-binary masks: membership is ``mask != 0`` after the nearest resize, class 0 is replaced."""
    gen = torch.Generator().manual_seed(5)
    masks = torch.zeros(3, 4, 37, 37)
    masks[:, 0] = 1.0                                              # the input's class 0 is not read
    masks[:, 1:] = (torch.rand(3, 3, 37, 37, generator=gen) < 0.3).float() * 0.3
    masks[:, 2] = -masks[:, 2] / 0.3
    small = F.interpolate(masks.reshape(12, 1, 37, 37), size=(20, 20), mode="nearest").reshape(3, 4, 400)
    small[:, 0] = (small[:, 1:] != 0).sum(dim=1) == 0
    bits = R.class_bits(masks, 20)
    for c in range(4):
        assert torch.equal(((bits >> c) & 1).bool(), small[:, c] != 0), c


def test_registry_and_constructor():
    from label_anything.models import model_registry
    from label_anything.models.similarity import SimilarityFewShotSegmenter, build_similarity
    from labelanything_amd import similarity as S
    assert SimilarityFewShotSegmenter is S.SimilarityFewShotSegmenter and model_registry["similarity"] is build_similarity
    model = model_registry["similarity"](image_size=480, compare_size=128)
    assert isinstance(model, SimilarityFewShotSegmenter) and (model.image_size, model.compare_size, model.custom_preprocess) == (480, 128, False)
    assert model.encoder is None and len(model.state_dict()) == 0 and list(model.parameters()) == []
    assert build_similarity(image_size=480).compare_size is None          # similarity.py:24-26: the default is overwritten at once
    with pytest.raises(NotImplementedError, match="Only cosine"):
        build_similarity(similarity="dot")
    with pytest.raises(ValueError, match="Encoder is None"):
        model({"prompt_masks": torch.zeros(1, 1, 2, 8, 8), "dims": torch.zeros(1, 2, 2)})


def test_entry_points_are_in_the_table_and_exported():
    for name, sig in (("la_sim_prepare", "pliiips"), ("la_sim_class_bits", "piiiiips"), ("la_sim_max_plan", "iiiiiihh"),
                      ("la_sim_max", "pppiiiiipqps")):
        assert _lib.SIGNATURES[name] == sig and name in _lib.EXPORTS


def test_plan_splits_the_keys_of_a_large_episode_and_needs_no_gpu():
    assert _lib.sim_max_plan(1, 36, 36, 64, 2, ncu=256) == (1, 0)
    ks, floats = _lib.sim_max_plan(1, 16384, 16384, 768, 2, ncu=256)
    assert ks > 1 and floats == ks * 2 * 16384
    assert _lib.sim_max_plan(1, 256, 771, 384, 5, ncu=256)[0] > 1 and _lib.sim_max_plan(1, 400, 1200, 1024, 2, ncu=256)[0] > 1


def _refused(monkeypatch, error, match, fn, *args):
    fake = CountingLibrary()
    monkeypatch.setattr(_lib, "_lib", fake)
    with pytest.raises(error, match=match):
        fn(*args)
    assert fake.calls == [], "the library was entered"


def test_wrappers_refuse_before_the_library_is_entered(monkeypatch):
    f16, f32, i32 = (lambda *s: torch.zeros(*s, dtype=torch.float16)), (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    L = _lib
    # D = 96
    _refused(monkeypatch, ValueError, "multiple of 64", L.sim_max, f16(1, 4, 96), f16(1, 8, 96), i32(1, 8), 2, f32(1, 2, 4))
    _refused(monkeypatch, ValueError, "multiple of 64", L.sim_prepare, f32(1, 4, 96), 2, 2, f16(1, 4, 96))
    _refused(monkeypatch, ValueError, "multiple of 64", L.sim_max_plan, 1, 4, 8, 96, 2, 256)
    _refused(monkeypatch, ValueError, "multiple of 64", L.sim_max_plan, 1, 4, 8, 1088, 2, 256)
    # N = 33
    _refused(monkeypatch, ValueError, "N = 33", L.sim_max, f16(1, 4, 64), f16(1, 8, 64), i32(1, 8), 33, f32(1, 33, 4))
    _refused(monkeypatch, ValueError, "N = 33", L.sim_class_bits, f32(1, 33, 4, 4), 2, i32(1, 4))
    # K of the class words against K of the keys; the supports' width against the queries'
    _refused(monkeypatch, ValueError, r"bits must be .*\[1, 8\]", L.sim_max, f16(1, 4, 64), f16(1, 8, 64), i32(1, 7), 2, f32(1, 2, 4))
    _refused(monkeypatch, ValueError, "does not go with", L.sim_max, f16(1, 4, 64), f16(1, 8, 128), i32(1, 8), 2, f32(1, 2, 4))
    _refused(monkeypatch, ValueError, "out must be", L.sim_max, f16(1, 4, 64), f16(1, 8, 64), i32(1, 8), 2, f32(1, 2, 5))
    # operand types
    _refused(monkeypatch, ValueError, "fp16", L.sim_max, f32(1, 4, 64), f16(1, 8, 64), i32(1, 8), 2, f32(1, 2, 4))
    _refused(monkeypatch, ValueError, "out16 must be", L.sim_prepare, f32(1, 4, 64), 2, 3, f16(1, 4, 64))
    # host tensors of the right shapes
    _refused(monkeypatch, RuntimeError, "device tensors", L.sim_max, f16(1, 4, 64), f16(1, 8, 64), i32(1, 8), 2, f32(1, 2, 4))
    _refused(monkeypatch, RuntimeError, "device tensors", L.sim_prepare, f32(1, 4, 64), 2, 2, f16(1, 4, 64))
    _refused(monkeypatch, RuntimeError, "device tensors", L.sim_class_bits, f32(1, 3, 4, 4), 2, i32(1, 4))
