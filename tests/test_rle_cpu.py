"""CPU: run-length annotations on the host (labelanything_amd/annotations.py) - the COCO string codec, packing with the reference's
empty-mask rule, plan_prompts against the plan the REFERENCE drew (tools/make_golden_rle_episode.py ->
tests/golden/rle_episode.{json,safetensors}), and the host restatement of the rle.hip kernels (tests/rle_ref.py) against the
reference's tensors."""
import random

import numpy as np
import pytest
import torch

from labelanything_amd import annotations as A
from tests import rle_ref as R

META, GOLD = R.load_fixture()


def test_string_codec_round_trips_on_random_masks():
    rng = np.random.default_rng(0)
    for trial in range(40):
        h, w = int(rng.integers(1, 90)), int(rng.integers(1, 90))
        m = rng.random((h, w)) < rng.uniform(0.05, 0.95)
        m[0, 0] = trial % 2                                  # with and without a leading zero-length run
        rle = A.rle_from_mask(m)
        assert (rle["counts"][0] == 0) == bool(trial % 2) and sum(rle["counts"]) == h * w
        s = A.rle_to_string(rle["counts"])
        assert isinstance(s, bytes) and all(48 <= b < 112 for b in s)
        assert A.rle_from_string(s).tolist() == rle["counts"] and A.rle_from_string(s.decode("ascii")).tolist() == rle["counts"]
        assert np.array_equal(R.definition_decode(rle["counts"], h, w), m.astype(np.uint8))


def test_string_codec_worked_example_and_long_runs():
    counts = [6, 1, 40, 4, 5, 4, 5, 4, 21]
    assert A.rle_to_string(counts) == b"61X13mN000`0"
    assert A.rle_from_string("61X13mN000`0").tolist() == counts
    big = [70000, 3, 40000, 2 ** 15, 1, 2 ** 20 + 7, 33000, 5, 2 ** 15 - 1, 2 ** 15 + 1]         # counts and differences beyond 2^15
    assert A.rle_from_string(A.rle_to_string(big)).tolist() == big
    with pytest.raises(ValueError):
        A.rle_from_string(b"61X")                            # the last group announces another one


def test_rle_from_mask_is_the_column_major_definition():
    m = np.zeros((3, 4), dtype=np.uint8)
    m[1, 0] = m[2, 0] = m[0, 1] = m[2, 3] = 1
    rle = A.rle_from_mask(m)
    assert rle == {"size": [3, 4], "counts": [1, 3, 7, 1]}
    assert np.array_equal(R.definition_decode(rle["counts"], 3, 4), m)
    assert A.rle_from_mask(np.ones((2, 2)))["counts"] == [0, 4] and A.rle_from_mask(np.zeros((2, 2)))["counts"] == [4]
    assert A.as_rle({"size": [3, 4], "counts": A.rle_to_string(rle["counts"])}, 3, 4)["counts"].tolist() == [1, 3, 7, 1]
    try:
        import pycocotools  # noqa: F401
    except ImportError:
        with pytest.raises(TypeError, match="frPyObjects"):
            A.as_rle([[0.0, 0.0, 2.0, 0.0, 2.0, 2.0]], 3, 4)


def test_packing_offsets_empty_rule_and_fallback_clamp():
    a = {"size": [3, 4], "counts": [1, 3, 7, 1]}
    empty = {"size": [5, 2], "counts": [10]}
    p = A.pack_rles([a, empty, empty, empty, a], [0, 1, 1, 1, 0], [1, 2, 0, 1, 1], [(3, 4), (5, 2)], fallbacks=[None, None, (1, 3), (-4, 99), None])
    assert p.meta[:, 0].tolist() == [0, 4, 7, 10, 13] and p.meta[:, 1].tolist() == [4, 3, 3, 3, 4]
    assert p.meta[:, 2:4].tolist() == [[3, 4], [5, 2], [5, 2], [5, 2], [3, 4]]
    assert p.meta[:, 4:7].tolist() == [[0, 1, 0], [1, 2, 0], [1, 0, 1], [1, 1, 2], [0, 1, 1]]       # image, slot, order within the image
    assert p.runs.dtype == np.int32 and p.runs.tolist() == [1, 3, 7, 1] + [0, 1, 9] + [8, 1, 1] + [4, 1, 5] + [1, 3, 7, 1]
    assert p.area.tolist() == [4, 1, 1, 1, 4] and p.n_classes == 3 and p.n_images == 2
    for k, (x, y) in ((1, (0, 0)), (2, (1, 3)), (3, (0, 4))):                                      # (0, 0) | as given | clamped into 5 x 2
        m = R.definition_decode(p.runs[p.meta[k, 0]:p.meta[k, 0] + p.meta[k, 1]], 5, 2)
        assert m.sum() == 1 and m[y, x] == 1
    last = A.pack_rles([empty], [0], [0], [(5, 2)], fallbacks=[(1, 4)])                              # the last pixel: no trailing zero run
    assert last.runs.tolist() == [9, 1]


def test_packing_rejects_bad_sizes_and_sums():
    ok = {"size": [3, 4], "counts": [1, 3, 7, 1]}
    with pytest.raises(ValueError, match="mole"):
        A.pack_rles([{"size": [3, 4], "counts": [1, 3, 7]}], [0], [0], [(3, 4)], names=["mole"])
    with pytest.raises(ValueError, match="annotation 1"):
        A.pack_rles([ok, {"size": [3, 4], "counts": [5, -1, 8]}], [0, 0], [0, 0], [(3, 4)])
    with pytest.raises(ValueError, match="mole"):
        A.pack_rles([ok], [0], [0], [(4, 3)], names=["mole"])                                      # not its image's size
    with pytest.raises(ValueError, match="2\\^31"):
        A.pack_rles([], [], [], [(65536, 32768)])
    with pytest.raises(ValueError):
        A.pack_rles([ok], [1], [0], [(3, 4)])


@pytest.mark.parametrize("tag", ["custom1", "custom0"])
def test_plan_prompts_draws_the_reference_plan(tag):
    packed = R.fixture_packed(META)
    want = R.fixture_plan(META, tag, packed)
    seed = META["episodes"][tag]["seed"]
    random.seed(seed)
    np.random.seed(seed)
    got = A.plan_prompts(packed, ["bbox", "mask", "point"], max_points_annotations=META["max_points_annotations"],
                         max_points_per_annotation=META["max_points_per_annotation"], add_box_noise=True)
    assert got["types"] == want["types"] and got["draws"] == want["draws"] and got["classes"] == want["classes"]
    assert got["boxes"] == want["boxes"]                                       # same generator calls, same float64 arithmetic: exact
    many = [k for k in range(len(packed)) if packed.meta[k, 4] == 0 and packed.meta[k, 5] == 1]
    assert len(many) > META["max_points_annotations"] and all(got["types"][k] == "mask" for k in many)
    # the file's area steers the number of points, the decoded area the rank: they differ in this fixture
    assert any(abs(packed.info[k]["area"] - packed.area[k]) > 1 for k, _ in got["draws"])


@pytest.mark.parametrize("tag", ["custom1", "custom0"])
def test_restated_kernels_match_the_reference(tag):
    packed = R.fixture_packed(META)
    plan = R.fixture_plan(META, tag, packed)
    custom = META["episodes"][tag]["custom_preprocess"]
    masks, fm, pts, fp, gts = R.host_episode(packed, plan, META["side"], custom)
    want = R.unpack_bits(GOLD[f"{tag}.prompt_masks_bits"], META["episodes"][tag]["prompt_masks_shape"])
    assert np.array_equal(masks, want.astype(np.float32))
    assert np.array_equal(fm, GOLD[f"{tag}.flag_masks"].numpy())
    assert np.array_equal(fp, GOLD[f"{tag}.flag_points"].numpy())
    assert np.array_equal(pts.view(np.uint32), GOLD[f"{tag}.prompt_points"].numpy().view(np.uint32))
    assert torch.equal(torch.from_numpy(gts), R.fixture_ground_truths(META, GOLD))
    for i, (h, w) in enumerate(META["sizes"]):                               # decode: the run search against the format's definition
        ks = [k for k in range(len(packed)) if packed.meta[k, 4] == i]
        dense = np.stack([R.decode(R.scan(packed.runs[packed.meta[k, 0]:packed.meta[k, 0] + packed.meta[k, 1]])[0], h, w) for k in ks])
        if not any(packed.info[k]["area"] == 0 for k in ks):                  # the fixture stores the decode BEFORE the empty-mask rule
            assert np.array_equal(dense, R.unpack_bits(GOLD[f"decoded_bits.{i}"], dense.shape))


def test_area_of_the_scan_is_the_decoded_area():
    packed = R.fixture_packed(META)
    for k in range(len(packed)):
        ends, area = R.scan(packed.runs[packed.meta[k, 0]:packed.meta[k, 0] + packed.meta[k, 1]])
        assert area == packed.area[k] == R.decode(ends, int(packed.meta[k, 2]), int(packed.meta[k, 3])).sum() >= 1
