"""Query substitution bookkeeping against the reference (tests/golden/substitution.*, tools/make_golden_substitution.py): the step
sequence, the rotations of tensor and list keys and the query / support split of ``Substitutor`` run on CPU tensors with
num_points=0, so no kernel is involved.  Cases recorded with num_points > 0 are compared on every key the error points do not touch,
and on the points / flags the batch started with."""
import json
import os

import pytest
import torch
from safetensors.torch import load_file

from labelanything_amd.substitution import Substitutor

GOLD = os.path.join(os.path.dirname(__file__), "golden", "substitution")
META = json.load(open(GOLD + ".json"))["cases"]
T = load_file(GOLD + ".safetensors")
BATCH_KEYS = ["embeddings", "prompt_points", "flag_points", "prompt_bboxes", "flag_bboxes", "prompt_masks", "flag_masks",
              "flag_examples", "dims"]


def dataset_batch(name):
    cfg = META[name]
    batch = {k: T[f"{name}.in.{k}"].clone() for k in BATCH_KEYS}
    m1, bsz = cfg["M1"], cfg["B"]
    # the list keys as the generator built them (their per-step values are in the fixture's json)
    step0 = cfg["steps"][0]
    batch["classes"] = [list(x) for x in step0["classes"]]
    batch["image_ids"] = [[100 * b + m for m in range(m1)] for b in range(bsz)]
    batch["intended_classes"] = step0["intended_classes"]
    return batch, T[f"{name}.in.gts"].clone()


@pytest.mark.parametrize("name", sorted(META))
def test_steps_match_reference(name):
    cfg = META[name]
    sub = Substitutor(num_points=0, substitute=cfg["sub"])
    sub.reset(batch=dataset_batch(name))
    steps = list(sub)
    assert len(steps) == len(cfg["steps"]) == (cfg["M1"] + 1 if cfg["sub"] else 1)
    assert sub.num_steps == len(steps)
    grown = cfg["n"] > 0 and cfg["sub"]
    for i, (inp, gt) in enumerate(steps):
        pre = f"{name}.step{i}."
        assert torch.equal(gt, T[pre + "gt"]), (name, i)
        want = {k[len(pre):] for k in T if k.startswith(pre)} - {"gt", "logits", "ranks", "new_points", "new_labels"}
        assert set(k for k, v in inp.items() if isinstance(v, torch.Tensor)) == want
        for k in want:
            ref = T[pre + k]
            got = inp[k]
            if grown and k in ("prompt_points", "flag_points"):
                ref = ref[:, :, :, :got.shape[3]]          # the reference's batch carries the error points appended since step 0
            assert got.dtype == ref.dtype and torch.equal(got, ref), (name, i, k)
        lists = cfg["steps"][i]
        for k in ("classes", "image_ids", "intended_classes"):
            assert inp[k] == lists[k], (name, i, k)


def test_images_key_is_rotated_like_embeddings():
    batch, gts = dataset_batch("b2_m6_c6_n0")
    batch["images"] = batch.pop("embeddings")
    sub = Substitutor(num_points=0)
    sub.reset(batch=(batch, gts))
    for i, (inp, _) in enumerate(sub):
        assert torch.equal(inp["images"], T[f"b2_m6_c6_n0.step{i}.embeddings"])


def test_final_support_order_differs_for_six_images():
    # the rotations compose (each index tensor is applied to the already rotated batch): the supports do not come back in order
    batch, gts = dataset_batch("b2_m6_c6_n0")
    sub = Substitutor(num_points=0)
    sub.reset(batch=(batch, gts))
    *_, (last, _) = list(sub)
    assert last["image_ids"][0][0] == 0 and last["image_ids"][0] != list(range(6))


def test_threshold_not_built():
    with pytest.raises(NotImplementedError):
        Substitutor(threshold=0.5)


def test_reference_import_path():
    from label_anything.experiment.substitution import Substitutor as S, generate_points_from_errors as G
    from labelanything_amd import substitution
    assert S is substitution.Substitutor and G is substitution.generate_points_from_errors


def test_sampler_refuses_cpu_tensors():
    from labelanything_amd.substitution import generate_points_from_errors
    with pytest.raises(RuntimeError):
        generate_points_from_errors(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long), 1)
