"""CPU: tests/model_checks.py::compare_gradients on the committed ``*_train`` fixtures, with no model and no GPU: gradients made of the
stored tensors pass, and one moved entry, one scaled norm, one nonzero dead entry or one wrongly shaped sliced tensor does not.  The floors
(1e-2 of the largest norm, 1e-2 of the largest stored entry) and the inequality are pinned at twice and at half the tolerance.
"""
import pytest
import torch

from tests.model_checks import compare_gradients, load_train_fixture

# fixture stem -> the tolerance its model test passes: max(3e-4, 4 e_kink) of the json, or 3e-4
STEMS = {"multi_embedding_e4": "kink", "levels_l2": "kink", "convcls_r1": "kink", "nodown_r1": "kink", "token_pool_tp_d64": 3e-4,
         "oneway_ow_d64": 3e-4}


def fixture(stem):
    """(names, grads, gold, meta, tol, stored): grads holds the stored tensors; for a key stored only by its norm, one element of that norm;
    zeros for the dead ones.  A sliced tensor gets one more row, whose single entry completes the stored norm."""
    gold, meta = load_train_fixture(stem)
    tol = max(3e-4, 4 * float(meta["e_kink"])) if STEMS[stem] == "kink" else STEMS[stem]
    stored = {k[5:]: v for k, v in gold.items() if k.startswith("grad.")}
    norms = dict(zip(meta["keys"], gold["grad_norm"]))
    grads = {k: torch.zeros(3) for k in meta["dead"]}
    for k in meta["keys"] + meta.get("inert", []):
        if k not in stored:
            grads[k] = norms[k].reshape(1).clone()
        elif k in meta.get("sliced", {}):
            rest = torch.zeros_like(stored[k][:1])
            rest.view(-1)[0] = (norms[k].double() ** 2 - stored[k].double().norm() ** 2).clamp_min(0).sqrt()
            grads[k] = torch.cat([stored[k], rest])
        else:
            grads[k] = stored[k].clone()
    return list(grads), grads, gold, meta, tol, stored


def scales(gold, meta, stored):
    """(floor of the norms, floor of the entries) as compare_gradients states them."""
    compared = {k: v for k, v in stored.items() if k not in meta.get("inert", [])}
    return 1e-2 * float(gold["grad_norm"].max()), 1e-2 * max(float(v.abs().max()) for v in compared.values()), compared


@pytest.mark.parametrize("stem", list(STEMS))
def test_the_stored_gradients_pass(stem):
    names, grads, gold, meta, tol, _ = fixture(stem)
    compare_gradients(names, grads, gold, meta, tol, label=stem + " cpu")
    with pytest.raises(AssertionError):
        compare_gradients(names[1:], grads, gold, meta, tol, label=stem + " cpu")          # a name the json does not account for


@pytest.mark.parametrize("stem", list(STEMS))
def test_one_moved_entry_fails_at_twice_the_tolerance_and_passes_at_half(stem):
    names, grads, gold, meta, tol, stored = fixture(stem)
    _, efloor, compared = scales(gold, meta, stored)
    for k in (min(compared, key=lambda k: float(compared[k].abs().max())), max(compared, key=lambda k: float(compared[k].abs().max()))):
        step = tol * max(float(compared[k].abs().max()), efloor)                 # the smallest tensor sits on the floor, the largest on its own scale
        moved = dict(grads)
        moved[k] = grads[k].clone()
        moved[k].view(-1)[0] += 0.5 * step
        compare_gradients(names, moved, gold, meta, tol, label=stem + " cpu")
        moved[k] = grads[k].clone()
        moved[k].view(-1)[0] += 2 * step
        with pytest.raises(AssertionError, match=k.replace(".", r"\.")):
            compare_gradients(names, moved, gold, meta, tol, label=stem + " cpu")


@pytest.mark.parametrize("stem", list(STEMS))
def test_one_scaled_norm_fails(stem):
    names, grads, gold, meta, tol, stored = fixture(stem)
    nfloor, _, _ = scales(gold, meta, stored)
    only_norm = [k for k in meta["keys"] if k not in stored]
    assert only_norm
    for k in (min(only_norm, key=lambda k: float(grads[k])), max(only_norm, key=lambda k: float(grads[k]))):
        off = dict(grads)
        off[k] = grads[k] + 2 * tol * max(float(grads[k]), nfloor)
        with pytest.raises(AssertionError, match=k.replace(".", r"\.")):
            compare_gradients(names, off, gold, meta, tol, label=stem + " cpu")


@pytest.mark.parametrize("stem", list(STEMS))
def test_one_nonzero_entry_of_a_dead_tensor_fails(stem):
    names, grads, gold, meta, tol, _ = fixture(stem)
    k = meta["dead"][-1]
    live = dict(grads)
    live[k] = torch.tensor([0.0, 1e-30, 0.0])
    with pytest.raises(AssertionError, match=k.replace(".", r"\.")):
        compare_gradients(names, live, gold, meta, tol, label=stem + " cpu")


def test_a_sliced_tensor_of_another_shape_fails():
    names, grads, gold, meta, tol, _ = fixture("convcls_r1")
    assert meta["sliced"]
    for k in meta["sliced"]:
        flat = dict(grads)
        flat[k] = grads[k].flatten()                                              # the same entries and norm; the slice is no longer rows
        with pytest.raises(AssertionError, match=k.replace(".", r"\.")):
            compare_gradients(names, flat, gold, meta, tol, label="convcls_r1 cpu")
