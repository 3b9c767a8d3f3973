"""What every model-option test module (tests/test_*_model_gpu.py) checks in the same way: a fixture case through the engine's argmax, HIP
graph replay, the embedding cache and one training step.  Plain functions; a module keeps its constants, its stage list and the tests of
its own feature, and calls these for the rest.  Where the modules once differed, the stricter form is the one here (profiles/model_checks.md).
"""
import json
import os

import torch
from safetensors.torch import load_file

from labelanything_amd.episodes import make_episode
from labelanything_amd.models import Lam
from tests.helpers import GOLDEN, argmax_disagreement, load_golden, make_gt, rel_err


def load_model(cases, name, prefix=""):
    """(lam, case, gold, meta) of tests/golden/<prefix><name>: the case's model on the device, reading the fixture's selected rows."""
    case = cases[name]
    gold, meta = load_golden(f"{prefix}{name}")
    lam = Lam(case["cfg"], seed=case["weight_seed"]).cuda()
    lam.selected_rows = gold.get("selected_rows")
    return lam, case, gold, meta


def load_train_fixture(stem):
    """(gold, meta) of tests/golden/<stem>_train.{safetensors,json}."""
    with open(os.path.join(GOLDEN, f"{stem}_train.json")) as fh:
        meta = json.load(fh)
    return load_file(os.path.join(GOLDEN, f"{stem}_train.safetensors")), meta


def check_argmax(name, out, gold, margin, band_share=None):
    """The fused argmax is the argmax of the logits, and differs from the reference's only inside the margin band.  ``band_share``: (the
    fixture's json, the largest share of the reference's pixels the generator may have recorded inside the band) where the json carries it."""
    note = ""
    if band_share is not None:
        meta, max_share = band_share
        assert 0 <= meta["margin_band_share"] <= max_share and meta["margin"] == margin        # the generator's figure, not ours
        note = f" ({meta['margin_band_share']:.2%} of the reference's pixels lie inside it)"
    assert torch.equal(out["logits"].argmax(dim=1).cpu(), out["argmax"].cpu())
    n_diff, n_real = argmax_disagreement(out["logits"], gold["argmax"].long(), gold["logits"], margin_rel=margin)
    print(f"[{name}] argmax differs on {n_diff} pixels, {n_real} outside the {margin:.0e} margin band{note}")
    assert n_real == 0


def check_graph_replay(lam, case, keys=("logits", "argmax")):
    """A captured graph gives the eager run's bits, on the captured inputs and on new ones, and is captured once."""
    b1 = make_episode(**case["episode"])
    b2 = make_episode(**{**case["episode"], "seed": 778})
    e1, e2 = lam.forward_argmax(b1), lam.forward_argmax(b2)
    lam.use_graphs = True
    g1 = lam.forward_argmax(b1)       # capture
    g2 = lam.forward_argmax(b2)       # replay with new inputs
    g1b = lam.forward_argmax(b1)
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(e1[k], g1[k]) and torch.equal(e2[k], g2[k]) and torch.equal(e1[k], g1b[k]), k
    assert len(lam._graphs) == 1
    assert not torch.equal(e1["logits"], e2["logits"])


def check_cached_predict(lam, case, exact=False):
    """predict from generate_class_embeddings' result, and from the test-time cache (experiment/utils.py:210-249), against the full forward:
    within 1e-6, or the same bits.  Returns (the cached embeddings, the full forward's logits) for the module's own assertions."""
    from labelanything_amd.cache import set_class_embeddings
    same = torch.equal if exact else (lambda a, b: rel_err(a, b) <= 1e-6)
    batch = make_episode(**case["episode"])
    full = lam(batch)["logits"]
    examples = {k: (v[:, 1:] if k in ("embeddings", "dims") else v) for k, v in batch.items()}
    ce = lam.generate_class_embeddings(examples)
    q = {"embeddings": batch["embeddings"][:, :1], "dims": batch["dims"][:, 0]}
    pred = lam.predict(q, ce)
    torch.cuda.synchronize()
    assert same(pred, full)
    set_class_embeddings(lam, {k: v[0] for k, v in examples.items()})
    assert same(lam.predict(q), full)
    return ce, full


def run_training_step(lam, case, gold_fwd, gold, meta, tol, label=""):
    """zero_grad, forward_backward on the case's episode and the fixture's ground truth; logits and loss against the reference's within
    ``tol``.  Returns (trainer, forward_backward's result, gradient view by name); the trainer has not applied an update."""
    from labelanything_amd.train import LamTrainer
    if "selected_rows" in gold:                                  # the training fixture was made on the forward fixture's rows
        assert torch.equal(gold["selected_rows"], gold_fwd["selected_rows"])
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=meta["seed_gt"])
    tr = LamTrainer(lam)
    tr.zero_grad()
    res = tr.forward_backward(batch, gt)
    torch.cuda.synchronize()
    assert rel_err(res["logits"], gold_fwd["logits"]) <= tol
    loss = float(res["loss"])
    print(f"[train {label}] loss {loss:.8f} reference {meta['loss']:.8f} (fp64 {meta['loss_fp64']:.8f})")
    assert abs(loss - meta["loss"]) <= tol * abs(meta["loss"])
    return tr, res, dict(zip(tr.names, tr.opt.grad_views))


def compare_gradients(names, grads, gold, meta, tol, label=""):
    """``grads`` (name -> tensor, on any device) against a ``*_train`` fixture.  The json's ``keys``, ``dead`` and ``inert`` (where it has
    one) are exactly ``names``; ``dead`` tensors, which the reference's forward never reaches either, are zero.
    Every tensor of ``keys`` by its norm: | ||g|| - ||ref|| | <= ||g - ref||, relative to the tensor's own norm floored at 1e-2 of the
    largest.  The stored tensors entry by entry, relative to the tensor's scale floored at 1e-2 of the largest stored gradient: several
    parameters have an analytically zero gradient, and the reference's value for them is rounding noise.  A tensor of ``sliced`` is stored
    as its first rows; one of ``inert`` is left to the caller's own bound."""
    keys, dead, inert = meta["keys"], meta["dead"], meta.get("inert", [])
    assert sorted(names) == sorted(keys + dead + inert)
    for k in dead:
        assert float(grads[k].abs().max()) == 0.0, k
    gn = torch.stack([grads[k].norm() for k in keys]).cpu()
    floor = 1e-2 * float(gold["grad_norm"].max())
    rel_n = (gn - gold["grad_norm"]).abs() / gold["grad_norm"].clamp_min(floor)
    at = keys[int(rel_n.argmax())]
    print(f"[train {label}] worst gradient-norm difference {float(rel_n.max()):.3e} at {at}")
    sliced = meta.get("sliced", {})
    full = {k[5:]: v for k, v in gold.items() if k.startswith("grad.") and k[5:] not in inert}
    gmax = max(float(v.abs().max()) for v in full.values())
    worst = {}
    for k, v in full.items():
        mine = grads[k].cpu()
        if k in sliced:
            mine = mine[:sliced[k]]
        assert mine.shape == v.shape, k
        worst[k] = float((mine - v).abs().max()) / max(float(v.abs().max()), 1e-2 * gmax)
    print(f"[train {label}] worst entry-wise gradient difference {max(worst.values()):.3e} at {max(worst, key=worst.get)}")
    assert float(rel_n.max()) <= tol, (at, float(rel_n.max()))
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, bad


def check_default_model_untouched(monkeypatch, lam, case, twin, wrappers, substring, message):
    """The default model (``twin()`` builds one from the option's weights) launches none of the option's ``_lib`` wrappers, has no parameter
    named ``*substring*``, and gives the same bits before and after the option's kernels (forward and backward) have run in the process."""
    from labelanything_amd import _lib
    from labelanything_amd.train import LamTrainer
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=3)
    plain = twin()

    def forbidden(*a, **kw):
        raise AssertionError(message)

    with monkeypatch.context() as mp:
        for fn in wrappers:
            mp.setattr(_lib, fn, forbidden)
        before = plain.forward_argmax(batch)
        before = {k: before[k].clone() for k in ("logits", "argmax")}
        tr = LamTrainer(twin())
        tr.zero_grad()
        tr.forward_backward(batch, gt)
        torch.cuda.synchronize()
        assert not any(substring in k for k in tr.names)
    with_option = lam.forward_argmax(batch)
    tr2 = LamTrainer(lam)
    tr2.zero_grad()
    tr2.forward_backward(batch, gt)
    after = twin().forward_argmax(batch)
    torch.cuda.synchronize()
    assert torch.equal(after["logits"], before["logits"]) and torch.equal(after["argmax"], before["argmax"])
    assert rel_err(with_option["logits"], before["logits"]) > 1e-2                # the option is not a no-op
