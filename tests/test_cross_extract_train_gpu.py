"""GPU: training ``embedding_extraction="cross_attention"`` - the extraction graph alone against autograd through the fp64 restatement
(tests/cross_extract_ref.py), and ``LamTrainer(lam, embedding_dropout=...)`` against the REFERENCE's train-mode step
(tests/golden/cross_extract_<case>_train*; tools/make_golden_cross_extract_train.py; cases in tests/cases_cross_extract_train.py).

Bounds, as in the other model-option modules: 2e-5 max-norm for decoder-only forward quantities, GRAD_TOL = 3e-4 for gradients in the
units of tests.model_checks.compare_gradients (a tensor's norm against its own floored at 1e-2 of the largest; entries against the tensor's
scale floored at 1e-2 of the largest gradient); the generator refuses a fixture whose reference fp32-vs-fp64 error, times four, exceeds it.
"""
import os

import pytest
import torch
from safetensors.torch import load_file

from labelanything_amd.episodes import make_episode
from tests import cross_extract_ref as R
from tests import model_checks as MC
from tests.cases_cross_extract import XE_CASES
from tests.cases_cross_extract_train import EX, XE_TRAIN
from tests.helpers import GOLDEN, make_gt, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-5
GRAD_TOL = 3e-4
NORM3 = sorted(f"{EX}layers.{l}.norm3.{p}" for l in range(2) for p in ("weight", "bias"))
TRAIN_IDS = [s["case"] for s in XE_TRAIN]


def model_for(name):
    return MC.load_model(XE_CASES, name, "cross_extract_")


def train_fixture(name):
    """(gold, meta, gold_fwd): the training fixture and, in the place of the eval fixture, the train-mode logits (a query is dropped)."""
    gold, meta = MC.load_train_fixture(f"cross_extract_{name}")
    logits = load_file(os.path.join(GOLDEN, f"cross_extract_{name}_train_logits.safetensors"))["logits"]
    return gold, meta, {"logits": logits, "selected_rows": gold["selected_rows"]}


def run_training_step(lam, case, gold_fwd, gold, meta, tol, label="", **trainer_kw):
    """tests.model_checks.run_training_step with the trainer's keyword arguments (that one builds ``LamTrainer(lam)`` itself)."""
    from labelanything_amd.train import LamTrainer
    assert torch.equal(gold["selected_rows"], gold_fwd["selected_rows"])
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=meta["seed_gt"])
    tr = LamTrainer(lam, **trainer_kw)
    tr.zero_grad()
    res = tr.forward_backward(batch, gt)
    torch.cuda.synchronize()
    assert rel_err(res["logits"], gold_fwd["logits"]) <= tol
    loss = float(res["loss"])
    print(f"[train {label}] loss {loss:.8f} reference {meta['loss']:.8f} (fp64 {meta['loss_fp64']:.8f})")
    assert abs(loss - meta["loss"]) <= tol * abs(meta["loss"])
    return tr, res, dict(zip(tr.names, tr.opt.grad_views))


# (x1 has one query: there is no mixed mask)
@pytest.mark.parametrize("name,keep_kind", [(k, kind) for k in XE_CASES for kind in ("all", "mixed")
                                            if kind == "all" or int(XE_CASES[k]["cfg"].embeddings_per_example) > 1])
def test_module_gradients_against_the_float64_restatement(name, keep_kind):
    """The two-layer extraction graph alone (la_extract_fold / la_extract_pool_lse / la_extract_unfold and their backwards
    la_extract_fold_bwd / la_extract_pool_bwd / la_extract_unfold_bwd under the autograd nodes, layer 0 in the broadcast form) on the
    fixture's subsampled stream: the gradients of the stream and of the 33 live tensors against autograd through the fp64 restatement,
    for the objective sum(emb * weights) with the dropped queries' weights zero.  Bound: GRAD_TOL in compare_gradients' units."""
    from labelanything_amd.train import DecoderGraph
    lam, case, _, _ = model_for(name)
    ops = load_file(os.path.join(GOLDEN, f"cross_extract_{name}_stream.safetensors"))
    b, m, c = ops["flag_examples_in"].shape
    stream = ops["stream"]
    p, hw, d = stream.shape
    n = int(case["cfg"].embeddings_per_example)
    keep = torch.ones(n, dtype=torch.bool)
    if keep_kind == "mixed":
        keep[n // 2:] = False
    weights = torch.randn(b, n, c, d, generator=torch.Generator().manual_seed(7)) * keep.view(1, n, 1, 1)
    names = [k for k, _ in lam.named_parameters() if k.startswith(EX)]
    assert len(names) == 37
    params = dict(lam.named_parameters())
    for k in names:
        params[k].requires_grad_(True)
    xs = stream.reshape(p * hw, d).cuda().requires_grad_(True)
    graph = DecoderGraph(lam)
    emb = graph.extract_embeddings(xs, b, m, c, hw)
    (emb * weights.cuda()).sum().backward()
    torch.cuda.synchronize()
    # fp64 on the CPU from the same fp32 values
    w64 = {k: v.detach().double().cpu().requires_grad_(k in names) for k, v in lam.state_dict().items() if k.startswith(EX)}
    x64 = stream.double().requires_grad_(True)
    ref_emb = R.extract(x64, b, m, c, w64, "folded")
    assert rel_err(emb, ref_emb) <= TOL
    live = [k for k in names if k not in NORM3]
    # (the folded restatement never reads k_proj.bias, which cancels in the softmax: its gradient is the exact zero)
    ref = torch.autograd.grad((ref_emb * weights.double()).sum(), [x64] + [w64[k] for k in live], allow_unused=True)
    assert [k for k, g in zip(live, ref[1:]) if g is None] == [f"{EX}layers.{l}.cross_attn_image_to_token.k_proj.bias" for l in range(2)]
    ref = [torch.zeros_like(t) if g is None else g for g, t in zip(ref, [x64] + [w64[k] for k in live])]
    got = {"stream": xs.grad.view(p, hw, d).cpu(), **{k: params[k].grad.cpu() for k in live}}
    want = {"stream": ref[0], **dict(zip(live, ref[1:]))}
    assert all(params[k].grad is None or float(params[k].grad.abs().max()) == 0.0 for k in NORM3)
    nmax = max(float(v.norm()) for v in want.values())
    gmax = max(float(v.abs().max()) for v in want.values())
    worst_n, worst_e = {}, {}
    for k, v in want.items():
        g = got[k].double()
        worst_n[k] = abs(float(g.norm()) - float(v.norm())) / max(float(v.norm()), 1e-2 * nmax)
        worst_e[k] = float((g - v).abs().max()) / max(float(v.abs().max()), 1e-2 * gmax)
    kn, ke = max(worst_n, key=worst_n.get), max(worst_e, key=worst_e.get)
    print(f"[module {name} keep {keep.tolist()}] worst norm difference {worst_n[kn]:.3e} at {kn}; worst entry-wise {worst_e[ke]:.3e} at {ke}; "
          f"stream {worst_e['stream']:.3e} (bound {GRAD_TOL:.0e})")
    for l in range(2):                     # the key bias cancels in the softmax: la_extract_fold_bwd writes an exact zero
        assert float(got[f"{EX}layers.{l}.cross_attn_image_to_token.k_proj.bias"].abs().max()) == 0.0
    assert max(worst_n.values()) <= GRAD_TOL and max(worst_e.values()) <= GRAD_TOL, (kn, worst_n[kn], ke, worst_e[ke])


@pytest.mark.parametrize("name", list(XE_CASES))
def test_training_forward_without_dropout_is_the_eval_forward(name):
    """embedding_dropout = 0.0 keeps every query: the training graph's class_examples_embeddings and logits are the eval fixture's."""
    from labelanything_amd.train import LamTrainer
    lam, case, gold, _ = model_for(name)
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=17)
    tr = LamTrainer(lam, embedding_dropout=0.0)
    tr.zero_grad()
    res = tr.forward_backward(batch, gt)
    torch.cuda.synchronize()
    assert bool(res["extraction_keep"].all())
    errs = {k: rel_err(res[k], gold[k]) for k in ("class_examples_embeddings", "logits")}
    print(f"[{name}] training forward vs the eval fixture: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + f" (bound {TOL:.0e})")
    assert all(v <= TOL for v in errs.values()), errs
    assert torch.equal(res["flag_examples"].cpu(), gold["flag_examples"])


@pytest.mark.parametrize("spec", XE_TRAIN, ids=TRAIN_IDS)
def test_one_training_step_matches_the_reference(spec):
    name = spec["case"]
    lam, case, _, _ = model_for(name)
    gold, meta, gold_fwd = train_fixture(name)
    keep = gold["extraction_keep"].bool()
    lam.extraction_keep = keep
    tr, res, grads = run_training_step(lam, case, gold_fwd, gold, meta, TOL, label=name, embedding_dropout=0.2)
    e_ref = float(meta["e_ref32"])
    print(f"[train {name}] keep {keep.tolist()}; gradient bound {GRAD_TOL:.0e}; the reference's own fp32-vs-fp64 error {e_ref:.3e} (x4 = {4 * e_ref:.3e})")
    assert 4 * e_ref <= GRAD_TOL
    # the mask that was used comes back, and the flags are zero exactly for the dropped queries (and the classes no support shows)
    assert torch.equal(res["extraction_keep"], keep)
    flags = res["flag_examples"].cpu()
    assert torch.equal(flags, gold["flag_examples"])
    assert bool((flags[:, ~keep] == 0).all()) and bool((flags[:, keep] != 0).any(dim=1).any())
    # norm3 sits in the dead tail of the flat buffer and its gradient is exactly zero
    tail = [k for k in tr.names if k.startswith(tuple(k3.rsplit(".", 1)[0] for k3 in NORM3))]
    assert sorted(tail) == NORM3 and min(tr.names.index(k) for k in tail) > tr.names.index("mask_decoder.class_mlp.layers.2.bias")
    assert all(float(grads[k].abs().max()) == 0.0 for k in NORM3)
    MC.compare_gradients(tr.names, grads, gold, meta, GRAD_TOL, label=name)


def test_two_steps_draw_the_mask_move_the_extraction_and_keep_inference_working():
    """extraction_keep = None: every step draws its mask with draw_extraction_keep from the host generator.  Two optimizer steps move the
    extraction parameters, leave norm3 alone, and inference on the updated model runs (the engine repacks the folded layer-0 queries)."""
    from labelanything_amd.train import LamTrainer, draw_extraction_keep
    name = "x5_d64"
    lam, case, _, _ = model_for(name)
    n = int(case["cfg"].embeddings_per_example)
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=17)
    before_out = lam.forward_argmax(batch)["logits"].clone()
    before = {k: p.detach().clone() for k, p in lam.named_parameters() if k.startswith(EX)}
    assert lam.extraction_keep is None
    tr = LamTrainer(lam, embedding_dropout=0.2)
    masks = []
    for seed in (1, 3):
        torch.manual_seed(seed)
        want = draw_extraction_keep(n, 0.2)
        torch.manual_seed(seed)
        res = tr.step(batch, gt)
        assert torch.equal(res["extraction_keep"], want), (seed, res["extraction_keep"].tolist(), want.tolist())
        masks.append(want)
    torch.cuda.synchronize()
    assert not torch.equal(masks[0], masks[1])                     # seeds 1 and 3 drop different queries of the five
    after = dict(lam.named_parameters())
    moved = [k for k, v in before.items() if not torch.equal(after[k].detach(), v)]
    # (k_proj.bias has an exactly zero gradient: only the weight decay moves it, and not from zero)
    still = set(before) - set(moved)
    assert set(NORM3) <= still and all(k in NORM3 or k.endswith("k_proj.bias") for k in still), sorted(still)
    out = lam.forward_argmax(batch)["logits"]
    torch.cuda.synchronize()
    fin = torch.isfinite(before_out)
    assert torch.equal(torch.isfinite(out), fin) and not torch.equal(out[fin], before_out[fin])
