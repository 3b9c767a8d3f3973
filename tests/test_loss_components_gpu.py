"""GPU: the device LabelAnythingLoss (la_logits_objective + la_prompt_contrastive) against the reference's fixtures
(tests/golden/loss_components.safetensors, train_loss_components.safetensors: tools/make_golden_loss_components.py) and the fp64
restatement (tests/loss_components_ref.py); determinism, graph replay and the trainer paths with the composite loss."""
import json
import math
import os

import pytest
import torch
from safetensors.torch import load_file

from labelanything_amd import _lib as L
from labelanything_amd.loss import LabelAnythingLoss
from tests import loss_components_ref as R
from tests import loss_profiles as P
from tests.helpers import GOLDEN

pytestmark = pytest.mark.gpu
COMPOSITE = {"focal": {"weight": 0.725}, "dice": {"weight": 0.025}, "fp": {"weight": 0.1}, "prompt_contrastive": {"weight": 0.25}}


def _device_run(comps, cwt, logits, target, emb, flags, t_prime=None, bias=None):
    crit = LabelAnythingLoss(comps, class_weighting=cwt).cuda()
    pc = crit.prompt_components["prompt_contrastive"] if "prompt_contrastive" in crit.prompt_components else None
    if pc is not None and t_prime is not None:
        with torch.no_grad():
            pc.t_prime.copy_(t_prime)
            pc.bias.copy_(bias)
    x = logits.cuda().requires_grad_(True)
    e = emb.cuda().requires_grad_(True)
    res = crit({"logits": x, "class_examples_embeddings": e, "flag_examples": flags.cuda()}, target.cuda())
    res["value"].backward()
    out = {"value": res["value"].detach().cpu(), "components": {k: v.cpu() for k, v in res["components"].items()},
           "grad_logits": x.grad.cpu(), "grad_emb": e.grad.cpu() if e.grad is not None else torch.zeros_like(emb)}
    if pc is not None:
        out["grad_t_prime"], out["grad_bias"] = pc.t_prime.grad.cpu(), pc.bias.grad.cpu()
    return out


def test_fixture_cases_match_the_reference():
    t = load_file(os.path.join(GOLDEN, "loss_components.safetensors"))
    with open(os.path.join(GOLDEN, "loss_components.json")) as fh:
        meta = json.load(fh)
    names = meta["component_order"]
    for name, m in meta["cases"].items():
        got = _device_run(m["components"], m["class_weighting"], t[f"{name}.logits"], t[f"{name}.target"], t[f"{name}.emb"],
                          t[f"{name}.flags"], t[f"{name}.t_prime"], t[f"{name}.bias"])
        ref_v = float(t[f"{name}.value"])
        assert abs(float(got["value"]) - ref_v) <= 2e-6 * max(1.0, abs(ref_v)), (name, float(got["value"]), ref_v)
        assert list(got["components"]) == list(m["components"]), name
        for k, v in got["components"].items():
            r = float(t[f"{name}.components"][names.index(k)])
            assert abs(float(v) - r) <= 2e-6 * max(1.0, abs(r)), (name, k, float(v), r)
        g, rg = got["grad_logits"], t[f"{name}.grad_logits"]
        assert torch.isfinite(g).all(), name
        assert float((g - rg).abs().max()) <= 5e-6 * float(rg.abs().max()), (name, float((g - rg).abs().max()))
        if "prompt_contrastive" in m["components"]:
            for k in ("grad_emb", "grad_t_prime", "grad_bias"):
                assert torch.isfinite(got[k]).all(), (name, k)
                err = float((got[k] - t[f"{name}.{k}"]).abs().max())
                assert err <= 1e-5 * max(1.0, float(t[f"{name}.{k}"].abs().max())), (name, k, err)


def _random_inputs(b, c, h, w, m=2, d=48, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(b, c, h, w, generator=g) * 4
    target = torch.randint(0, c, (b, h, w), generator=g)
    target[torch.rand(b, h, w, generator=g) < 0.1] = -100
    if c > 3:
        target[0][target[0] == 2] = 1                          # class 2 absent from image 0
    logits[:, 1:, -3:, :] = float("-inf")                        # padded rows
    logits[:, 0, -3:, :] = 0.0
    target[:, -3:, :] = -100
    emb = torch.randn(b, m, c, d, generator=g)
    flags = (torch.rand(b, m, c, generator=g) < 0.8).to(torch.uint8)
    return logits, target, emb, flags


@pytest.mark.parametrize("shape", [(1, 2, 1024, 1024), (3, 21, 200, 333), (2, 64, 40, 52), (2, 6, 33, 35), (2, 64, 37, 41)])
def test_random_shapes_match_the_restatement(shape):
    logits, target, emb, flags = _random_inputs(*shape, seed=shape[1])
    got = _device_run(COMPOSITE, True, logits, target, emb, flags)
    dev = "cuda"
    x = logits.to(dev).double().requires_grad_(True)
    e = emb.to(dev).double().requires_grad_(True)
    tp = torch.tensor([math.log(10.0)], dtype=torch.float64, device=dev, requires_grad=True)
    bs = torch.tensor([-10.0], dtype=torch.float64, device=dev, requires_grad=True)
    val, comps = R.objective(COMPOSITE, True, x, target.to(dev), e, flags.to(dev), tp, bs)
    val.backward()
    assert abs(float(got["value"]) - float(val)) <= 5e-6 * max(1.0, abs(float(val))), (float(got["value"]), float(val))
    for k, v in comps.items():
        assert abs(float(got["components"][k]) - float(v)) <= 5e-6 * max(1.0, abs(float(v))), k
    rg = x.grad.cpu()
    assert float((got["grad_logits"].double() - rg).abs().max()) <= 1e-5 * float(rg.abs().max())
    for mine, ref in ((got["grad_emb"], e.grad), (got["grad_t_prime"], tp.grad), (got["grad_bias"], bs.grad)):
        ref = ref.cpu()
        assert float((mine.double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))


def test_logits_components_alone_and_without_gradient():
    logits, target, _, _ = _random_inputs(2, 5, 48, 64, seed=9)
    for comps in ({"dice": {"weight": 0.5}}, {"fp": {"weight": 2.0}}, {"focal": {"weight": 1.0, "gamma": 1.5}, "fp": {"weight": 0.3}}):
        crit = LabelAnythingLoss(comps, class_weighting=False)
        res = crit(logits.cuda(), target.cuda())                    # logits only, no autograd: no gradient buffer
        x = logits.double().requires_grad_(False)
        val, ref = R.objective(comps, False, x, target)
        assert abs(float(res["value"]) - float(val)) <= 5e-6 * max(1.0, abs(float(val))), comps
        assert set(res["components"]) == set(comps)
        assert int(crit.bad_targets) == 0
        # with a gradient: against the sum of the components' own fp64 gradients, per image and relative to the smallest of them
        # (tests/loss_profiles.py); the tolerance is the fp32 restatement's error under the same measure times its margin
        xg = logits.cuda().requires_grad_(True)
        with_grad = LabelAnythingLoss(comps, class_weighting=False)(xg, target.cuda())
        with_grad["value"].backward()
        assert torch.equal(with_grad["value"].detach(), res["value"])
        cw = R.class_weights(target, logits.shape[1], False)
        gamma = float(comps.get("focal", {}).get("gamma", 2.0))
        fns = {"focal": lambda v: R.focal(v, target, gamma, cw), "dice": lambda v: R.dice(v, target, cw), "fp": lambda v: R.false_positive(v, target)}
        parts = [P._grad64(fns[k], logits)[1] * float(kw["weight"]) ** 2 for k, kw in comps.items()]
        mask = sum({"focal": 1, "dice": 2, "fp": 4}[k] for k in comps)
        weights = {k: float(comps.get(k, {}).get("weight", 0.0)) for k in ("focal", "dice", "fp")}
        const = P.image_ratio(P.logits32(logits, target, mask, gamma, False, weights=weights)["grad"], parts)
        fig = P.image_ratio(xg.grad, parts)
        print(f"{sorted(comps)}: gradient {fig:.3g}, restatement {const:.3g}")
        assert fig <= P.MARGIN * max(const, P.U), (comps, fig, const)


def test_two_calls_are_bitwise_identical():
    logits, target, emb, flags = _random_inputs(2, 21, 96, 128, seed=4)
    a = _device_run(COMPOSITE, True, logits, target, emb, flags)
    b = _device_run(COMPOSITE, True, logits, target, emb, flags)
    assert torch.equal(a["value"], b["value"])
    for k in ("grad_logits", "grad_emb", "grad_t_prime", "grad_bias"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(a["components"][k], b["components"][k]) for k in a["components"])


def test_graph_replay_matches_eager_bitwise():
    logits, target, emb, flags = _random_inputs(2, 6, 64, 80, m=3, d=64, seed=5)
    x, t = logits.cuda(), target.cuda()
    bsz, c = x.shape[:2]
    hw = x.shape[2] * x.shape[3]
    e = emb.cuda().reshape(bsz, -1, emb.shape[-1]).contiguous()
    f = flags.cuda().reshape(bsz, -1).contiguous()
    tp = torch.tensor([math.log(10.0)], device="cuda")
    bs = torch.tensor([-10.0], device="cuda")
    ws1 = torch.empty(L.logits_objective_workspace_bytes(bsz, c, hw), dtype=torch.uint8, device="cuda")
    ws2 = torch.empty(L.prompt_contrastive_workspace_bytes(bsz, e.shape[1], e.shape[2]), dtype=torch.uint8, device="cuda")

    def outputs():
        return [torch.empty(1, device="cuda"), torch.empty(3, device="cuda"), torch.empty_like(x), torch.empty(c, device="cuda"),
                torch.empty(1, device="cuda"), torch.empty_like(e), torch.empty(1, device="cuda"), torch.empty(1, device="cuda")]

    def launch(o):
        L.logits_objective(x, t, -100, 7, 0.725, 2.0, 0.025, 0.1, True, o[0], o[1], o[2], o[3], ws1)
        L.prompt_contrastive(e, f, c, tp, bs, o[4], o[5], o[6], o[7], ws2)

    eager = outputs()
    launch(eager)
    torch.cuda.synchronize()
    graphed = outputs()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch(graphed)                                          # warm-up on a side stream
    torch.cuda.current_stream().wait_stream(s)
    for o in graphed:
        o.zero_()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        launch(graphed)
    for o in graphed:
        o.zero_()
    gr.replay()
    gr.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, graphed):
        assert torch.equal(a, b)


def test_limits_raise_clear_errors():
    crit = LabelAnythingLoss({"prompt_contrastive": {"weight": 1.0}}).cuda()
    logits = torch.zeros(1, 2, 4, 4, device="cuda")
    with pytest.raises(RuntimeError, match="must be <="):
        crit({"logits": logits, "class_examples_embeddings": torch.randn(1, 2, 2, 1100, device="cuda"),
              "flag_examples": torch.ones(1, 2, 2, device="cuda")}, torch.zeros(1, 4, 4, dtype=torch.long, device="cuda"))
    with pytest.raises(RuntimeError, match="C <= 64"):
        LabelAnythingLoss({"focal": {"weight": 1.0}})(torch.zeros(1, 65, 4, 4, device="cuda"), torch.zeros(1, 4, 4, dtype=torch.long).cuda())
    with pytest.raises(RuntimeError, match="device tensors"):
        LabelAnythingLoss({"dice": {"weight": 1.0}})(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long))


def test_out_of_range_targets_are_counted():
    logits, target, _, _ = _random_inputs(2, 4, 16, 16, seed=2)
    target[0, 0, :5] = 7
    crit = LabelAnythingLoss({"focal": {"weight": 1.0}, "dice": {"weight": 1.0}}, class_weighting=True)
    res = crit(logits.cuda(), target.cuda())
    assert int(crit.bad_targets) == 5 and torch.isfinite(res["value"])


# ---- trainer ------------------------------------------------------------------------------------------------------------------------
def _trainer(case, rows, loss, **kw):
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    lam = Lam(case["cfg"], seed=case["weight_seed"]).cuda()
    lam.selected_rows = rows
    return lam, LamTrainer(lam, loss=loss, **kw)


def test_three_steps_match_the_reference_fixture():
    """tests/golden/train_loss_components.safetensors: the reference's WrapperModule with focal 0.725 + dice 0.025 +
    prompt_contrastive 0.25 (class weighting), torch AdamW (the loss's t_prime / bias appended) and the HF warm-up schedule."""
    from labelanything_amd.episodes import make_episode
    case = R.TRAIN_LC_CASE
    gold = load_file(os.path.join(GOLDEN, "train_loss_components.safetensors"))
    with open(os.path.join(GOLDEN, "train_loss_components.json")) as fh:
        keys = json.load(fh)["keys"]
    batch = make_episode(**case["episode"])
    crit = LabelAnythingLoss({k: dict(v) for k, v in R.CASE_A.items()}, class_weighting=True)
    lam, tr = _trainer(case, gold["selected_rows"], crit, lr=case["lr"], weight_decay=case["weight_decay"], num_warmup_steps=case["warmup"])
    assert sorted(tr.names) == keys
    pc = crit.prompt_components["prompt_contrastive"]
    losses, comps, tps, bss = [], [], [float(pc.t_prime)], [float(pc.bias)]
    names = list(R.NAMES)
    for step in range(case["steps"]):
        tr.zero_grad()
        res = tr.forward_backward(batch, gold["gt"])
        losses.append(float(res["loss"]))
        comps.append([float(res["loss_components"].get(k, 0.0)) for k in names])
        if step == 0:
            g0 = {k: gv.clone() for k, gv in zip(tr.names, tr.opt.grad_views)}
            assert float((res["logits"].cpu() - gold["logits0"]).abs().max()) <= 2e-5 * float(gold["logits0"][torch.isfinite(gold["logits0"])].abs().max())
        tr.apply_update()
        lam.invalidate()
        tps.append(float(pc.t_prime))
        bss.append(float(pc.bias))
    assert torch.allclose(torch.tensor(losses), gold["loss"], rtol=2e-5, atol=0), (losses, gold["loss"])
    assert torch.allclose(torch.tensor(comps), gold["components"], rtol=2e-5, atol=1e-7), (comps, gold["components"])
    gn = torch.stack([g0[k].norm() for k in keys]).cpu()
    floor_g = 1e-3 * float(gold["grad_norm"].max())
    assert float(((gn - gold["grad_norm"]).abs() / gold["grad_norm"].clamp_min(floor_g)).max()) <= 1e-3
    # t_prime / bias: AdamW's first real step moves each by ~lr in the sign of its gradient; the trajectory follows the reference's
    assert torch.allclose(torch.tensor(tps), gold["t_prime"], rtol=0, atol=2e-5 * case["lr"] / 1e-3), (tps, gold["t_prime"])
    assert torch.allclose(torch.tensor(bss), gold["bias"], rtol=0, atol=2e-5 * case["lr"] / 1e-3), (bss, gold["bias"])
    assert tps[-2] != tps[0] and bss[-2] != bss[0]


def test_accumulated_substitution_returns_the_standalone_loss_per_step():
    from labelanything_amd.substitution import Substitutor
    from tests.cases import CASES
    from tests.helpers import dataset_batch
    case = CASES["novit_d256_2w3s"]
    batch, gts = dataset_batch(case, seed=4)
    comps = {k: dict(v) for k, v in COMPOSITE.items()}
    crit = LabelAnythingLoss(comps, class_weighting=True)
    _, tr = _trainer(case, torch.tensor([0, 5, 9]), crit, lr=1e-3)
    start = [float(p) for p in crit.parameters()]
    sub = Substitutor(num_points=1, long_side_length=256, generator=torch.Generator(device="cuda").manual_seed(7))
    ref_crit = LabelAnythingLoss({k: dict(v) for k, v in COMPOSITE.items()}, class_weighting=True).cuda()
    steps = 0
    for r in tr.substitution_steps(batch, gts, sub, accumulate=True):
        steps += 1
        with torch.no_grad():
            ref = ref_crit({"logits": r["logits"], "class_examples_embeddings": r["class_examples_embeddings"],
                            "flag_examples": r["input"]["flag_examples"]}, r["gt"])
        assert torch.equal(r["loss"], ref["value"]), (r["step"], float(r["loss"]), float(ref["value"]))
        assert set(r["loss_components"]) == set(COMPOSITE)
        for k, v in ref["components"].items():
            assert torch.equal(r["loss_components"][k], v), (r["step"], k)
    assert steps == batch["embeddings"].shape[1] + 1
    assert [float(p) for p in crit.parameters()] != start        # one update at the end moved t_prime / bias


def test_trainable_encoder_step_with_the_composite_loss():
    from labelanything_amd.episodes import make_episode
    from tests.cases import TRAIN_ENC_CASE as case
    from tests.helpers import make_gt
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=3)
    crit = LabelAnythingLoss({k: dict(v) for k, v in COMPOSITE.items()}, class_weighting=True)
    _, tr = _trainer(case, None, crit, lr=1e-3, train_encoder=True)
    before = [float(p) for p in crit.parameters()]
    for _ in range(2):
        res = tr.step(batch, gt)
        assert torch.isfinite(res["loss"]) and set(res["loss_components"]) == set(COMPOSITE)
    assert [float(p) for p in crit.parameters()] != before
    i = tr.names.index("loss.prompt_components.prompt_contrastive.t_prime")
    assert tr.opt.tensor_steps[i] == 2
