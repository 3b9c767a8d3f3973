#!/usr/bin/env python
"""Golden vectors for the loss components beyond focal (dice, fp, prompt_contrastive): the REFERENCE's LabelAnythingLoss
(loss/__init__.py) is imported and run on seeded logits / targets / class-example embeddings; its value, components and autograd
gradients (logits, embeddings, t_prime, bias) go to tests/golden/loss_components.safetensors (+ .json: the configurations).  Before
anything is written the fp64 restatement (tests/loss_components_ref.py) must agree with the reference.

A training fixture follows (tests/golden/train_loss_components.safetensors): three AdamW steps of the reference's WrapperModule with
case (a)'s loss on a reduced decoder-only model with class_attention and example_attention - per-step losses and components,
per-tensor gradient norms of the first step and the t_prime / bias trajectory.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_loss_components.py [loss] [train]
"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tools.golden_lib as GL                               # noqa: E402  (stub finder, the reference first on sys.path)

import torch                                                # noqa: E402
from safetensors.torch import save_file                     # noqa: E402

from tests.loss_components_ref import CASE_A, NAMES, TRAIN_LC_CASE   # noqa: E402

# name: (components, class_weighting, B, C, H, W, M, D, t_prime)
CASES = {
    "a": (CASE_A, True, 2, 4, 24, 40, 3, 32, None),
    "b": ({"focal": {"weight": 0.8}, "fp": {"weight": 0.1}, "prompt_contrastive": {"weight": 0.1}}, True, 3, 5, 20, 28, 2, 24, None),
    "c": ({"dice": {"weight": 1.0}}, False, 2, 3, 16, 20, 1, 8, None),
    "d": ({"focal": {"weight": 0.5}, "prompt_contrastive": {"weight": 1.0}}, True, 2, 3, 12, 16, 3, 16, math.log(50.0)),
    "e": ({"focal": {"weight": 0.6}, "dice": {"weight": 0.3}, "fp": {"weight": 0.2}}, True, 2, 4, 16, 24, 2, 8, None),
}
def make_inputs(name):
    comps, cwt, b, c, h, w, m, d, tp = CASES[name]
    g = torch.Generator().manual_seed(40 + ord(name))
    logits = torch.randn(b, c, h, w, generator=g) * 3
    target = torch.randint(0, c, (b, h, w), generator=g)
    emb = torch.randn(b, m, c, d, generator=g)
    flags = torch.ones(b, m, c, dtype=torch.uint8)
    if name == "a":
        target[:, -4:, :] = -100                     # padded rows: ignored target, -inf logits except the background class
        logits[:, 1:, -4:, :] = float("-inf")
        logits[:, 0, -4:, :] = 0.0
        target[torch.rand(b, h, w, generator=g) < 0.05] = -100
        flags[0, 1, :] = 0                           # an example row without prompts
        flags[1, :, 2] = 0                           # a class column without examples
        emb[1, 0, 1] *= 1e-14                        # a row whose norm is below F.normalize's eps
    if name == "b":
        target[0][target[0] >= 3] = 1                # classes 3, 4 absent from image 0
        target[1][target[1] == 2] = 0                # class 2 absent from image 1
        target[2, :3, :] = -100                      # image 2 has ignored pixels: background counts as present there
        flags[2, 1, 4] = 0
    if name == "d":
        flags[1] = 0                                 # an image with no flagged row contributes nothing
        target[torch.rand(b, h, w, generator=g) < 0.1] = -100
    if name == "e":
        target[1][target[1] == 3] = 0                # class 3 of image 1 is flagged off: -inf plane, no target pixel
        logits[1, 3] = float("-inf")
        target[0, :2, :] = -100
    return comps, cwt, logits, target, emb, flags, tp


def reference_loss_class():
    """The REFERENCE's LabelAnythingLoss: this repo's label_anything.loss re-exports the device one, which must not be picked up here."""
    from label_anything.loss import LabelAnythingLoss
    assert not LabelAnythingLoss.__module__.startswith("labelanything_amd"), LabelAnythingLoss.__module__
    return LabelAnythingLoss


def run_reference(comps, cwt, logits, target, emb, flags, tp):
    LabelAnythingLoss = reference_loss_class()
    crit = LabelAnythingLoss({k: dict(v) for k, v in comps.items()}, class_weighting=cwt)
    if tp is not None:
        with torch.no_grad():
            crit.prompt_components["prompt_contrastive"].t_prime.fill_(tp)
    x = logits.clone().requires_grad_(True)
    e = emb.clone().requires_grad_(True)
    res = crit({"logits": x, "class_examples_embeddings": e, "flag_examples": flags.clone()}, target)
    res["value"].backward()
    pc = crit.prompt_components["prompt_contrastive"] if "prompt_contrastive" in crit.prompt_components else None
    zero = torch.zeros(1)
    return {"value": res["value"].detach().reshape(1),
            "components": torch.tensor([float(res["components"].get(k, 0.0)) for k in NAMES]),
            "grad_logits": x.grad.clone(), "grad_emb": e.grad.clone() if e.grad is not None else torch.zeros_like(emb),
            "t_prime": pc.t_prime.detach().clone() if pc is not None else zero, "bias": pc.bias.detach().clone() if pc is not None else zero,
            "grad_t_prime": pc.t_prime.grad.clone() if pc is not None else zero, "grad_bias": pc.bias.grad.clone() if pc is not None else zero}


def check_restatement(name, inp, ref):
    from tests import loss_components_ref as R
    comps, cwt, logits, target, emb, flags, _ = inp
    x = logits.double().requires_grad_(True)
    e = emb.double().requires_grad_(True)
    tp = ref["t_prime"].double().requires_grad_(True)
    bs = ref["bias"].double().requires_grad_(True)
    val, cv = R.objective(comps, cwt, x, target, e, flags, tp, bs)
    val.backward()
    assert abs(float(val) - float(ref["value"])) <= 2e-6 * max(1.0, abs(float(ref["value"]))), (name, float(val), float(ref["value"]))
    for i, k in enumerate(NAMES):
        if k in cv:
            assert abs(float(cv[k]) - float(ref["components"][i])) <= 2e-6 * max(1.0, abs(float(ref["components"][i]))), (name, k)
    gl = ref["grad_logits"]
    fin = torch.isfinite(x.grad)
    assert bool(fin.all()) and bool(torch.isfinite(gl).all()), name
    assert float((x.grad - gl).abs().max()) <= 1e-5 * float(gl.abs().max()), (name, float((x.grad - gl).abs().max()))
    if "prompt_contrastive" in comps:
        for mine, theirs in ((e.grad, ref["grad_emb"]), (tp.grad, ref["grad_t_prime"]), (bs.grad, ref["grad_bias"])):
            assert float((mine - theirs).abs().max()) <= 1e-5 * max(1.0, float(theirs.abs().max())), name


def make_loss():
    out, meta = {}, {}
    for name in CASES:
        inp = make_inputs(name)
        ref = run_reference(*inp)
        comps, cwt, logits, target, emb, flags, tp = inp
        if name == "d":
            # the reference's gradients are NaN for t_prime, bias and image 1's rows: loss / valid_b with valid_b = 0 is inf, the
            # boolean index drops it from the value but its backward multiplies 0 by 1 / valid_b.  The device loss gives that image
            # a zero gradient; what is stored is the reference on image 0 alone, scaled by 1 / B (its share of the batch mean)
            assert bool(ref["grad_t_prime"].isnan().all()) and bool(ref["grad_emb"][1].isnan().all())
            one = run_reference(comps, cwt, logits[:1], target[:1], emb[:1], flags[:1], tp)
            b = logits.shape[0]
            ref["grad_t_prime"], ref["grad_bias"] = one["grad_t_prime"] / b, one["grad_bias"] / b
            ref["grad_emb"] = torch.cat([one["grad_emb"] / b, torch.zeros_like(emb[1:])])
        check_restatement(name, inp, ref)
        for k, v in {"logits": logits, "target": target, "emb": emb, "flags": flags, **ref}.items():
            out[f"{name}.{k}"] = v.clone().contiguous()
        meta[name] = {"components": comps, "class_weighting": cwt, "value": float(ref["value"]),
                      "reported": {k: float(ref["components"][i]) for i, k in enumerate(NAMES) if k in comps}}
        print(name, meta[name]["value"], meta[name]["reported"])
    save_file(out, os.path.join(ROOT, "tests", "golden", "loss_components.safetensors"))
    with open(os.path.join(ROOT, "tests", "golden", "loss_components.json"), "w") as fh:
        json.dump({"cases": meta, "component_order": NAMES, "generated_by": "tools/make_golden_loss_components.py",
                   "torch": torch.__version__}, fh, indent=1)


def make_train():
    from label_anything.experiment.utils import WrapperModule
    from transformers import get_scheduler
    from tests.helpers import make_gt
    from labelanything_amd.episodes import make_episode

    case = TRAIN_LC_CASE
    lam, sd = GL.build_reference(case)
    lam.train()
    cfg = case["cfg"]
    batch = make_episode(**case["episode"])
    c = batch["flag_examples"].shape[2]
    gt = make_gt(batch, c, seed=case["gt_seed"])
    gr = torch.Generator().manual_seed(case["weight_seed"] + 7)
    rows = torch.cat([torch.zeros(1, dtype=torch.long), torch.randperm(cfg.bank_size - 1, generator=gr)[: c - 1] + 1])
    lam.prompt_encoder.class_encoder.sample_rows = lambda C, device, _r=rows: _r.to(device)
    crit = reference_loss_class()({k: dict(v) for k, v in CASE_A.items()}, class_weighting=True)
    model = WrapperModule(lam, crit)
    params = model.get_learnable_params({})          # no image encoder in this model: every tensor learns
    opt = torch.optim.AdamW(params, lr=case["lr"], weight_decay=case["weight_decay"])
    sched = get_scheduler("constant_with_warmup", opt, num_warmup_steps=case["warmup"], num_training_steps=100)
    named = dict(model.named_parameters())
    named = {k: p for k, p in named.items() if p.requires_grad and not k.startswith("model.image_encoder.")}
    pc = crit.prompt_components["prompt_contrastive"]
    losses, comps, tps, bss, gtp, gbs = [], [], [pc.t_prime.item()], [pc.bias.item()], [], []
    out = {"gt": gt, "selected_rows": rows}
    for step in range(case["steps"]):
        res = model(batch, gt)
        loss = res["loss"]["value"]
        loss.backward()
        losses.append(float(loss))
        comps.append([float(res["loss"]["components"].get(k, 0.0)) for k in NAMES])
        gtp.append(float(pc.t_prime.grad))
        gbs.append(float(pc.bias.grad))
        if step == 0:
            grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in named.items()}
            out["logits0"] = res["logits"].detach().clone()
            out["class_examples_embeddings0"] = res["class_examples_embeddings"].detach().clone()
        opt.step()
        sched.step()
        opt.zero_grad()
        tps.append(pc.t_prime.item())
        bss.append(pc.bias.item())
    # the trainer's names: the model's tensors without the "model." prefix, the loss's as the reference's checkpoints name them
    keys = sorted(k[len("model."):] if k.startswith("model.") else k for k in named)
    g = {(k[len("model."):] if k.startswith("model.") else k): v for k, v in grads.items()}
    out["loss"] = torch.tensor(losses)
    out["components"] = torch.tensor(comps)
    out["grad_norm"] = torch.stack([g[k].norm() for k in keys])
    out["t_prime"], out["bias"] = torch.tensor(tps), torch.tensor(bss)
    out["grad_t_prime"], out["grad_bias"] = torch.tensor(gtp), torch.tensor(gbs)
    save_file(out, os.path.join(ROOT, "tests", "golden", "train_loss_components.safetensors"))
    with open(os.path.join(ROOT, "tests", "golden", "train_loss_components.json"), "w") as fh:
        json.dump({"keys": keys, "losses": losses, "components": comps, "component_order": NAMES, "t_prime": tps, "bias": bss,
                   "generated_by": "tools/make_golden_loss_components.py", "torch": torch.__version__}, fh, indent=1)
    print("losses", losses, "t_prime", tps, "bias", bss, "tensors", len(keys))


def main():
    which = sys.argv[1:] or ["loss", "train"]
    if "loss" in which:
        make_loss()
    if "train" in which:
        make_train()


if __name__ == "__main__":
    main()
