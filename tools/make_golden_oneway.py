#!/usr/bin/env python
"""Golden vectors of the one-way mask decoder from the REFERENCE (build container only; builds on tools/make_golden.py's stub finder):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_oneway.py [--only NAME] [--no-train]

For every case of tests/cases_oneway.py the seeded weights (``init_state_dict``) are strict-loaded into
``_build_lam(..., fusion_transformer="OneWayTransformer")`` and the seeded episode runs through the reference's ``Lam.forward`` on CPU /
fp32, the class-encoder rows pinned as tools/make_golden_multi_embedding.py:fixed_rows does.  tests/golden/oneway_<case>.json holds the
reference's state-dict keys and shapes IN ITS ORDER; the .safetensors its OUTPUTS: class_embeddings, every ``SRC_STRIDE``-th pixel row,
pixel column and channel of the mask-decoder transformer's image output (a forward hook), low_res_logits, logits and argmax.  The json
also records the share of pixels whose top-two logit gap lies inside the 2e-3 margin band on the reference's own logits; it must be at
most 5 % (otherwise pick another weight seed).  For the case of ``OW_TRAIN`` one training step (focal objective, class weighting) is
stored as oneway_<case>_train.{safetensors,json}: loss, per-tensor gradient norms, the full gradients of ``OW_TRAIN_FULL``, the
reference's own fp32-vs-fp64 gradient error, the tensors that received no gradient and the smallest ReLU pre-activation of the stream MLPs
in the fp64 run relative to the largest, which must lie outside ``KINK_BAND`` (tests/cases_oneway.py says why).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tools.make_golden as MG          # noqa: E402,F401  (installs the stub finder, puts the reference first on sys.path)

import torch                            # noqa: E402
from safetensors.torch import save_file  # noqa: E402
from label_anything.models.build_lam import _build_lam   # noqa: E402  (the reference)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def build_reference(case):
    from labelanything_amd.weights import init_state_dict
    cfg = case["cfg"]
    assert cfg.encoder_spec is None, "decoder-only cases"
    lam = _build_lam(
        build_vit=None, use_vit=False, image_embed_dim=cfg.image_embed_dim, embed_dim=cfg.embed_dim, image_size=cfg.image_size,
        class_attention=cfg.class_attention, example_attention=cfg.example_attention, example_class_attention=cfg.example_class_attention,
        spatial_convs=cfg.spatial_convs, class_encoder=dict(cfg.class_encoder) if cfg.class_encoder else None,
        custom_preprocess=cfg.custom_preprocess, fusion_transformer=cfg.fusion_transformer)
    lam.eval()
    sd = init_state_dict(cfg, case["weight_seed"])
    lam.load_state_dict(sd, strict=True)
    return lam, sd


def band_share(logits, margin):
    """Share of pixels whose top-two gap is within margin * max|finite logit| (the pixels the argmax test does not compare)."""
    top2 = logits.float().topk(2, dim=1).values
    scale = float(logits[torch.isfinite(logits)].abs().max())
    return float(((top2[:, 0] - top2[:, 1]) <= margin * scale).double().mean())


def run_forward(name, case):
    from labelanything_amd.episodes import make_episode
    from tests.cases_oneway import MARGIN, MAX_BAND_SHARE, SRC_STRIDE
    from tools.make_golden_multi_embedding import fixed_rows
    lam, sd = build_reference(case)
    ref_keys = [[k, list(v.shape)] for k, v in lam.state_dict().items()]
    tr = "mask_decoder.transformer."
    assert sorted(k for k, _ in ref_keys) == sorted(sd) and all(list(sd[k].shape) == s for k, s in ref_keys)
    assert [k for k, _ in ref_keys if k.startswith(tr)] == [k for k in sd if k.startswith(tr)], \
        "init_state_dict must give the transformer's keys in the reference's order"
    cfg = case["cfg"]
    batch = make_episode(**case["episode"])
    b, m, c = batch["flag_examples"].shape
    rows = fixed_rows(lam, case, c)
    seen = {}
    hook = lam.mask_decoder.transformer.register_forward_hook(lambda mod, inp, out: seen.update(tokens=out[0], image=out[1]))
    with torch.no_grad():
        seg_low, pe_result = lam._forward(batch)
        hook.remove()
        ref = lam(batch)
    g, d = cfg.grid, cfg.embed_dim
    img = seen["image"]
    assert tuple(img.shape) == (b, g * g, d), img.shape
    assert torch.equal(seen["tokens"], pe_result["class_embeddings"]), "the one-way transformer hands the class tokens back untouched"
    st = SRC_STRIDE
    tensors = {
        "class_embeddings": pe_result["class_embeddings"].contiguous(),
        "transformer_image_sample": img.view(b, g, g, d)[:, ::st, ::st, ::st].flatten(1, 2).contiguous(),
        "low_res_logits": seg_low.contiguous(),
        "logits": ref["logits"].contiguous(),
        "argmax": ref["logits"].argmax(dim=1).to(torch.uint8).contiguous(),
    }
    if rows is not None:
        tensors["selected_rows"] = rows
    share = band_share(ref["logits"], MARGIN)
    assert share <= MAX_BAND_SHARE, f"{name}: {share:.3%} of the reference's pixels lie inside the margin band; pick another weight seed"
    path = os.path.join(GOLDEN, f"oneway_{name}.safetensors")
    save_file(tensors, path)
    fin = torch.isfinite(ref["logits"])
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "classes": c, "src_stride": st,
            "full_image_shape": list(img.shape), "state_dict": ref_keys, "margin": MARGIN, "margin_band_share": share,
            "image_scale": float(img.abs().max()), "low_res_scale": float(seg_low.abs().max()),
            "finite_logit_fraction": float(fin.double().mean()), "torch": torch.__version__,
            "generated_by": "tools/make_golden_oneway.py"}
    with open(os.path.join(GOLDEN, f"oneway_{name}.json"), "w") as fh:
        json.dump(meta, fh, indent=1, default=list)
    assert bool(torch.isfinite(seg_low).all())
    print(f"[{name}] tensors {len(ref_keys)} classes {c} bytes {os.path.getsize(path)} band share {share:.4f} low-res scale "
          f"{meta['low_res_scale']:.3f}")


def grads_of(case, gt, double: bool):
    from label_anything.experiment.utils import WrapperModule
    from label_anything.loss import LabelAnythingLoss
    from labelanything_amd.episodes import make_episode
    from tools.make_golden_multi_embedding import fixed_rows
    lam, sd = build_reference(case)
    lam.train()
    batch = make_episode(**case["episode"])
    if double:
        lam.double()
        batch = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}
    rows = fixed_rows(lam, case, batch["flag_examples"].shape[2])
    pre = []         # ReLU pre-activations of the stream MLPs: how close the step comes to a kink (tests.cases_oneway.KINK_BAND)
    hooks = [blk.mlp.lin1.register_forward_hook(lambda mod, inp, out: pre.append(float(out.detach().abs().min() / out.detach().abs().max())))
             for blk in lam.mask_decoder.transformer.layers]
    model = WrapperModule(lam, LabelAnythingLoss({"focal": {"weight": 1.0}}, class_weighting=True))
    res = model(batch, gt)
    loss = res["loss"]["value"]
    loss.backward()
    for h in hooks:
        h.remove()
    grads_of.relu_gap = min(pre)
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in lam.named_parameters()}
    assert all(k in sd for k in grads)
    return float(loss), grads, rows


def run_train(name, case, seed_gt, full):
    from labelanything_amd.episodes import make_episode
    from tests.helpers import make_gt
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=seed_gt)
    loss32, g32, rows = grads_of(case, gt, double=False)
    loss64, g64, _ = grads_of(case, gt, double=True)
    from tests.cases_oneway import KINK_BAND
    relu_gap = grads_of.relu_gap            # of the fp64 run
    assert relu_gap >= KINK_BAND, f"{name}: a ReLU pre-activation of the stream MLP lies at {relu_gap:.2e} of the largest; pick another weight seed"
    keys = sorted(k for k, g in g32.items() if g is not None)
    assert keys == sorted(k for k, g in g64.items() if g is not None)
    dead = sorted(k for k, g in g32.items() if g is None)
    assert all(f"mask_decoder.transformer.layers.{l}.norm3.{n}" in dead for l in range(2) for n in ("weight", "bias"))
    gmax = max(float(g64[k].abs().max()) for k in keys)
    # the reference's own fp32 error on every gradient tensor, in the units of the tests' bound: of the tensor's scale, floored at 1e-2
    # of the largest gradient
    e32 = {k: float((g32[k].double() - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-2 * gmax) for k in keys}
    out = {"loss": torch.tensor([loss32]), "grad_norm": torch.stack([g32[k].norm() for k in keys])}
    if rows is not None:
        out["selected_rows"] = rows
    for k in full:
        out["grad." + k] = g32[k].contiguous()
    path = os.path.join(GOLDEN, f"oneway_{name}_train.safetensors")
    save_file(out, path)
    with open(os.path.join(GOLDEN, f"oneway_{name}_train.json"), "w") as fh:
        json.dump({"keys": keys, "dead": dead, "loss": loss32, "loss_fp64": loss64, "e_ref32": max(e32.values()),
                   "e_ref32_worst_tensor": max(e32, key=e32.get), "seed_gt": seed_gt,
                   "relu_min_gap": relu_gap, "weight_seed": case["weight_seed"], "torch": torch.__version__,
                   "generated_by": "tools/make_golden_oneway.py"}, fh, indent=1)
    print(f"[{name} train] loss {loss32:.8f} (fp64 {loss64:.8f}) e_ref32 {max(e32.values()):.3e} at {max(e32, key=e32.get)} "
          f"tensors {len(keys)} dead {dead} bytes {os.path.getsize(path)}")


def main():
    from tests.cases_oneway import OW_CASES, OW_TRAIN, OW_TRAIN_FULL
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    for name, case in OW_CASES.items():
        if a.only in (None, name):
            run_forward(name, case)
    if not a.no_train and a.only in (None, OW_TRAIN["case"]):
        run_train(OW_TRAIN["case"], OW_CASES[OW_TRAIN["case"]], OW_TRAIN["seed_gt"], OW_TRAIN_FULL)


if __name__ == "__main__":
    main()
