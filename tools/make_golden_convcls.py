#!/usr/bin/env python
"""Golden vectors of ``conv_classification`` / ``classification_layer_downsample_rate=1`` from the REFERENCE (build container only; builds
on tools/make_golden.py's stub finder):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_convcls.py [--only NAME] [--no-train]

For every case of tests/cases_convcls.py the seeded weights (``init_state_dict``, including ``mask_decoder.prototype_tconv.*``; the state
dict strict-loads) go into ``_build_lam(..., classification_layer_downsample_rate=r, conv_classification=...)``, the seeded episode runs
through the reference's ``Lam.forward`` on CPU / fp32 and the reference's OUTPUTS are written to tests/golden/<case>.safetensors:
low_res_logits, logits, argmax, selected_rows.  The operands of the final ``_classify`` (the feature map as NHWC rows and the prototypes) go
to <case>_feat.safetensors for the conv cases; at cf = 256 the map is 4 MB, so only its first ``feature_rows`` rows are kept (the json says
how many): they determine the logit rows 0 .. feature_rows - 3.

The json holds the model's key list and shapes, the initialisation scale of prototype_tconv (weights.PROTOTYPE_TCONV_FAN) and the measured
magnitude of the low-resolution logits.

For ``CC_TRAIN`` (and ``CC_TRAIN_PLAIN``, the same step without the two tensors) one decoder-only training step (WrapperModule + focal loss, as tools/make_golden_train.py) is stored as <case>_train:
loss, per-tensor gradient norms, a handful of full gradients (of the two prototype_tconv tensors the first CC_TCONV_ROWS input channels),
and ``e_kink`` - the worst per-tensor difference between the reference's own fp32 and fp64 gradients, relative to the tensor's scale
floored at 1e-2 of the model's largest gradient.
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
FEATURE_BYTES = 900_000                 # what <case>_feat.safetensors may spend on feature rows


def build_reference(case):
    from labelanything_amd.weights import init_state_dict
    cfg = case["cfg"]
    assert cfg.encoder_spec is None, "decoder-only cases"
    lam = _build_lam(
        build_vit=None, use_vit=False, image_embed_dim=cfg.image_embed_dim, embed_dim=cfg.embed_dim, image_size=cfg.image_size,
        class_attention=cfg.class_attention, example_attention=cfg.example_attention, example_class_attention=cfg.example_class_attention,
        spatial_convs=cfg.spatial_convs, class_encoder=dict(cfg.class_encoder) if cfg.class_encoder else None,
        custom_preprocess=cfg.custom_preprocess, classification_layer_downsample_rate=cfg.classification_layer_downsample_rate,
        conv_classification=cfg.conv_classification)
    lam.eval()
    sd = init_state_dict(cfg, case["weight_seed"])
    lam.load_state_dict(sd, strict=True)
    return lam, sd


def fixed_rows(lam, case, c):
    cfg = case["cfg"]
    if not cfg.bank_size:
        return None
    gr = torch.Generator().manual_seed(case["weight_seed"] + 7)
    rows = torch.cat([torch.zeros(1, dtype=torch.long), torch.randperm(cfg.bank_size - 1, generator=gr)[: c - 1] + 1])
    lam.prompt_encoder.class_encoder.sample_rows = lambda C, device, _r=rows: _r.to(device)
    return rows


def run_forward(name, case):
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.weights import PROTOTYPE_TCONV_FAN
    lam, sd = build_reference(case)
    cfg = case["cfg"]
    batch = make_episode(**case["episode"])
    c = batch["flag_examples"].shape[2]
    rows = fixed_rows(lam, case, c)
    calls = []
    md = lam.mask_decoder
    orig = md._classify

    def spy(query_embeddings, class_embeddings, flag_examples):
        out = orig(query_embeddings, class_embeddings, flag_examples)
        calls.append((query_embeddings.detach().clone(), class_embeddings.detach().clone(), out.detach().clone()))
        return out

    md._classify = spy
    with torch.no_grad():
        seg_low, _ = lam._forward(batch)
        n_calls = len(calls)
        ref = lam(batch)
    md._classify = orig
    assert n_calls == 1, n_calls
    feat, protos, seg = calls[0]
    assert torch.equal(seg, seg_low)
    b, cf, h, w = feat.shape
    assert cf == cfg.class_width
    tensors = {
        "low_res_logits": seg_low.contiguous(),
        "logits": ref["logits"].contiguous(),
        "argmax": ref["logits"].argmax(dim=1).to(torch.uint8).contiguous(),
    }
    if rows is not None:
        tensors["selected_rows"] = rows
    path = os.path.join(GOLDEN, f"{name}.safetensors")
    save_file(tensors, path)
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "grid": int(h // 4),
            "classification_layer_downsample_rate": cfg.classification_layer_downsample_rate,
            "conv_classification": cfg.conv_classification, "class_width": int(cf),
            "reference_shapes": {k: list(v.shape) for k, v in lam.state_dict().items()},
            "scale": {"low_res_logits": float(seg_low.abs().max()), "low_res_logits_rms": float(seg_low.pow(2).mean().sqrt()),
                      "features": float(feat.abs().max()), "prototypes": float(protos.abs().max())},
            "torch": torch.__version__, "generated_by": "tools/make_golden_convcls.py"}
    sizes = [os.path.getsize(path)]
    if cfg.conv_classification:
        keep = min(h, FEATURE_BYTES // (4 * cf * w * b))
        feat_rows = feat[:, :, :keep].permute(0, 2, 3, 1).contiguous()          # (B, rows, W, cf) NHWC
        fpath = os.path.join(GOLDEN, f"{name}_feat.safetensors")
        save_file({"feature_rows": feat_rows, "prototypes": protos.contiguous()}, fpath)
        sizes.append(os.path.getsize(fpath))
        meta["feature_rows"] = int(keep)
        meta["prototype_tconv_init"] = {"std": float((PROTOTYPE_TCONV_FAN * cf) ** -0.5), "fan": PROTOTYPE_TCONV_FAN * int(cf),
                                        "measured_std": float(sd["mask_decoder.prototype_tconv.0.weight"].std())}
    with open(os.path.join(GOLDEN, f"{name}.json"), "w") as fh:
        json.dump(meta, fh, indent=1, default=list)
    print(f"[{name}] cf {cf} map {h} x {w} bytes {sizes} scale {meta['scale']}")


def grads_of(case, gt, double: bool):
    from label_anything.experiment.utils import WrapperModule
    from label_anything.loss import LabelAnythingLoss
    from labelanything_amd.episodes import make_episode
    lam, sd = build_reference(case)
    lam.train()
    batch = make_episode(**case["episode"])
    if double:
        lam.double()
        batch = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}
    fixed_rows(lam, case, batch["flag_examples"].shape[2])
    model = WrapperModule(lam, LabelAnythingLoss({"focal": {"weight": 1.0}}, class_weighting=True))
    res = model(batch, gt)
    loss = res["loss"]["value"]
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in lam.named_parameters()}
    assert all(k in sd for k in grads)
    return float(loss), grads


def run_train(name, case, seed_gt, full, tconv, tconv_rows):
    from labelanything_amd.episodes import make_episode
    from tests.helpers import make_gt
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=seed_gt)
    loss32, g32 = grads_of(case, gt, double=False)
    loss64, g64 = grads_of(case, gt, double=True)
    assert sorted(k for k, g in g32.items() if g is not None) == sorted(k for k, g in g64.items() if g is not None)
    keys = sorted(k for k, g in g32.items() if g is not None)
    assert all(k in keys for k in tconv)
    gmax = max(float(g64[k].abs().max()) for k in keys)
    kink = {k: float((g32[k].double() - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-2 * gmax) for k in keys}
    e_kink = max(kink.values())
    # (the ground truth is not stored: tests rebuild it with make_gt(seed_gt), as test_gradients_match_oracle_autograd does)
    out = {"loss": torch.tensor([loss32]), "grad_norm": torch.stack([g32[k].norm() for k in keys]),
           "grad_max": torch.stack([g32[k].abs().max() for k in keys])}
    for k in full:
        out["grad." + k] = g32[k].contiguous()
    for k in tconv:
        out["grad." + k] = g32[k][:tconv_rows].contiguous()
    path = os.path.join(GOLDEN, f"{name}_train.safetensors")
    save_file(out, path)
    with open(os.path.join(GOLDEN, f"{name}_train.json"), "w") as fh:
        json.dump({"keys": keys, "dead": sorted(k for k, g in g32.items() if g is None), "loss": loss32, "loss_fp64": loss64, "e_kink": e_kink,
                   "e_kink_worst_tensor": max(kink, key=kink.get), "seed_gt": seed_gt, "sliced": {k: tconv_rows for k in tconv},
                   "torch": torch.__version__, "generated_by": "tools/make_golden_convcls.py"}, fh, indent=1)
    print(f"[{name} train] loss {loss32:.8f} (fp64 {loss64:.8f}) e_kink {e_kink:.3e} at {max(kink, key=kink.get)} tensors {len(keys)} "
          f"bytes {os.path.getsize(path)}")


def main():
    from tests.cases_convcls import CC_CASES, CC_TRAIN, CC_TRAIN_PLAIN, CC_TRAIN_FULL, CC_TCONV, CC_TCONV_ROWS
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    for name, case in CC_CASES.items():
        if a.only in (None, name):
            run_forward(name, case)
    if not a.no_train and a.only in (None, CC_TRAIN["case"]):
        run_train(CC_TRAIN["case"], CC_CASES[CC_TRAIN["case"]], CC_TRAIN["seed_gt"], CC_TRAIN_FULL, CC_TCONV, CC_TCONV_ROWS)
    if not a.no_train and a.only in (None, CC_TRAIN_PLAIN["case"]):
        run_train(CC_TRAIN_PLAIN["case"], CC_CASES[CC_TRAIN_PLAIN["case"]], CC_TRAIN_PLAIN["seed_gt"], CC_TRAIN_FULL, [], 0)


if __name__ == "__main__":
    main()
