#!/usr/bin/env python
"""Golden vectors of the per-example family (``segment_example_logits`` / ``embeddings_per_example``) from the REFERENCE (build
container only; builds on tools/make_golden.py's stub finder):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_multi_embedding.py [--only NAME] [--no-train]

For every case of tests/cases_multi_embedding.py the seeded weights (``init_state_dict`` - the per-example family adds no parameter, the
state dict strict-loads) go into ``_build_lam(..., embeddings_per_example=..., segment_example_logits=...)``, the seeded episode runs
through the reference's ``Lam.forward`` on CPU / fp32 and the reference's OUTPUTS are written to
tests/golden/multi_embedding_<case>.safetensors: class_examples_embeddings, the repeated flag_examples, low_res_logits, logits, argmax,
and - for the torch restatement of the changed steps in tests/multi_embedding_ref.py - the operands of the final classification (the
class_mlp output and every second row / column of the upscaled query features).

For ``ME_TRAIN`` one decoder-only training step (WrapperModule + focal loss, as tools/make_golden_train.py) is stored as
multi_embedding_<case>_train: loss, per-tensor gradient norms, a handful of full gradients.  The maximum over examples is a kink: the
same backward is run in float64 (``lam.double()``) and ``e_kink`` - the worst per-tensor difference between the reference's own fp32 and
fp64 gradients, relative to the tensor's scale floored at 1e-2 of the model's largest gradient - goes into the json beside the
statistics of the reference's top-2 gap over the examples.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tools.make_golden as MG          # noqa: E402  (installs the stub finder, puts the reference first on sys.path)

import torch                            # noqa: E402
from safetensors.torch import save_file  # noqa: E402
from label_anything.models.build_lam import _build_lam   # noqa: E402  (the reference)

GOLDEN = os.path.join(ROOT, "tests", "golden")
FEATURE_STRIDE = 2                      # upscaled query features are kept at every second row / column (131 KB instead of 524 KB)


def build_reference(case):
    from labelanything_amd.weights import init_state_dict
    cfg = case["cfg"]
    assert cfg.encoder_spec is None, "decoder-only cases"
    lam = _build_lam(
        build_vit=None, use_vit=False, image_embed_dim=cfg.image_embed_dim, embed_dim=cfg.embed_dim, image_size=cfg.image_size,
        class_attention=cfg.class_attention, example_attention=cfg.example_attention, example_class_attention=cfg.example_class_attention,
        spatial_convs=cfg.spatial_convs, class_encoder=dict(cfg.class_encoder) if cfg.class_encoder else None,
        custom_preprocess=cfg.custom_preprocess,
        # handed over UNRESOLVED where the case is segment_example_logits alone, so that the reference's own builder resolves them
        segment_example_logits=cfg.segment_example_logits, embeddings_per_example=cfg.embeddings_per_example if cfg.pool_side > 1 else None)
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


def gap_stats(protos, feats, flags):
    """Top-2 gap of the reference's per-example logits over the valid examples, relative to the logit scale."""
    b, nc, cf = protos.shape
    n, c = flags.shape[1], flags.shape[2]
    per = torch.einsum("btf,bfp->btp", protos.double(), feats.double().flatten(2)).view(b, n, c, -1)
    per = per.masked_fill(flags.logical_not().unsqueeze(-1), float("-inf"))
    top = per.topk(2, dim=1).values
    gap = (top[:, 0] - top[:, 1])
    gap = gap[torch.isfinite(gap)]
    scale = float(per[torch.isfinite(per)].abs().max())
    return {"logit_scale": scale, "gap_below_1e-4": float((gap < 1e-4 * scale).double().mean()),
            "gap_below_1e-5": float((gap < 1e-5 * scale).double().mean())}


def run_forward(name, case):
    from labelanything_amd.episodes import make_episode
    lam, _ = build_reference(case)
    batch = make_episode(**case["episode"])
    c = batch["flag_examples"].shape[2]
    rows = fixed_rows(lam, case, c)
    seen = {}
    md = lam.mask_decoder
    orig = md._classify

    def spy(query_embeddings, class_embeddings, flag_examples):
        seen["features"], seen["protos"], seen["flags"] = query_embeddings.detach().clone(), class_embeddings.detach().clone(), flag_examples
        return orig(query_embeddings, class_embeddings, flag_examples)

    md._classify = spy
    with torch.no_grad():
        seg_low, pe_result = lam._forward(batch)
        ref = lam(batch)
    md._classify = orig
    k = case["cfg"].pool_side
    m = batch["flag_examples"].shape[1]
    cee = ref["class_examples_embeddings"]
    assert tuple(cee.shape) == (1, m * k * k, c, case["cfg"].embed_dim), cee.shape
    flags = pe_result["flag_examples"]
    assert tuple(flags.shape) == tuple(cee.shape[:3])
    tensors = {
        "class_examples_embeddings": cee.contiguous(),
        "flag_examples": flags.to(torch.uint8).contiguous(),
        "low_res_logits": seg_low.contiguous(),
        "logits": ref["logits"].contiguous(),
        "argmax": ref["logits"].argmax(dim=1).to(torch.uint8).contiguous(),
        "protos": seen["protos"].contiguous(),
        "features_s2": seen["features"][:, :, ::FEATURE_STRIDE, ::FEATURE_STRIDE].contiguous(),
    }
    if rows is not None:
        tensors["selected_rows"] = rows
    path = os.path.join(GOLDEN, f"multi_embedding_{name}.safetensors")
    save_file(tensors, path)
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "pool_side": k,
            "examples": int(cee.shape[1]), "decoder_tokens": int(cee.shape[1] * c), "feature_stride": FEATURE_STRIDE,
            "top2_gap": gap_stats(seen["protos"], seen["features"], flags.bool()),
            "nan_fraction_of_invalid_classes": float(torch.isnan(ref["logits"]).double().mean()),
            "torch": torch.__version__, "generated_by": "tools/make_golden_multi_embedding.py"}
    with open(os.path.join(GOLDEN, f"multi_embedding_{name}.json"), "w") as fh:
        json.dump(meta, fh, indent=1, default=list)
    print(f"[{name}] examples {cee.shape[1]} tokens {cee.shape[1] * c} bytes {os.path.getsize(path)} gap {meta['top2_gap']}")


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


def run_train(name, case, seed_gt, full):
    from labelanything_amd.episodes import make_episode
    from tests.helpers import make_gt
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=seed_gt)
    loss32, g32 = grads_of(case, gt, double=False)
    loss64, g64 = grads_of(case, gt, double=True)
    keys = sorted(k for k, g in g32.items() if g is not None)
    assert keys == sorted(k for k, g in g64.items() if g is not None)
    gmax = max(float(g64[k].abs().max()) for k in keys)
    kink = {k: float((g32[k].double() - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-2 * gmax) for k in keys}
    e_kink = max(kink.values())
    # (the ground truth is not stored: tests rebuild it with make_gt(seed_gt), as test_gradients_match_oracle_autograd does)
    out = {"loss": torch.tensor([loss32]), "grad_norm": torch.stack([g32[k].norm() for k in keys])}
    for k in full:
        out["grad." + k] = g32[k].contiguous()
    path = os.path.join(GOLDEN, f"multi_embedding_{name}_train.safetensors")
    save_file(out, path)
    with open(os.path.join(GOLDEN, f"multi_embedding_{name}_train.json"), "w") as fh:
        json.dump({"keys": keys, "dead": sorted(k for k, g in g32.items() if g is None), "loss": loss32, "loss_fp64": loss64, "e_kink": e_kink,
                   "e_kink_worst_tensor": max(kink, key=kink.get), "seed_gt": seed_gt, "torch": torch.__version__,
                   "generated_by": "tools/make_golden_multi_embedding.py"}, fh, indent=1)
    print(f"[{name} train] loss {loss32:.8f} (fp64 {loss64:.8f}) e_kink {e_kink:.3e} at {max(kink, key=kink.get)} tensors {len(keys)} "
          f"bytes {os.path.getsize(path)}")


def main():
    from tests.cases_multi_embedding import ME_CASES, ME_TRAIN, ME_TRAIN_FULL
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    for name, case in ME_CASES.items():
        if a.only in (None, name):
            run_forward(name, case)
    if not a.no_train and a.only in (None, ME_TRAIN["case"]):
        run_train(ME_TRAIN["case"], ME_CASES[ME_TRAIN["case"]], ME_TRAIN["seed_gt"], ME_TRAIN_FULL)


if __name__ == "__main__":
    main()
