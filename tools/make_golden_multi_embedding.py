#!/usr/bin/env python
"""Golden vectors of the per-example family (``segment_example_logits`` / ``embeddings_per_example``) from the REFERENCE (build
container only; tools/golden_lib.py imports it):

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
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

import torch                            # noqa: E402
from tests.cases_multi_embedding import ME_CASES, ME_TRAIN, ME_TRAIN_FULL   # noqa: E402

FEATURE_STRIDE = 2                      # upscaled query features are kept at every second row / column (131 KB instead of 524 KB)


def option(case):
    """What ``_build_lam`` is given beyond the plain model: handed over UNRESOLVED where the case is segment_example_logits alone, so
    that the reference's own builder resolves them."""
    cfg = case["cfg"]
    return {"segment_example_logits": cfg.segment_example_logits,
            "embeddings_per_example": cfg.embeddings_per_example if cfg.pool_side > 1 else None}


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
    lam, _, batch, rows = GL.reference_episode(case, **option(case))
    calls = GL.spy_classify(lam)
    with torch.no_grad():
        seg_low, pe_result = lam._forward(batch)
        ref = lam(batch)
    features, protos, _ = calls[-1]
    k = case["cfg"].pool_side
    _, m, c = batch["flag_examples"].shape
    cee = ref["class_examples_embeddings"]
    assert tuple(cee.shape) == (1, m * k * k, c, case["cfg"].embed_dim), cee.shape
    flags = pe_result["flag_examples"]
    assert tuple(flags.shape) == tuple(cee.shape[:3])
    tensors = {
        "class_examples_embeddings": cee.contiguous(),
        "flag_examples": flags.to(torch.uint8).contiguous(),
        **GL.logit_tensors(seg_low, ref),
        "protos": protos.contiguous(),
        "features_s2": features[:, :, ::FEATURE_STRIDE, ::FEATURE_STRIDE].contiguous(),
    }
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "pool_side": k,
            "examples": int(cee.shape[1]), "decoder_tokens": int(cee.shape[1] * c), "feature_stride": FEATURE_STRIDE,
            "top2_gap": gap_stats(protos, features, flags.bool()),
            "nan_fraction_of_invalid_classes": float(torch.isnan(ref["logits"]).double().mean())}
    size = GL.write_fixture(f"multi_embedding_{name}", tensors, meta, rows)
    print(f"[{name}] examples {cee.shape[1]} tokens {cee.shape[1] * c} bytes {size} gap {meta['top2_gap']}")


def train():
    name = ME_TRAIN["case"]
    step = GL.run_train(ME_CASES[name], ME_TRAIN["seed_gt"], **option(ME_CASES[name]))
    GL.write_train(f"multi_embedding_{name}", step, ME_TRAIN_FULL, "e_kink")


if __name__ == "__main__":
    GL.main(ME_CASES, run_forward, [(ME_TRAIN["case"], train)])
