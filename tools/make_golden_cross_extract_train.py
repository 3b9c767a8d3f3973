#!/usr/bin/env python
"""Training fixtures of ``embedding_extraction="cross_attention"`` from the REFERENCE (build container only; tools/golden_lib.py
imports it):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_cross_extract_train.py [--only NAME] [--no-write]

For every entry of ``XE_TRAIN`` (tests/cases_cross_extract_train.py) the reference's model of the case runs one training step in train
mode - focal objective with class weighting, fp32 and fp64 (``GL.run_train``).  In train mode EmbeddingTransformer.forward drops learned
queries with draws from the host generator (prompt_encoder.py:301-307); a forward pre-hook on the module seeds that generator with
``keep_seed`` right before, so the fp32 and the fp64 run, and a test that calls ``draw_extraction_keep`` under the same seed, see the same
mask.  tests/golden/cross_extract_<case>_train.safetensors holds the loss, the per-tensor gradient norms, ``extraction_keep``, the
returned ``flag_examples``, ``selected_rows``, the full gradients of
``XE_TRAIN_FULL`` and the first ``XE_TRAIN_SLICED_ROWS`` rows of the 2048-wide MLP weights' gradients; cross_extract_<case>_train_logits.safetensors the train-mode ``logits`` (with a dropped query they differ from the eval
fixture's; a file of their own keeps both below the size limit of a committed file); the json the live and dead tensors,
the reference's own fp32-vs-fp64 gradient error ``e_ref32`` and the conditions below as measured.  The existing fixtures of
tools/make_golden_cross_extract.py are not touched (``GL.main`` is given an empty case table).

A fixture is refused unless: the mask drops a query and keeps one; 4 e_ref32 <= 3e-4; the dead tensors are exactly the ones dead without the extraction
(the prompt transformer's final attention, embeddings of prompt types the episode lacks) plus the four norm3 of the extraction; the gradient norms of ``XE_MUST_BE_ABOVE`` lie above 1e-2 of the largest norm, as do at least
29 of the 33 live extraction tensors and, of the prompt-encoder tensors upstream of the extraction, as many as ``XE_MIN_UPSTREAM_ABOVE``
asks for the case (80 of 101 on x4).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

import torch                            # noqa: E402
from tests.cases_cross_extract import XE_CASES   # noqa: E402
from tests.cases_cross_extract_train import (EX, XE_FLOOR, XE_GRAD_TOL, XE_MIN_LIVE_EXTRACTION_ABOVE, XE_MIN_UPSTREAM_ABOVE,   # noqa: E402
                                             XE_MUST_BE_ABOVE, XE_TRAIN, XE_TRAIN_FULL, XE_TRAIN_SLICED, XE_TRAIN_SLICED_ROWS)

EVAL_DEAD = ("prompt_encoder.transformer.final_attn_token_to_image.", "prompt_encoder.transformer.norm_final_attn.")
UNUSED_PROMPT_TYPES = ("prompt_encoder.no_mask_embed.", "prompt_encoder.no_sparse_embedding.", "prompt_encoder.point_embeddings.",
                       "prompt_encoder.not_a_point_embed.", "prompt_encoder.not_a_mask_embed.", "prompt_encoder.mask_downscaling.")


def option(case):
    cfg = case["cfg"]
    return dict(embedding_extraction="cross_attention", segment_example_logits=cfg.segment_example_logits,
                embeddings_per_example=cfg.embeddings_per_example if cfg.embeddings_per_example > 1 else None)


def watcher(keep_seed):
    """-> watch(lam): seeds the host generator before the extraction module's forward; records the flags it returns and the logits."""
    def watch(lam):
        seen = {}
        module = lam.prompt_encoder.embedding_extraction
        module.register_forward_pre_hook(lambda mod, args: torch.manual_seed(keep_seed) and None)
        module.register_forward_hook(lambda mod, args, out: seen.update(
            flags=next(v for k, v in out.items() if v.dim() == 3).detach().clone()))
        lam.register_forward_hook(lambda mod, args, out: seen.update(logits=out["logits"].detach().clone()))
        return seen
    return watch


def train(spec):
    name = spec["case"]
    case = XE_CASES[name]
    n = int(case["cfg"].embeddings_per_example)
    step = GL.run_train(case, spec["seed_gt"], watch=watcher(spec["keep_seed"]), **option(case))
    flags32, flags64 = step.watched32["flags"], step.watched64["flags"]
    assert torch.equal(flags32, flags64), "the fp32 and the fp64 run drew different masks"
    valid = flags32.any(dim=1)                                         # (B, C): classes some support shows
    assert bool(valid.any())
    b_, c_ = [int(v) for v in valid.nonzero()[0]]
    keep = flags32[b_, :, c_].bool()                                   # the mask, read off a valid class
    assert torch.equal(flags32.bool(), valid[:, None, :] & keep[None, :, None])
    torch.manual_seed(spec["keep_seed"])
    assert torch.equal(keep, torch.rand(n) > 0.2), "the mask is not the rule's under keep_seed"
    assert bool(keep.any()) and not bool(keep.all()), f"{name}: keep {keep.tolist()} must drop a query and keep one"
    # dead: what the forward never reaches without the extraction either (the prompt transformer's final attention, and the embeddings of
    # prompt types the episode does not use) plus exactly the four norm3 of the extraction
    norm3 = sorted(f"{EX}layers.{l}.norm3.{p}" for l in range(2) for p in ("weight", "bias"))
    assert sorted(k for k in step.dead if k.startswith(EX)) == norm3, step.dead
    rest = [k for k in step.dead if not k.startswith(EX)]
    assert sorted(k for k in rest if k.startswith(EVAL_DEAD)) == sorted(k for k in step.g32 if k.startswith(EVAL_DEAD))
    assert all(k.startswith(EVAL_DEAD + UNUSED_PROMPT_TYPES) for k in rest), rest
    keys = step.keys
    norms = {k: float(step.g64[k].norm()) for k in keys}
    floor = XE_FLOOR * max(norms.values())
    low = [k for k in XE_MUST_BE_ABOVE if norms[k] <= floor]
    assert not low, f"{name}: gradient norms at or below the comparison floor: {low}"
    live_ex = [k for k in keys if k.startswith(EX)]
    assert len(live_ex) == 33, len(live_ex)
    ex_above = sum(norms[k] > floor for k in live_ex)
    upstream = [k for k in keys if k.startswith("prompt_encoder.") and not k.startswith(EX)]
    up_above = sum(norms[k] > floor for k in upstream)
    assert ex_above >= XE_MIN_LIVE_EXTRACTION_ABOVE, (ex_above, sorted((norms[k] / max(norms.values()), k) for k in live_ex)[:6])
    assert (len(upstream), up_above >= XE_MIN_UPSTREAM_ABOVE[name][1]) == (XE_MIN_UPSTREAM_ABOVE[name][0], True), (len(upstream), up_above)
    g32, g64 = step.g32, step.g64
    gmax = max(float(g64[k].abs().max()) for k in keys)
    e_ref32 = max(float((g32[k].double() - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-2 * gmax) for k in keys)
    assert 4 * e_ref32 <= XE_GRAD_TOL, f"{name}: 4 e_ref32 = {4 * e_ref32:.2e} exceeds {XE_GRAD_TOL:.0e}"
    tensors = {"extraction_keep": keep.to(torch.uint8), "flag_examples": flags32.to(torch.uint8).contiguous()}
    GL.write_fixture(f"cross_extract_{name}_train_logits", {"logits": step.watched32["logits"].contiguous()}, None)
    tensors.update({"grad." + k: g32[k][:XE_TRAIN_SLICED_ROWS].contiguous() for k in XE_TRAIN_SLICED})
    meta = {"case": name, "weight_seed": case["weight_seed"], "keep_seed": spec["keep_seed"], "extraction_keep": keep.tolist(),
            "embedding_dropout": 0.2, "sliced": {k: XE_TRAIN_SLICED_ROWS for k in XE_TRAIN_SLICED},
            "floor": XE_FLOOR, "norm_over_largest": {k: norms[k] / max(norms.values()) for k in XE_MUST_BE_ABOVE},
            "live_extraction_tensors": len(live_ex), "live_extraction_above_floor": int(ex_above),
            "upstream_tensors": len(upstream), "upstream_above_floor": int(up_above), "four_e_ref32": 4 * e_ref32, "grad_tol": XE_GRAD_TOL}
    GL.write_train(f"cross_extract_{name}", step, XE_TRAIN_FULL, "e_ref32", tensors=tensors, meta=meta, rows=step.rows)
    print(f"[{name} train] keep {keep.tolist()} extraction above floor {ex_above}/33 upstream {up_above}/{len(upstream)} 4 e_ref32 {4 * e_ref32:.2e}")


if __name__ == "__main__":
    GL.main({}, None, [(spec["case"], (lambda spec=spec: train(spec))) for spec in XE_TRAIN])
