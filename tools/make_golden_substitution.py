#!/usr/bin/env python
"""Golden vectors for query substitution: the REFERENCE's ``Substitutor`` (experiment/substitution.py) is imported and run on CPU
over synthetic dataset batches (prompts for all M+1 images, ground truths [B, M+1, H, W]), with seeded synthetic logits fed to
``generate_new_points`` after every step.  ``torch.randint`` is wrapped by a recorder that calls the real function, so the ranks the
reference drew are stored next to its outputs.  Stored in tests/golden/substitution.{safetensors,json}: every case's inputs, the
logits (small integers, stored as int8) and ranks of each step, and each step's model input and query ground truth.

Where the reference's row key ``b * B + c`` (substitution.py:83) is not injective (B >= 2 and C > B) its points can land on other
(b, c) than the draws were made for; the tests compare those cases against a host restatement instead (tests/test_substitution_gpu.py).

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_substitution.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tools.golden_lib            # noqa: E402,F401  (installs the stub finder, puts the reference first)

import torch                            # noqa: E402
from safetensors.torch import save_file  # noqa: E402

# name: B, M+1, C, (H, W) frame, num_points, substitute, dims rule, long side, custom_preprocess
CASES = {
    "b1_m2_c2_n0":      dict(B=1, M1=2, C=2, H=9, W=11, n=0, sub=True, dims="full"),
    "b2_m3_c3_n0":      dict(B=2, M1=3, C=3, H=10, W=12, n=0, sub=True, dims="ragged"),
    "b2_m6_c6_n0":      dict(B=2, M1=6, C=6, H=8, W=9, n=0, sub=True, dims="ragged", no_intended=True),
    "b1_m4_c4_nosub":   dict(B=1, M1=4, C=4, H=8, W=8, n=1, sub=False, dims="full"),
    "b1_m4_c5_n1":      dict(B=1, M1=4, C=5, H=12, W=10, n=1, sub=True, dims="ragged", empty=True),
    "b1_m6_c6_n1":      dict(B=1, M1=6, C=6, H=10, W=13, n=1, sub=True, dims="half", empty=True),
    "b2_m3_c3_n1":      dict(B=2, M1=3, C=3, H=11, W=9, n=1, sub=True, dims="ragged", empty=True),
    "b2_m2_c2_n3":      dict(B=2, M1=2, C=2, H=12, W=12, n=3, sub=True, dims="half"),
    "b1_m3_c4_n3":      dict(B=1, M1=3, C=4, H=10, W=14, n=3, sub=True, dims="ragged", long_side=480, custom=False),
    "b2_m4_c4_n1_nonin": dict(B=2, M1=4, C=4, H=9, W=10, n=1, sub=True, dims="ragged", empty=True),
    "b2_m3_c6_n1_nonin": dict(B=2, M1=3, C=6, H=10, W=11, n=1, sub=True, dims="half"),
}

# original sizes whose preprocess shape lands on / near a .5 rounding at long side 1024 (333 * 0.5 = 166.5, 1365 * 0.5 = 682.5)
HALF_DIMS = [(333, 2048), (1365, 2048), (427, 640), (375, 500), (2048, 1365), (999, 2046)]


def make_batch(cfg, g):
    B, M1, C, H, W = cfg["B"], cfg["M1"], cfg["C"], cfg["H"], cfg["W"]
    P, Q, S = 2, 1, 4
    batch = {
        "embeddings": torch.randn(B, M1, 2, 2, 2, generator=g),
        "prompt_points": torch.randint(0, 50, (B, M1, C, P, 2), generator=g).float(),
        "flag_points": torch.randint(0, 2, (B, M1, C, P), generator=g).float(),
        "prompt_bboxes": torch.randint(0, 50, (B, M1, C, Q, 4), generator=g).float(),
        "flag_bboxes": torch.randint(0, 2, (B, M1, C, Q), generator=g).float(),
        "prompt_masks": torch.randint(0, 2, (B, M1, C, S, S), generator=g).float(),
        "flag_masks": torch.randint(0, 2, (B, M1, C), generator=g).float(),
        "flag_examples": torch.randint(0, 2, (B, M1, C), generator=g).bool(),
    }
    if cfg["dims"] == "half":
        rows = [HALF_DIMS[(b * M1 + m) % len(HALF_DIMS)] for b in range(B) for m in range(M1)]
        dims = torch.tensor(rows).view(B, M1, 2)
    elif cfg["dims"] == "ragged":
        dims = torch.stack([torch.randint(H // 2, H + 1, (B, M1), generator=g), torch.randint(W // 2, W + 1, (B, M1), generator=g)], -1)
        dims[:, 0] = torch.tensor([H, W])          # the frame is the largest image
    else:
        dims = torch.tensor([H, W]).expand(B, M1, 2).clone()
    batch["dims"] = dims
    batch["classes"] = [[[int(x) for x in torch.randperm(20, generator=g)[:2]] for _ in range(M1)] for _ in range(B)]
    batch["image_ids"] = [[100 * b + m for m in range(M1)] for b in range(B)]
    batch["intended_classes"] = None if cfg.get("no_intended") else [[[b, m] for m in range(M1)] for b in range(B)]
    # ground truths: classes 0 .. C-2 (class C-1 absent), -100 outside each image's dims and on a few scattered pixels
    gts = torch.randint(0, C - 1, (B, M1, H, W), generator=g)
    if cfg["dims"] == "ragged":
        for b in range(B):
            for m in range(M1):
                h, w = int(dims[b, m, 0]), int(dims[b, m, 1])
                gts[b, m, h:] = -100
                gts[b, m, :, w:] = -100
    gts[torch.rand(B, M1, H, W, generator=g) < 0.05] = -100
    return batch, gts


def make_logits(cfg, gt, g):
    """Small-integer logits (exact in every format; ties exercise the first-maximal-index rule): mostly right, some errors.  With
    ``empty`` the last class is never predicted, so it has no errors at all (absent from the ground truth too)."""
    B, C = cfg["B"], cfg["C"]
    gtc = gt.clone()
    gtc[gtc == -100] = 0
    lg = torch.randint(-3, 3, (B, C) + tuple(gt.shape[1:]), generator=g)
    lg.scatter_add_(1, gtc.unsqueeze(1), torch.full_like(gtc.unsqueeze(1), 3))
    if cfg.get("empty"):
        lg[:, C - 1] = -8
    else:     # class C-1 predicted somewhere although it is in no ground truth: false positives only
        lg[:, C - 1, 0, 0] = 9
    return lg.to(torch.int8)


class RandintRecorder:
    def __init__(self):
        self.real = torch.randint
        self.calls = []

    def __call__(self, *args, **kw):
        out = self.real(*args, **kw)
        self.calls.append((int(args[1]), out.clone()))
        return out


def ranks_from_calls(calls, logits, gt, n):
    """The recorded draws placed at their (b, c): the reference draws in the order of torch.unique over (b, c) with errors."""
    B, C = logits.shape[:2]
    g = gt.clone()
    g[g == -100] = 0
    p = logits.float().argmax(1)
    ranks = torch.zeros(B, C, n, dtype=torch.int32)
    keys = []
    for b in range(B):
        for c in range(C):
            cnt = int((((g[b] == c) | (p[b] == c)) & (g[b] != p[b])).sum())
            if cnt:
                keys.append((b, c, cnt))
    assert len(keys) == len(calls), (len(keys), len(calls))
    for (b, c, cnt), (high, out) in zip(keys, calls):
        assert high == cnt, (b, c, high, cnt)
        ranks[b, c] = out.to(torch.int32)
    return ranks


def run_case(name, cfg, tensors, meta):
    from label_anything.experiment import substitution as RS
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    batch, gts = make_batch(cfg, g)
    pre = f"{name}."
    for k, v in batch.items():
        if isinstance(v, torch.Tensor):
            tensors[pre + "in." + k] = v.clone()
    tensors[pre + "in.gts"] = gts.clone()
    sub = RS.Substitutor(num_points=cfg["n"], substitute=cfg["sub"], long_side_length=cfg.get("long_side", 1024),
                         custom_preprocess=cfg.get("custom", True))
    sub.reset(batch=({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}, gts.clone()))
    steps = []
    for i, (inp, gt) in enumerate(sub):
        sp = f"{pre}step{i}."
        for k, v in inp.items():
            if isinstance(v, torch.Tensor):
                tensors[sp + k] = v.clone()
        tensors[sp + "gt"] = gt.clone()
        steps.append({k: v for k, v in inp.items() if not isinstance(v, torch.Tensor)})
        if cfg["n"] > 0 and cfg["sub"]:
            logits = make_logits(cfg, gt, g)
            rec = RandintRecorder()
            torch.randint = rec
            try:
                before = sub.batch["prompt_points"].shape[3]
                sub.generate_new_points(logits.float(), gt)
            finally:
                torch.randint = rec.real
            ranks = ranks_from_calls(rec.calls, logits, gt, cfg["n"])
            tensors[sp + "logits"] = logits
            tensors[sp + "ranks"] = ranks
            tensors[sp + "new_points"] = sub.batch["prompt_points"][:, 0, :, before:].clone()
            tensors[sp + "new_labels"] = sub.batch["flag_points"][:, 0, :, before:].clone()
    B, C = cfg["B"], cfg["C"]
    # b * B + c is injective over the (b, c) grid when C <= B; with C = B + 1 the colliding rows (b, B) / (b + 1, 0) still come out in
    # order when both have errors (the sort keeps their torch.unique order) but not when (b, B) has none (its zero row is appended last)
    meta[name] = dict(cfg, steps=steps, injective=bool(B == 1 or C <= B))
    print(f"{name}: {len(steps)} steps, injective key {meta[name]['injective']}")


def main():
    tensors, meta = {}, {}
    for name, cfg in CASES.items():
        run_case(name, cfg, tensors, meta)
    out = os.path.join(ROOT, "tests", "golden", "substitution")
    tensors = {k: v.contiguous() for k, v in tensors.items()}
    save_file(tensors, out + ".safetensors")
    with open(out + ".json", "w") as f:
        json.dump({"cases": meta, "half_dims": HALF_DIMS}, f, indent=1, sort_keys=True)
    print("wrote", out + ".safetensors", os.path.getsize(out + ".safetensors"), "bytes")


if __name__ == "__main__":
    main()
