#!/usr/bin/env python
"""Times the cosine-similarity segmenter (labelanything_amd.similarity, csrc/similarity.hip) against this tool's own eager restatement of
the reference's op sequence (models/similarity.py:122-195) in fp32 and under fp16 autocast, on the same GPU, in one call, alternating.

    python tools/bench_similarity.py [--out FILE] [--rounds 5] [--supports 1 5]

Configuration: the cosine.yaml recipe - image_size 480, compare_size 128, 30 x 30 embeddings of width 768 - with two classes (box masks at
256 x 256) and M1 = 1 and 5 support images.  Every arm is warmed up, then timed ``rounds`` times in turn (fused, fp16, fp32, fused, ...),
each window at least --window seconds of device events; the figures are per forward.  ``la_sim_max`` alone is timed the same way: its
rate is 2 Q K D flops over that time, its share of the 2.5 PFLOP/s fp16 peak beside it.  The fused logits are checked against the fp32
arm before anything is timed.  One JSON line per M1, also appended to --out.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from labelanything_amd import _lib as L                           # noqa: E402
from labelanything_amd.similarity import build_similarity        # noqa: E402

PEAK_F16 = 2.5e15
CS, D, G, N, S, HM = 128, 768, 30, 2, 480, 256


def episode(m1, seed=0):
    gen = torch.Generator().manual_seed(seed)
    emb = torch.randn(1, m1 + 1, D, G, G, generator=gen)
    masks = torch.zeros(1, m1, N, HM, HM)
    for j in range(m1):
        y0, x0 = (int(v) for v in torch.randint(0, HM // 2, (2,), generator=gen))
        h, w = (int(v) for v in torch.randint(HM // 4, HM // 2, (2,), generator=gen))
        masks[0, j, 1, y0:y0 + h, x0:x0 + w] = 1.0
    dims = torch.tensor([[[375, 500]] + [[480, 480]] * m1])
    return {"embeddings": emb.cuda(), "prompt_masks": masks.cuda(), "dims": dims}


def eager_compare_logits(batch):
    """models/similarity.py:122-192, op for op (einops spelled as reshapes)."""
    emb = batch["embeddings"]
    b, m, d, _, _ = emb.shape
    emb = F.interpolate(emb.flatten(0, 1), size=(CS, CS), mode="bicubic", align_corners=False).view(b, m, d, CS, CS)
    q = F.normalize(emb[:, 0], dim=1).flatten(2).transpose(1, 2)
    s = F.normalize(emb[:, 1:], dim=2).flatten(3).transpose(2, 3)
    pm = batch["prompt_masks"]
    _, m1, n, hm, wm = pm.shape
    pm = F.interpolate(pm.reshape(b * m1 * n, 1, hm, wm), size=(CS, CS), mode="nearest").reshape(b, m1, n, CS * CS)
    sim = torch.einsum("bqd,bmkd->bqmk", q, s)
    pm[:, :, 0, :] = (pm[:, :, 1:, :].sum(dim=2) == 0).float()
    logits = []
    for c in range(n):
        masked = sim.masked_fill(pm[:, :, c, :].unsqueeze(1) == 0, float("-inf"))
        logits.append(masked.view(b, sim.shape[1], -1).max(dim=-1).values)
    return torch.stack(logits, dim=1).view(b, n, CS, CS)


def eager_forward(batch):
    """+ postprocess_masks (:33-103) for one query without custom_preprocess."""
    logits = eager_compare_logits(batch).float()
    logits = F.interpolate(logits, (S, S), mode="bilinear", align_corners=False)
    oh, ow = (int(v) for v in batch["dims"][0, 0])
    hmax, wmax = int(batch["dims"][..., 0].max()), int(batch["dims"][..., 1].max())
    logits = F.interpolate(logits, (oh, ow), mode="bilinear", align_corners=False)
    logits = F.pad(logits, (0, wmax - ow, 0, hmax - oh), value=float("-inf"))
    logits[:, 0][logits[:, 0] == float("-inf")] = 0
    return logits


def timed(fn, window):
    """Mean seconds per call over a window of at least ``window`` seconds of device time."""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, total = 1, 0.0
    while True:
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        total = start.elapsed_time(stop) * 1e-3
        if total >= window:
            return total / n
        n = max(n + 1, int(n * 1.2 * window / max(total, 1e-6)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--supports", type=int, nargs="+", default=[1, 5])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_similarity: needs the GPU (there is no fallback)")
    model = build_similarity(image_size=S, compare_size=CS)
    for m1 in a.supports:
        batch = episode(m1)

        def fused():
            return model(batch)["logits"]

        def eager16():
            with torch.autocast("cuda", dtype=torch.float16):
                return eager_forward(batch)

        def eager32():
            return eager_forward(batch)

        # the kernel alone: random unit rows of the model's shapes, the episode's class words
        q, k = CS * CS, m1 * CS * CS
        q16 = F.normalize(torch.randn(1, q, D, device="cuda"), dim=2).half()
        k16 = F.normalize(torch.randn(1, k, D, device="cuda"), dim=2).half()
        bits = torch.empty(m1, CS * CS, device="cuda", dtype=torch.int32)
        L.sim_class_bits(batch["prompt_masks"].view(m1, N, HM, HM), CS, bits)
        ksplit, floats = L.sim_max_plan(1, q, k, D, N)
        work, out = torch.empty(max(floats, 1), device="cuda"), torch.empty(1, N, q, device="cuda")

        def kernel():
            L.sim_max(q16, k16, bits.view(1, k), N, out, work=work)

        with torch.no_grad():
            want, got = eager_compare_logits(batch), model.compare_logits(batch)
            err = float((got - want).abs().max() / want.abs().max())
            assert torch.equal(torch.isfinite(got), torch.isfinite(want)) and err <= 1e-3, err
            err16 = float((eager_forward(batch) - fused()).abs().nan_to_num(0.0).max())
            arms = {"fused": fused, "eager_fp16": eager16, "eager_fp32": eager32, "la_sim_max": kernel}
            for fn in arms.values():
                fn()
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name in arms}
            for _ in range(a.rounds):
                for name, fn in arms.items():
                    times[name].append(timed(fn, a.window))
        flops = 2.0 * q * k * D
        res = {"bench": "similarity", "supports": m1, "compare_size": CS, "width": D, "classes": N, "key_split": ksplit,
               "compare_logits_rel_err_vs_eager_fp32": err, "final_logits_abs_err_vs_eager_fp32": err16, "rounds": a.rounds,
               **{f"{name}_ms": {"min": min(t) * 1e3, "median": sorted(t)[len(t) // 2] * 1e3, "max": max(t) * 1e3} for name, t in times.items()}}
        res["fused_over_eager_fp16"] = sorted(times["eager_fp16"])[len(times["eager_fp16"]) // 2] / sorted(times["fused"])[len(times["fused"]) // 2]
        res["fused_ahead_of_fp16_beyond_spread"] = max(times["fused"]) < min(times["eager_fp16"])
        kt = sorted(times["la_sim_max"])[len(times["la_sim_max"]) // 2]
        res["la_sim_max_tflops"] = flops / kt * 1e-12
        res["la_sim_max_share_of_fp16_peak"] = flops / kt / PEAK_F16
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(line + "\n")
        del batch, q16, k16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
