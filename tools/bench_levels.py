#!/usr/bin/env python
"""The two-level classification head on the MI355X: device time of

  level_reduce   la_level_reduce alone (reads the fine logits and the coarse logits, writes the result);
  classify       la_classify alone (the fine logits from the 32-channel features);
  pair           la_classify followed by la_level_reduce - what classification_levels=2 runs in place of la_classify.  Fusing the two
                 would save one write and one read of 4 B C 16 g g bytes; this is the figure to weigh that against;
  wide           la_classify_wide (the coarse logits, D = 256; it reads 4 B g g D bytes, four times the head's traffic at 48 x 2 x 64 x 64);
  backward       la_level_reduce_bwd,

measured in ONE process with the variants' windows interleaved, at (B, C, g) = (48, 2, 64) and (8, 6, 30), and the decoder-only training
step (LamTrainer.step on cached embeddings) with classification_levels 2 against 1, alternating in the same way.  Every figure is the
median of --repeats windows of --iters launches after a warm-up, with the min - max spread beside it.  Bytes are the traffic model of
la_level_reduce: 4 B C (16 + 1) g g read, 4 B C 16 g g written; the fraction is of the 8.0 TB/s HBM3E peak.  One JSON line per measurement
goes to --out.

    python tools/bench_levels.py [--iters 50] [--repeats 7]
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                        # noqa: E402

from labelanything_amd import _lib as L             # noqa: E402

SHAPES = [dict(name="48x2_g64", b=48, c=2, g=64), dict(name="8x6_g30", b=8, c=6, g=30)]
HBM_PEAK = 8.0e12


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters        # us per call


def alternate(fns, iters, repeats, warm=5):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return out


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "windows": len(us)}


def bench_shape(s, iters, repeats, d=256, cf=32):
    b, c, g = s["b"], s["c"], s["g"]
    npix = 16 * g * g
    gen = torch.Generator().manual_seed(7)
    feat = torch.randn(b * npix, cf, generator=gen).cuda()
    protos = torch.randn(b, c, cf, generator=gen).cuda()
    tok = torch.randn(b, c, d, generator=gen).cuda()
    img = torch.randn(b * g * g, d, generator=gen).cuda()
    w = (0.3 * torch.randn(18, generator=gen)).cuda()
    bias = torch.zeros(1).cuda()
    cls0 = torch.empty(b, c, 4 * g, 4 * g, device="cuda")
    cls1 = torch.empty(b, c, g, g, device="cuda")
    seg = torch.empty_like(cls0)
    dseg = torch.randn(b, c, 4 * g, 4 * g, generator=gen).cuda()
    d0, d1 = torch.empty_like(cls0), torch.empty_like(cls1)
    dw, db = torch.zeros(18, device="cuda"), torch.zeros(1, device="cuda")
    L.classify(feat, protos, b, npix, c, cf, cls0)
    L.classify_wide(tok, img, b, g * g, c, d, cls1)
    fns = {
        "level_reduce": lambda: L.level_reduce(cls0, cls1, w, bias, b, c, g, g, seg),
        "classify": lambda: L.classify(feat, protos, b, npix, c, cf, cls0),
        "pair": lambda: (L.classify(feat, protos, b, npix, c, cf, cls0), L.level_reduce(cls0, cls1, w, bias, b, c, g, g, seg)),
        "wide": lambda: L.classify_wide(tok, img, b, g * g, c, d, cls1),
        "level_reduce_bwd": lambda: L.level_reduce_bwd(dseg, cls0, cls1, w, b, c, g, g, d0, d1, dw, db),
    }
    t = alternate(fns, iters, repeats)
    rd, wr = 4 * b * c * 17 * g * g, 4 * b * c * 16 * g * g
    med = statistics.median(t["level_reduce"])
    return {"what": "level_reduce", "shape": s, **{k: stats(v) for k, v in t.items()},
            "level_reduce_bytes": {"read": rd, "written": wr},
            "level_reduce_GBps": round((rd + wr) / med / 1e3, 1), "level_reduce_fraction_of_hbm_peak": round((rd + wr) / (med * 1e-6) / HBM_PEAK, 4),
            "intermediate_bytes_a_fused_kernel_would_save": 2 * wr,
            "wide_bytes_read": 4 * b * g * g * d, "wide_GBps": round(4 * b * g * g * d / statistics.median(t["wide"]) / 1e3, 1)}


def bench_step(iters, repeats, batch_size):
    """LamTrainer.step (decoder only, cached embeddings) for the tests' D = 256 geometry with classification_levels 2 against 1."""
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    from tests.cases_levels import LV_CASES
    from tests.helpers import make_gt
    case = LV_CASES["l2_noeca"]
    ep = {**case["episode"], "batch": batch_size}
    batch = make_episode(**ep)
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=17)
    fns = {}
    for levels in (2, 1):
        lam = Lam(dataclasses.replace(case["cfg"], classification_levels=levels), seed=3).cuda()
        lam.selected_rows = torch.arange(batch["flag_examples"].shape[2])
        tr = LamTrainer(lam)
        fns[f"levels_{levels}"] = (lambda tr=tr: tr.step(batch, gt))
    t = alternate(fns, iters, repeats, warm=3)
    return {"what": "decoder_only_training_step", "episode": ep, **{k: stats(v) for k, v in t.items()},
            "levels_2_over_1": round(statistics.median(t["levels_2"]) / statistics.median(t["levels_1"]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--step-batch", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "levels_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_levels needs an MI355X: there is nothing to measure on the CPU")
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats}]
    for s in SHAPES:
        lines.append(bench_shape(s, a.iters, a.repeats))
        print(json.dumps(lines[-1]), flush=True)
    lines.append(bench_step(a.step_iters, a.repeats, a.step_batch))
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
