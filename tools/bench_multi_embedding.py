#!/usr/bin/env python
"""The fused maximum-over-examples classification on the MI355X: device time of

  fused     la_classify_max - per-example logits, mask and maximum in one pass, the N C planes never written;
  two-step  la_classify on the N C prototypes as tokens, then the masked maximum over the examples in torch on the same buffers
            (masked_fill of the invalid examples + amax) - what the decoder would run without the fused kernel;

measured in ONE process, alternating (fused, two-step, fused, ...) so that both see the same clocks and neighbours, at
  B = 48, Npix = 120 x 120, N = 20, C = 2, Cf = 32   (Pascal 1-way 5-shot with embeddings_per_example = 4 at 480 px)
  B = 48, Npix = 256 x 256, N = 24, C = 3, Cf = 32
and the episodes / s of ``Lam.forward`` (HIP graph replay) for the Pascal model section (tests/cases_multi_embedding.py "e4" switches on the
ViT-MAE-B 480 px geometry) from cached embeddings.  Every figure is the median of --repeats windows of --iters launches after a
warm-up, with the min - max spread beside it; bytes are what the traffic model of each variant says (feat read once, seg written; the
two-step variant also writes and re-reads 4 N C bytes per pixel).  One JSON line per measurement goes to --out (default
profiles/multi_embedding_bench.jsonl, overwritten).

    python tools/bench_multi_embedding.py [--iters 50] [--repeats 7]
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

SHAPES = [dict(name="pascal_1w5s_480", b=48, npix=120 * 120, n=20, c=2, cf=32),
          dict(name="2w_256x256", b=48, npix=256 * 256, n=24, c=3, cf=32)]


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters        # us per call


def alternate(fns, iters, repeats):
    """{name: [us per call, one per window]} with the variants' windows interleaved."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return out


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "windows": len(us)}


def bench_shape(s, iters, repeats):
    b, npix, n, c, cf = s["b"], s["npix"], s["n"], s["c"], s["cf"]
    g = torch.Generator().manual_seed(7)
    feat = torch.randn(b * npix, cf, generator=g).cuda()
    protos = torch.randn(b, n, c, cf, generator=g).cuda()
    flags = (torch.rand(b, n, c, generator=g) < 0.8).to(torch.uint8)
    flags[:, 0] = 1
    flags = flags.cuda()
    seg = torch.empty(b, c, npix, device="cuda")
    win = torch.empty(b, c, npix, device="cuda", dtype=torch.int32)
    planes = torch.empty(b, n * c, npix, device="cuda")
    invalid = (flags == 0).view(b, n, c, 1)
    seg2 = torch.empty(b, c, npix, device="cuda")

    def fused():
        L.classify_max(feat, protos, flags, b, npix, n, c, cf, seg)

    def fused_win():
        L.classify_max(feat, protos, flags, b, npix, n, c, cf, seg, win)

    def two_step():
        L.classify(feat, protos.view(b, n * c, cf), b, npix, n * c, cf, planes)
        torch.amax(planes.view(b, n, c, npix).masked_fill(invalid, float("-inf")), dim=1, out=seg2)

    fused()
    two_step()
    torch.cuda.synchronize()
    same = bool(torch.equal(seg, seg2)) or float((seg - seg2).abs()[torch.isfinite(seg2)].max()) <= 1e-4
    t = alternate({"fused": fused, "two_step": two_step, "fused_with_winners": fused_win}, iters, repeats)
    px = b * npix
    bytes_fused, bytes_two = px * (4 * cf + 4 * c), px * (4 * cf + 4 * c + 2 * 4 * n * c)
    rec = {"what": "classify_max_vs_two_step", "shape": s, "results_agree": same,
           "fused": stats(t["fused"]), "two_step": stats(t["two_step"]), "fused_with_winners": stats(t["fused_with_winners"]),
           "model_bytes_per_pixel": {"fused": 4 * cf + 4 * c, "two_step": 4 * cf + 4 * c + 8 * n * c},
           "model_GBps": {"fused": round(bytes_fused / statistics.median(t["fused"]) / 1e3, 1),
                          "two_step": round(bytes_two / statistics.median(t["two_step"]) / 1e3, 1)},
           "two_step_over_fused": round(statistics.median(t["two_step"]) / statistics.median(t["fused"]), 3)}
    return rec


def bench_forward(iters, repeats, batch_size):
    """Lam.forward (graph replay) for the Pascal model section at 480 px, 1-way 5-shot, from cached (pre-neck, 768-channel) embeddings."""
    from labelanything_amd.config import LamConfig
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    cfg = LamConfig(encoder=None, use_vit=False, image_size=480, image_embed_dim=768, embed_dim=256, spatial_convs=3,
                    class_attention=False, example_attention=False, example_class_attention=False, custom_preprocess=False,
                    segment_example_logits=True, embeddings_per_example=4)
    out = []
    for tag, c in (("embeddings_per_example=4", cfg),
                   ("one prototype per class", dataclasses.replace(cfg, segment_example_logits=False, embeddings_per_example=None))):
        lam = Lam(c, seed=3).cuda()
        lam.use_graphs = True
        batch = make_episode(batch=batch_size, n_ways=1, k_shots=5, image_size=480, seed=5, prompts=("mask",), embeddings_channels=768, grid=30)
        batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        for _ in range(3):
            lam(batch)
        torch.cuda.synchronize()
        us = [window(lambda: lam(batch), iters) for _ in range(repeats)]
        eps = sorted(batch_size / (u * 1e-6) for u in us)
        out.append({"what": "lam_forward_from_cached_embeddings", "model": tag, "episodes_per_call": batch_size, "image_size": 480,
                    "n_ways": 1, "k_shots": 5, "episodes_per_s_median": round(statistics.median(eps), 1),
                    "episodes_per_s_min": round(eps[0], 1), "episodes_per_s_max": round(eps[-1], 1), "windows": repeats})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--forward-batch", type=int, default=8)
    ap.add_argument("--forward-iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_embedding_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multi_embedding needs an MI355X: there is nothing to measure on the CPU")
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats}]
    for s in SHAPES:
        lines.append(bench_shape(s, a.iters, a.repeats))
        print(json.dumps(lines[-1]), flush=True)
    for rec in bench_forward(a.forward_iters, a.repeats, a.forward_batch):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
