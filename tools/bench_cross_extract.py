#!/usr/bin/env python
"""The folded cross-attention extraction on the MI355X, at the Pascal geometry of parameters/validation/Pascal/mae_cross.yaml (30 x 30
grid, D = 256, 4 learned queries: R = 32 folded queries per pair) and the four episode shapes of its validation runs,
(M, C) in {(1, 2), (5, 2), (2, 3), (10, 3)}, B = 8 episodes per call.  Device time per layer of

  pool     la_extract_pool alone - the one pass over the (B M C, hw, D) stream;
  fused    la_extract_fold + la_extract_pool + la_extract_unfold - everything between q_proj and out_proj of one layer;
  eager    the LITERAL attention in torch, fp32, on the same buffers: k_proj and v_proj of the whole stream, softmax(q k^T / sqrt(hd)),
           weighted sum - what the layer costs without the kernel;

measured in ONE process with the variants' windows interleaved, so that all see the same clocks and neighbours.  Every figure is the median
of --repeats windows of --iters launches after a warm-up, with the min - max spread beside it.  Stream bytes per second and FLOP / s of
``pool`` are given against both roofs (8 TB/s HBM, 157 TFLOP/s fp32 MFMA): the model is 4 D bytes and 4 R D FLOP per stream row.  Then the
episodes / s of ``Lam.forward`` (HIP graph replay) from cached embeddings for the recipe's model section beside the pooled
embeddings_per_example = 4 model of tools/bench_multi_embedding.py, 1-way 5-shot.  One JSON line per measurement goes to --out.

    python tools/bench_cross_extract.py [--iters 50] [--repeats 7]
"""
import argparse
import dataclasses
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                        # noqa: E402

from labelanything_amd import _lib as L             # noqa: E402
from tools.bench_multi_embedding import alternate, stats, window   # noqa: E402

G, D, N, HEADS, B = 30, 256, 4, 8, 8
SHAPES = [dict(name="1w1s", m=1, c=2), dict(name="1w5s", m=5, c=2), dict(name="2w1s", m=2, c=3), dict(name="2w5s", m=10, c=3)]
HBM_BPS, MFMA_F32_FLOPS = 8e12, 157e12


def bench_shape(s, iters, repeats):
    m, c, hw, r, di, hd = s["m"], s["c"], G * G, HEADS * N, D // 2, D // 2 // HEADS
    bc, rows = B * c, B * c * N
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B * m * c, hw, D, generator=g).cuda()
    q = torch.randn(rows, di, generator=g).cuda()
    wk, wv = (torch.randn(di, D, generator=g) / 16).cuda(), (torch.randn(di, D, generator=g) / 16).cuda()
    bk, bv = (0.02 * torch.randn(di, generator=g)).cuda(), (0.02 * torch.randn(di, generator=g)).cuda()
    qt = torch.empty(bc, r, D, device="cuda")
    pooled = torch.empty(bc, r, D, device="cuda")
    o = torch.empty(rows, di, device="cuda")
    split, ns, per = L.extract_pool_plan(m, hw, D, r)
    scratch = torch.empty(bc * per, device="cuda")
    xp = x.view(B, m, c, hw, D)

    def pool():
        L.extract_pool(x, qt, B, m, c, hw, D, N, scratch, pooled)

    def fused():
        L.extract_fold(q, wk, bc, N, D, qt)
        L.extract_pool(x, qt, B, m, c, hw, D, N, scratch, pooled)
        L.extract_unfold(pooled, wv, bv, bc, N, D, o)

    def eager():
        keys = xp.permute(0, 2, 1, 3, 4).reshape(bc, m * hw, D)                       # "(b m c) hw d -> (b c) (m hw) d"
        k = torch.addmm(bk, keys.reshape(-1, D), wk.t()).view(bc, m * hw, HEADS, hd).transpose(1, 2)
        v = torch.addmm(bv, keys.reshape(-1, D), wv.t()).view(bc, m * hw, HEADS, hd).transpose(1, 2)
        qh = q.view(bc, N, HEADS, hd).transpose(1, 2)
        a = torch.softmax(qh @ k.transpose(2, 3) / math.sqrt(hd), dim=-1)
        return (a @ v).transpose(1, 2).reshape(rows, di)

    fused()
    ref = eager()
    torch.cuda.synchronize()
    agree = float((o - ref).abs().max() / ref.abs().max())
    t = alternate({"pool": pool, "fused": fused, "eager": eager}, iters, repeats)
    nrows = B * m * c * hw
    med = statistics.median(t["pool"]) * 1e-6
    return {"what": "extract_layer", "shape": dict(s, b=B, g=G, d=D, n=N, rows_per_pair=m * hw, pieces_per_pair=ns, workgroups=ns * bc),
            "fused_vs_eager_rel_diff": agree, "pool": stats(t["pool"]), "fused": stats(t["fused"]), "eager": stats(t["eager"]),
            "pool_stream_GBps": round(nrows * 4 * D / med / 1e9, 1), "pool_TFLOPs": round(nrows * 4 * r * D / med / 1e12, 2),
            "pool_fraction_of_hbm_roof": round(nrows * 4 * D / med / HBM_BPS, 4),
            "pool_fraction_of_fp32_mfma_roof": round(nrows * 4 * r * D / med / MFMA_F32_FLOPS, 4),
            "eager_over_fused": round(statistics.median(t["eager"]) / statistics.median(t["fused"]), 3)}


def bench_forward(iters, repeats, batch_size):
    from labelanything_amd.config import LamConfig
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    cfg = LamConfig(encoder=None, use_vit=False, image_size=480, image_embed_dim=768, embed_dim=256, spatial_convs=3,
                    class_attention=False, example_attention=False, example_class_attention=False, custom_preprocess=False,
                    segment_example_logits=True, embeddings_per_example=4)
    out = []
    for tag, c in (("x4: embedding_extraction=cross_attention, 4 queries", dataclasses.replace(cfg, embedding_extraction="cross_attention")),
                   ("e4: embeddings_per_example=4 (2 x 2 region means)", cfg)):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_extract_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cross_extract needs an MI355X: there is nothing to measure on the CPU")
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats}]
    for s in SHAPES:
        lines.append(bench_shape(s, a.iters, a.repeats))
        print(json.dumps(lines[-1]), flush=True)
    for rec in bench_forward(a.forward_iters, a.repeats, a.forward_batch):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
