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

--train measures the training side instead, on the recipe shape (480 px, 30 x 30 grid, D = 256, 4 queries, 768-channel embeddings, 2-way
5-shot: M = 5, C = 3 with the background), --train-batch episodes per step:

  pool / pool_lse / pool_bwd   la_extract_pool, la_extract_pool_lse and la_extract_pool_bwd per layer (per-pair queries), with the bytes
                               la_extract_pool_bwd moves - the stream read once, dx written once, the dqt partials (R / 64 of the stream)
                               written and read back - against the 8 TB/s HBM roof, and its 10 R D FLOP per stream row against the MFMA roof;
  module                       the two-layer extraction module forward + backward: the training graph's nodes (DecoderGraph.extract_embeddings)
                               beside the restatement of tests/cross_extract_ref.py in stock PyTorch eager fp32 on the same GPU, in its
                               folded and its literal form - the comparison target, since the option had no training path before;
  step                         LamTrainer.step of the whole model (embedding_dropout = 0.2) from precomputed embeddings.

    python tools/bench_cross_extract.py --train [--out profiles/cross_extract_train_bench.jsonl]
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


def bench_train_kernels(b, m, c, iters, repeats):
    hw, r = G * G, HEADS * N
    bc = b * c
    g = torch.Generator().manual_seed(13)
    x = torch.randn(b * m * c, hw, D, generator=g).cuda()
    qt = (torch.randn(bc, r, D, generator=g) * (4.3 / math.sqrt(D))).cuda()
    dout = torch.randn(bc, r, D, generator=g).cuda()
    out, lse = torch.empty(bc, r, D, device="cuda"), torch.empty(bc, r, device="cuda")
    dx, dqt = torch.empty_like(x), torch.empty_like(qt)
    scratch = torch.empty(bc * L.extract_pool_plan(m, hw, D, r)[2], device="cuda")
    rows, nt, per = L.extract_pool_bwd_plan(m, hw, D, r)
    scratch_b = torch.empty(bc * per, device="cuda")
    t = alternate({"pool": lambda: L.extract_pool(x, qt, b, m, c, hw, D, N, scratch, out),
                   "pool_lse": lambda: L.extract_pool_lse(x, qt, b, m, c, hw, D, N, scratch, out, lse),
                   "pool_bwd": lambda: L.extract_pool_bwd(x, qt, out, lse, dout, b, m, c, hw, D, N, scratch_b, dx, dqt)}, iters, repeats)
    nrows = b * m * c * hw
    med = statistics.median(t["pool_bwd"]) * 1e-6
    moved = nrows * 4 * D * 2 + 2 * bc * nt * r * D * 4                     # x in, dx out, the dqt partials out and in
    return {"what": "extract_pool_bwd", "shape": dict(b=b, m=m, c=c, g=G, d=D, n=N, rows_per_pair=m * hw, tile_rows=rows, tiles_per_pair=nt,
                                                      workgroups=nt * bc),
            "pool": stats(t["pool"]), "pool_lse": stats(t["pool_lse"]), "pool_bwd": stats(t["pool_bwd"]),
            "bwd_over_fwd": round(statistics.median(t["pool_bwd"]) / statistics.median(t["pool"]), 3),
            "bwd_bytes_moved": moved, "bwd_GBps": round(moved / med / 1e9, 1), "bwd_fraction_of_hbm_roof": round(moved / med / HBM_BPS, 4),
            "bwd_TFLOPs": round(nrows * 10 * r * D / med / 1e12, 2),
            "bwd_fraction_of_fp32_mfma_roof": round(nrows * 10 * r * D / med / MFMA_F32_FLOPS, 4)}


def bench_train_model(batch_size, iters, repeats):
    from labelanything_amd.config import LamConfig
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import DecoderGraph, LamTrainer
    from tests import cross_extract_ref as R
    from tests.helpers import make_gt
    cfg = LamConfig(encoder=None, use_vit=False, image_size=480, image_embed_dim=768, embed_dim=256, spatial_convs=3,
                    class_attention=False, example_attention=False, example_class_attention=False, custom_preprocess=False,
                    segment_example_logits=True, embeddings_per_example=N, embedding_extraction="cross_attention")
    lam = Lam(cfg, seed=3).cuda()
    batch = make_episode(batch=batch_size, n_ways=2, k_shots=5, image_size=480, seed=5, prompts=("mask",), embeddings_channels=768, grid=G)
    b, m, c = batch["flag_examples"].shape
    gt = make_gt(batch, c, seed=17)
    # the module alone, forward + backward, on a stream of the step's shape
    ex = R.PRE + "."
    names = [k for k, _ in lam.named_parameters() if k.startswith(ex)]
    params = dict(lam.named_parameters())
    for k in names:
        params[k].requires_grad_(True)
    hw = G * G
    x = torch.randn(b * m * c * hw, D, generator=torch.Generator().manual_seed(17)).cuda().requires_grad_(True)
    wout = torch.randn(b, N, c, D, generator=torch.Generator().manual_seed(18)).cuda()
    graph = DecoderGraph(lam)
    w = {k: params[k] for k in names}

    def clear():
        x.grad = None
        for k in names:
            params[k].grad = None

    def ours():
        clear()
        (graph.extract_embeddings(x, b, m, c, hw) * wout).sum().backward()

    def eager(form):
        def run():
            clear()
            (R.extract(x.view(b * m * c, hw, D), b, m, c, w, form) * wout).sum().backward()
        return run

    ours()
    mine = x.grad.clone()
    eager("folded")()
    agree = float((mine - x.grad).abs().max() / x.grad.abs().max())
    t = alternate({"ours": ours, "eager_folded": eager("folded"), "eager_literal": eager("literal")}, max(1, iters // 5), repeats)
    clear()
    for k in names:
        params[k].requires_grad_(False)
    rec = [{"what": "extraction_module_forward_backward", "shape": dict(b=b, m=m, c=c, g=G, d=D, n=N), "dx_vs_eager_rel_diff": agree,
            "ours": stats(t["ours"]), "eager_folded": stats(t["eager_folded"]), "eager_literal": stats(t["eager_literal"]),
            "eager_folded_over_ours": round(statistics.median(t["eager_folded"]) / statistics.median(t["ours"]), 3),
            "eager_literal_over_ours": round(statistics.median(t["eager_literal"]) / statistics.median(t["ours"]), 3)}]
    tr = LamTrainer(lam, embedding_dropout=0.2)
    dev_batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    for _ in range(3):
        tr.step(dev_batch, gt)
    torch.cuda.synchronize()
    us = [window(lambda: tr.step(dev_batch, gt), max(1, iters // 10)) for _ in range(repeats)]
    rec.append({"what": "training_step", "model": "x4: embedding_extraction=cross_attention, 4 queries, embedding_dropout 0.2",
                "episodes_per_step": batch_size, "n_ways": 2, "k_shots": 5, "image_size": 480, "step": stats(us),
                "episodes_per_s_median": round(batch_size / (statistics.median(us) * 1e-6), 2)})
    return rec, (b, m, c)


def main_train(a):
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats}]
    recs, (b, m, c) = bench_train_model(a.train_batch, a.iters, a.repeats)
    lines.append(bench_train_kernels(b, m, c, a.iters, a.repeats))
    lines += recs
    out = a.out if a.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "cross_extract_train_bench.jsonl")
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    with open(out, "w") as fh:
        for rec in lines:
            print(json.dumps(rec), flush=True)
            fh.write(json.dumps(rec) + "\n")


DEFAULT_OUT = os.path.join(ROOT, "profiles", "cross_extract_bench.jsonl")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--forward-batch", type=int, default=8)
    ap.add_argument("--forward-iters", type=int, default=10)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--train", action="store_true", help="measure the training side (la_extract_pool_bwd, the module, the whole step)")
    ap.add_argument("--train-batch", type=int, default=2, help="episodes per training step")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cross_extract needs an MI355X: there is nothing to measure on the CPU")
    if a.train:
        return main_train(a)
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
