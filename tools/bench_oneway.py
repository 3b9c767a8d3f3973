#!/usr/bin/env python
"""The one-way mask decoder's stream MLP on the MI355X (``fusion_transformer="OneWayTransformer"``; D = 256, hidden width 2048).

  (a) kernel   ``la_stream_mlp`` against the unfused chain  lin1 (+ ReLU) -> lin2 (+ residual) -> LayerNorm  on the same buffers, the
               launches ``LamEngine.one_way`` issues for the MLP half of a layer (exact-fp32 MFMA GEMMs, the hidden layer through global
               memory).  Rows: 900, 7 200 and 43 200 (30 x 30 grid: 1, 8 and 48 episodes) and 4 096 and 32 768 (64 x 64 grid: 1 and 8).
  (b) episode  ``Lam.forward`` from cached 768-channel embeddings with ``use_graphs`` at the model section and batch shapes of
               parameters/trainval/other/COCO_mae_oneway256.yaml (480 px, 30 x 30 grid, 2 ways): the one-way decoder fused, the
               one-way decoder on the chain (``LamEngine(fuse_oneway=False)``), and the two-way decoder of the same geometry for scale.

The variants' windows alternate in ONE process, so that all see the same clocks and neighbours; every figure is the median of --repeats
windows of --iters calls after a warm-up, with the min - max spread beside it.  One JSON line per measurement goes to --out.

    python tools/bench_oneway.py [--iters 20] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                        # noqa: E402

from tools.bench_multi_embedding import alternate, stats   # noqa: E402

D, H, G = 256, 2048, 30
ROWS = (900, 7200, 43200, 4096, 32768)


def planes(w):
    hi = w.to(torch.float16)
    return hi.contiguous(), (w - hi.float()).to(torch.float16).contiguous()


def kernel_against_chain(rows, iters, repeats):
    from labelanything_amd import _lib as L
    g = torch.Generator().manual_seed(rows)
    x0 = torch.randn(rows, D, generator=g).cuda()
    w1, w2 = (torch.randn(H, D, generator=g) / D ** 0.5).cuda(), (torch.randn(D, H, generator=g) / H ** 0.5).cuda()
    b1, b2 = (0.1 * torch.randn(H, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g)).cuda(), (0.1 * torch.randn(D, generator=g)).cuda()
    p1, p2 = planes(w1), planes(w2)
    xa, xb = x0.clone(), x0.clone()
    hbuf = torch.empty(rows, H, device="cuda")

    def fused():
        L.stream_mlp(xa, p1, b1, p2, b2, gamma, beta, 1e-5)

    def chain():
        L.gemm(xb, w1, bias=b1, out16=hbuf, act=L.ACT_RELU)
        L.gemm(hbuf, w2, bias=b2, res=xb, out32=xb)
        L.layernorm(xb, gamma, beta, 1e-5, out32=xb, dt=L.LA_F32)

    fused()
    chain()
    torch.cuda.synchronize()
    diff = float((xa - xb).abs().max() / xb.abs().max())
    t = alternate({"stream_mlp": fused, "chain": chain}, iters, repeats)
    med = {k: statistics.median(v) for k, v in t.items()}
    flop = 2.0 * 2 * rows * D * H            # of the definition: two GEMMs (the kernel issues three fp16 products for each)
    return {"what": "stream_mlp_against_chain", "rows": rows, "stream_mlp": stats(t["stream_mlp"]), "chain": stats(t["chain"]),
            "chain_over_stream_mlp": round(med["chain"] / med["stream_mlp"], 3),
            "spreads_overlap": not (max(t["stream_mlp"]) < min(t["chain"]) or max(t["chain"]) < min(t["stream_mlp"])),
            "stream_mlp_TFLOPs_of_the_definition": round(flop / med["stream_mlp"] * 1e-6, 1), "first_call_max_norm_difference": diff}


def episode(batch_size, shots, iters, repeats):
    from labelanything_amd.config import LamConfig
    from labelanything_amd.engine import LamEngine
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    import dataclasses
    cfg = LamConfig(encoder=None, use_vit=False, image_size=480, image_embed_dim=768, embed_dim=D, spatial_convs=3, class_attention=False,
                    example_attention=False, example_class_attention=False, custom_preprocess=True, fusion_transformer="OneWayTransformer")
    lams = {"oneway_fused": Lam(cfg, seed=3).cuda(), "oneway_chain": Lam(cfg, seed=3).cuda(),
            "twoway": Lam(dataclasses.replace(cfg, fusion_transformer="TwoWayTransformer"), seed=3).cuda()}
    lam = lams["oneway_chain"]
    lam.engine()                # (sets the cache key that keeps the hand-built engine in place)
    lam._engine = LamEngine(lam.cfg, lam.state_dict(), lam._device(), lam.compute_dtype, lam.decoder_dtype, lam.precise, fuse_oneway=False)
    lams["oneway_fused"].engine().ONEWAY_MLP_MIN_ROWS = 0       # the fused kernel whatever the default threshold says
    batch = make_episode(batch=batch_size, n_ways=2, k_shots=shots, image_size=480, seed=5, prompts=("mask",), embeddings_channels=768, grid=G)
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    for m in lams.values():
        m.use_graphs = True
    fns = {tag: (lambda m=m: m(batch)) for tag, m in lams.items()}
    for fn in fns.values():
        fn()
    assert not lams["oneway_chain"].engine().fuse_oneway and lams["oneway_fused"].engine().oneway_mlp_fused(3, 1)
    t = alternate(fns, iters, repeats)
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"what": "lam_forward_from_cached_embeddings", "batch": batch_size, "shots": shots, "stream_rows": batch_size * G * G,
            **{k: stats(v) for k, v in t.items()}, "chain_over_fused": round(med["oneway_chain"] / med["oneway_fused"], 3),
            "fused_over_twoway": round(med["oneway_fused"] / med["twoway"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oneway_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_oneway needs an MI355X: there is nothing to measure on the CPU")
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats,
              "shape": dict(d=D, h=H, g=G)}]
    print(json.dumps(lines[0]), flush=True)
    for rows in ROWS:
        lines.append(kernel_against_chain(rows, a.iters, a.repeats))
        print(json.dumps(lines[-1]), flush=True)
    for bsz, shots in ((2, 4), (4, 2), (16, 1)):
        lines.append(episode(bsz, shots, a.iters, a.repeats))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
