#!/usr/bin/env python
"""The TokenPool prompt encoder against the plain prompt encoder of the same commit on the MI355X, at the cfg3 shape: MAE-480 geometry
(30 x 30 grid, 768-channel precomputed embeddings behind the neck, D = 256), 5-way 5-shot episodes (M = 25 supports, C = 6 classes,
P = 150 pairs), mask prompts, the model section of parameters/trainval/pascal/mae_pool.yaml with and without ``prompt_encoder: TokenPool``,
same weights, same episodes.

  stage    ``LamEngine.prompt_encoder`` alone from post-neck support features, replayed from a HIP graph (the launch sequence of the
           model's own replay): sparse tokens, dense prompts (la_mask_embed / la_mask_embed_pooled), the two-way transformer, pooling or
           token mean, merge attention, class mean;
  episode  ``Lam.forward`` from the cached 768-channel embeddings with ``use_graphs`` (neck, prompt encoder, mask decoder, post-processing).

The two variants' windows alternate in ONE process, so that both see the same clocks and neighbours; every figure is the median of
--repeats windows of --iters calls after a warm-up, with the min - max spread beside it.  The stream model beside the times: the plain
stage's fp32 stream is P hw D 4 bytes per episode, TokenPool's B M hw D 4, C times less.  One JSON line per measurement goes to --out.

    python tools/bench_token_pool.py [--batch 2] [--iters 20] [--repeats 7]
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

from tools.bench_multi_embedding import alternate, stats   # noqa: E402

G, D, WAYS, SHOTS = 30, 256, 5, 5


def models():
    from labelanything_amd.config import LamConfig
    from labelanything_amd.models import Lam
    cfg = LamConfig(encoder=None, use_vit=False, image_size=480, image_embed_dim=768, embed_dim=D, spatial_convs=3, class_attention=False,
                    example_attention=False, example_class_attention=True, custom_preprocess=True,
                    class_encoder={"name": "RandomMatrixEncoder", "bank_size": 100, "embed_dim": D})
    rows = torch.cat([torch.zeros(1, dtype=torch.long), torch.randperm(99, generator=torch.Generator().manual_seed(3))[:WAYS] + 1])
    out = {}
    for tag, c in (("plain", cfg), ("token_pool", dataclasses.replace(cfg, prompt_encoder="TokenPool"))):
        lam = Lam(c, seed=3).cuda()
        lam.selected_rows = rows
        out[tag] = lam
    return out


def graphed(fn):
    """fn replayed from a HIP graph, captured after a warm-up that sizes every arena buffer."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2, help="episodes per call")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_pool_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_token_pool needs an MI355X: there is nothing to measure on the CPU")
    from labelanything_amd.episodes import make_episode
    b, m, c, hw = a.batch, WAYS * SHOTS, WAYS + 1, G * G
    lams = models()
    batch = make_episode(batch=b, n_ways=WAYS, k_shots=SHOTS, image_size=480, seed=5, prompts=("mask",), embeddings_channels=768, grid=G)
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats,
              "shape": dict(b=b, m=m, c=c, g=G, d=D, pairs=b * m * c, supports=b * m),
              "stream_MB_per_call": {"plain": round(b * m * c * hw * D * 4 / 1e6, 1), "token_pool": round(b * m * hw * D * 4 / 1e6, 1)}}]
    print(json.dumps(lines[0]), flush=True)

    # the stage alone, from post-neck support features
    support = torch.randn(b * m * hw, D, generator=torch.Generator().manual_seed(9)).cuda()
    stage = {}
    for tag, lam in lams.items():
        eng = lam.engine()
        inp, _ = lam._prepare(batch, with_post=False)
        masks = (inp["prompt_masks"], inp["flag_masks"])

        def run(eng=eng, inp=inp, masks=masks):
            return eng.prompt_encoder(support, b, m, G, None, None, masks, inp["flag_examples"], inp["selected_rows"])
        stage[tag] = graphed(run)
    t = alternate(stage, a.iters, a.repeats)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append({"what": "prompt_encoder_stage", "plain": stats(t["plain"]), "token_pool": stats(t["token_pool"]),
                  "plain_over_token_pool": round(med["plain"] / med["token_pool"], 3),
                  "us_per_episode": {k: round(v / b, 1) for k, v in med.items()}})
    print(json.dumps(lines[-1]), flush=True)

    # the whole decoder-only episode
    for lam in lams.values():
        lam.use_graphs = True
    episode = {tag: (lambda lam=lam: lam(batch)) for tag, lam in lams.items()}
    t = alternate(episode, a.iters, a.repeats)
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append({"what": "lam_forward_from_cached_embeddings", "plain": stats(t["plain"]), "token_pool": stats(t["token_pool"]),
                  "plain_over_token_pool": round(med["plain"] / med["token_pool"], 3),
                  "episodes_per_s": {k: round(b / (v * 1e-6), 1) for k, v in med.items()}})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
