#!/usr/bin/env python
"""The DINOv3 ViT-B/16 encoder forward on the MI355X against the ViT-MAE-B encoder of the same width, both at 480 px.

  (a) encoder  ``ImageEncoder("vit_b_dinov3")`` and ``ImageEncoder("vit_b_mae")`` on the same --images seeded images: 905 against 901
               tokens per image, the same twelve blocks; DINOv3 adds la_rope_qk per block and drops the position-table residual.
  (b) kernel   ``la_rope_qk`` alone on the q | k | v buffer of that batch (rows x 2304 fp16), with the bytes it has to move
               (patch rows x 2 ea x 2 bytes, each way) over its time.

How the windows are taken and where the JSON lines go: tools/bench_encoder.py.

    python tools/bench_dinov3.py [--images 8] [--iters 10] [--repeats 7]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                        # noqa: E402

from tools.bench_encoder import alternate, batch, forwards, main, stats   # noqa: E402

SIDE = 480


def encoders(images, iters, repeats):
    x = batch(images, SIDE, 11)
    encs, t = forwards({name: (name, x) for name in ("vit_b_dinov3", "vit_b_mae")}, iters, repeats)
    med = {k: statistics.median(v) for k, v in t.items()}
    return {"what": "encoder_forward_480", "images": images, "dinov3_block_path": encs["vit_b_dinov3"].lam.engine().last_block_path,
            **{k: stats(v) for k, v in t.items()}, "dinov3_over_mae": round(med["vit_b_dinov3"] / med["vit_b_mae"], 4),
            "difference_us": round(med["vit_b_dinov3"] - med["vit_b_mae"], 2),
            "spreads_overlap": not (max(t["vit_b_dinov3"]) < min(t["vit_b_mae"]) or max(t["vit_b_mae"]) < min(t["vit_b_dinov3"]))}


def rope_kernel(images, iters, repeats):
    from labelanything_amd import _lib as L
    from labelanything_amd.engine import rope_table
    heads, hd, prefix, grid = 12, 64, 5, SIDE // 16
    t, ea = grid * grid + prefix, heads * hd
    g = torch.Generator().manual_seed(12)
    qkv = torch.randn(images * t, 3 * ea, generator=g).to(torch.float16).cuda()
    cos, sin = (v.cuda() for v in rope_table(grid, hd, 100.0))
    times = alternate({"rope_qk": lambda: L.rope_qk(qkv, t, prefix, heads, hd, hd, cos, sin)}, iters * 10, repeats)["rope_qk"]
    moved = images * grid * grid * 2 * ea * 2 * 2            # read + write of the q | k columns of the patch rows
    return {"what": "la_rope_qk_per_layer", "images": images, "rows": images * t, "ld": 3 * ea, **stats(times),
            "bytes_moved": moved, "GBps": round(moved / statistics.median(times) * 1e-3, 1)}


def records(images, iters, repeats):
    enc = encoders(images, iters, repeats)
    yield enc
    rope = rope_kernel(images, iters, repeats)
    yield rope
    if enc["difference_us"] > 0:
        yield {"what": "rope_share_of_the_difference", "layers": 12, "share": round(12 * rope["median_us"] / enc["difference_us"], 3)}


if __name__ == "__main__":
    main("bench_dinov3", "r14_dinov3_bench.jsonl", records)
