#!/usr/bin/env python
"""The DINOv3 ViT-B/16 encoder forward on the MI355X against the ViT-MAE-B encoder of the same width, both at 480 px.

  (a) encoder  ``ImageEncoder("vit_b_dinov3")`` and ``ImageEncoder("vit_b_mae")`` on the same --images seeded images: 905 against 901
               tokens per image, the same twelve blocks; DINOv3 adds la_rope_qk per block and drops the position-table residual.
  (b) kernel   ``la_rope_qk`` alone on the q | k | v buffer of that batch (rows x 2304 fp16), with the bytes it has to move
               (patch rows x 2 ea x 2 bytes, each way) over its time.

The variants' windows alternate in ONE process, so that all see the same clocks and neighbours; every figure is the median of --repeats
windows of --iters calls after a warm-up, with the min - max spread beside it.  One JSON line per measurement goes to --out.

    python tools/bench_dinov3.py [--images 8] [--iters 10] [--repeats 7]
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

SIDE = 480


def encoders(images, iters, repeats):
    from labelanything_amd.models import ImageEncoder
    g = torch.Generator().manual_seed(11)
    x = torch.randn(images, 3, SIDE, SIDE, generator=g).cuda()
    encs = {name: ImageEncoder(name, image_size=SIDE, seed=3).cuda() for name in ("vit_b_dinov3", "vit_b_mae")}
    fns = {name: (lambda e=e: e(x)) for name, e in encs.items()}
    for fn in fns.values():
        fn()
    t = alternate(fns, iters, repeats)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_dinov3_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dinov3 needs an MI355X: there is nothing to measure on the CPU")
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats}]
    print(json.dumps(lines[0]), flush=True)
    for fn in (encoders, rope_kernel):
        lines.append(fn(a.images, a.iters, a.repeats))
        print(json.dumps(lines[-1]), flush=True)
    enc, rope = lines[1], lines[2]
    if enc["difference_us"] > 0:
        lines.append({"what": "rope_share_of_the_difference", "layers": 12,
                      "share": round(12 * rope["median_us"] / enc["difference_us"], 3)})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
