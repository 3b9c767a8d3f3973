#!/usr/bin/env python
"""The DINOv2 ViT-B/14 encoder forward on the MI355X, and its padded patch gather beside the plain one.

  (a) encoder  ``ImageEncoder("vit_b_dinov2")`` on --images seeded images at 224 px (the recipe of parameters/trainval/coco/dinov2.yaml:
               257 tokens per image, position table resampled 37 -> 16) and at 518 px (1370 tokens, the table as stored).
  (b) gather   ``la_im2col_patch_pad`` (p = 14, K = 588 -> Kp = 640) alone on those batches, in the operand form the encoder uses (fp16
               plane pairs, LA_F16X2) and as plain fp16, with the bytes it has to move (the image read once, every output column - padding
               included - written once) over its time; beside it ``la_im2col_patch`` (p = 16, K = 768) on the same images as the
               yardstick - at 518 px on their top-left 512 x 512 corner, the largest part a 16 px grid covers.

The variants' windows alternate in ONE process, so that all see the same clocks and neighbours; every figure is the median of --repeats
windows of --iters calls after a warm-up, with the min - max spread beside it.  One JSON line per measurement goes to --out.

    python tools/bench_dinov2.py [--images 8] [--iters 10] [--repeats 7]
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

SIDES = (224, 518)


def batch(images, side):
    g = torch.Generator().manual_seed(11 + side)
    return torch.randn(images, 3, side, side, generator=g).cuda()


def encoders(images, iters, repeats):
    from labelanything_amd.models import ImageEncoder
    xs = {side: batch(images, side) for side in SIDES}
    encs = {side: ImageEncoder("vit_b_dinov2", image_size=side, seed=3).cuda() for side in SIDES}
    fns = {f"forward_{side}": (lambda e=encs[side], x=xs[side]: e(x)) for side in SIDES}
    for fn in fns.values():
        fn()
    t = alternate(fns, iters, repeats)
    return {"what": "vit_b_dinov2_forward", "images": images,
            "block_path": {str(side): encs[side].lam.engine().last_block_path for side in SIDES},
            "patch_split": {str(side): bool(encs[side].lam.engine().patch_split) for side in SIDES},
            **{k: stats(v) for k, v in t.items()}}


def gathers(images, iters, repeats, side):
    from labelanything_amd import _lib as L
    from labelanything_amd.engine import patch_kp
    x14 = batch(images, side)
    s16 = side // 16 * 16
    x16 = x14[..., :s16, :s16].contiguous()
    kp, k16 = patch_kp(14), patch_kp(16)
    rows14, rows16 = images * (side // 14) ** 2, images * (s16 // 16) ** 2
    fns, moved = {}, {}
    for form, split in (("f16x2", True), ("f16", False)):
        planes = 2 if split else 1
        o14 = torch.empty(rows14, planes * kp, dtype=torch.float16, device="cuda")
        o16 = torch.empty(rows16, planes * k16, dtype=torch.float16, device="cuda")
        fns[f"pad_p14_{form}"] = lambda o=o14, s=split: L.im2col_patch_pad(x14, 14, kp, o, split=s)
        fns[f"plain_p16_{form}"] = lambda o=o16, s=split: L.im2col_patch(x16, 16, o, split=s)
        moved[f"pad_p14_{form}"] = x14.numel() * 4 + o14.numel() * 2
        moved[f"plain_p16_{form}"] = x16.numel() * 4 + o16.numel() * 2
    t = alternate(fns, iters * 10, repeats)
    rec = {"what": f"patch_gather_{side}", "images": images, "side_p14": side, "side_p16": s16, "Kp": kp}
    for k, v in t.items():
        rec[k] = {**stats(v), "bytes_moved": moved[k], "GBps": round(moved[k] / statistics.median(v) * 1e-3, 1)}
    for form in ("f16x2", "f16"):
        rec[f"pad_over_plain_rate_{form}"] = round(rec[f"pad_p14_{form}"]["GBps"] / rec[f"plain_p16_{form}"]["GBps"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_dinov2_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dinov2 needs an MI355X: there is nothing to measure on the CPU")
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats}]
    print(json.dumps(lines[0]), flush=True)
    lines.append(encoders(a.images, a.iters, a.repeats))
    print(json.dumps(lines[-1]), flush=True)
    for side in SIDES:
        lines.append(gathers(a.images, a.iters, a.repeats, side))
        print(json.dumps(lines[-1]), flush=True)
        form = "f16x2" if lines[1]["patch_split"][str(side)] else "f16"
        lines.append({"what": f"gather_share_of_forward_{side}", "form": form,
                      "share": round(lines[-1][f"pad_p14_{form}"]["median_us"] / lines[1][f"forward_{side}"]["median_us"], 5)})
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
