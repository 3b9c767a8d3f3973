#!/usr/bin/env python
"""The DINOv2 ViT-B/14 encoder forward on the MI355X, and its padded patch gather beside the plain one.

  (a) encoder  ``ImageEncoder("vit_b_dinov2")`` on --images seeded images at 224 px (the recipe of parameters/trainval/coco/dinov2.yaml:
               257 tokens per image, position table resampled 37 -> 16) and at 518 px (1370 tokens, the table as stored).
  (b) gather   ``la_im2col_patch_pad`` (p = 14, K = 588 -> Kp = 640) alone on those batches, in the operand form the encoder uses (fp16
               plane pairs, LA_F16X2) and as plain fp16, with the bytes it has to move (the image read once, every output column - padding
               included - written once) over its time; beside it ``la_im2col_patch`` (p = 16, K = 768) on the same images as the
               yardstick - at 518 px on their top-left 512 x 512 corner, the largest part a 16 px grid covers.

How the windows are taken and where the JSON lines go: tools/bench_encoder.py.

    python tools/bench_dinov2.py [--images 8] [--iters 10] [--repeats 7]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                                        # noqa: E402

from tools.bench_encoder import alternate, batch, forwards, main, stats   # noqa: E402

SIDES = (224, 518)


def encoders(images, iters, repeats):
    encs, t = forwards({f"forward_{side}": ("vit_b_dinov2", batch(images, side, 11 + side)) for side in SIDES}, iters, repeats)
    engines = {str(side): encs[f"forward_{side}"].lam.engine() for side in SIDES}
    return {"what": "vit_b_dinov2_forward", "images": images, "block_path": {k: e.last_block_path for k, e in engines.items()},
            "patch_split": {k: bool(e.patch_split) for k, e in engines.items()}, **{k: stats(v) for k, v in t.items()}}


def gathers(images, iters, repeats, side):
    from labelanything_amd import _lib as L
    from labelanything_amd.engine import patch_kp
    x14 = batch(images, side, 11 + side)
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


def records(images, iters, repeats):
    enc = encoders(images, iters, repeats)
    yield enc
    for side in SIDES:
        gather = gathers(images, iters, repeats, side)
        yield gather
        form = "f16x2" if enc["patch_split"][str(side)] else "f16"
        yield {"what": f"gather_share_of_forward_{side}", "form": form,
               "share": round(gather[f"pad_p14_{form}"]["median_us"] / enc[f"forward_{side}"]["median_us"], 5)}


if __name__ == "__main__":
    main("bench_dinov2", "r15_dinov2_bench.jsonl", records)
