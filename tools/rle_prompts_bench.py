#!/usr/bin/env python
"""Episode prompts from run-length annotations on the MI355X: the path this repository had (decode every annotation into a dense mask
on the host, stack per image, upload, one ``prompt_masks_from_instances`` launch per image - ``collate.annotations_to_tensor`` on dense
masks) against the run-length path (``RleBatch``: one upload of the packed runs, one scan, one launch for the episode), for the output
both have: the mask prompts and their flags.  Ground truths and point prompts have no device predecessor; their times are reported as
they are.

The host decode of the old path is the COCO format's DEFINITION in numpy (np.repeat of alternating 0 / 1, reshaped (w, h), transposed),
not pycocotools' C decoder, which is not available here: it is named ``numpy_definition_decode`` in the output.

Episode: seeded, 5-way 5-shot at COCO size - 26 images of 480 x 640, about 7 blob-shaped annotations each.  Both paths run in one
process, alternating, after warm-up; each repetition is timed by a host clock around a final synchronise.  One JSON line per
measurement on stdout (and appended to --out).

    python tools/rle_prompts_bench.py [--reps 15] [--out profiles/rle_prompts_bench.jsonl]
    python tools/rle_prompts_bench.py --mappings      # measurement library: both thread mappings of the tiled kernels
    python tools/rle_prompts_bench.py --profile       # one pass of each new-path call, for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                  # noqa: E402
import torch                                        # noqa: E402

N_IMAGES, H, W, WAYS, SIDE = 26, 480, 640, 5, 1024


def blob(rng):
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), dtype=bool)
    cy, cx = rng.uniform(0.1, 0.9) * H, rng.uniform(0.1, 0.9) * W
    for _ in range(int(rng.integers(2, 5))):
        ry, rx = rng.uniform(0.04, 0.2) * H, rng.uniform(0.04, 0.2) * W
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        cy, cx = cy + rng.uniform(-ry, ry), cx + rng.uniform(-rx, rx)
    return m


def make_episode(seed=0):
    """Per image its annotation dicts (file order) with compressed-string RLEs, as a COCO file holds them."""
    from labelanything_amd.annotations import rle_from_mask, rle_to_string
    rng = np.random.default_rng(seed)
    cat_ids = [-1] + list(range(1, WAYS + 1))
    images = []
    for _ in range(N_IMAGES):
        anns = []
        for _ in range(int(rng.integers(5, 10))):
            m = blob(rng)
            rle = rle_from_mask(m)
            ys, xs = np.nonzero(m)
            anns.append({"category_id": int(rng.integers(1, WAYS + 1)), "area": float(m.sum()),
                         "bbox": [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)],
                         "segmentation": {"size": rle["size"], "counts": rle_to_string(rle["counts"])}})
        images.append(anns)
    return images, cat_ids


def numpy_definition_decode(counts):
    return np.repeat(np.arange(counts.size, dtype=np.uint8) & 1, counts).reshape(W, H).T


def stats(times):
    return {"median_ms": round(statistics.median(times) * 1e3, 3), "min_ms": round(min(times) * 1e3, 3), "max_ms": round(max(times) * 1e3, 3)}


def timed_alternating(fns, reps, warmup=3):
    out = {k: [] for k in fns}
    for r in range(warmup + reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                out[k].append(time.perf_counter() - t0)
    return {k: stats(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mappings", action="store_true", help="A/B of the tiled kernels' thread mappings (needs make DEBUG=1)")
    ap.add_argument("--profile", action="store_true", help="run each new-path call a few times and exit (for rocprofv3)")
    args = ap.parse_args()
    if args.mappings:
        import tools._dbglib as D
        D.use_debug_library()
    from labelanything_amd import annotations as A
    from labelanything_amd.collate import annotations_to_tensor
    if not torch.cuda.is_available():
        raise SystemExit("this benchmark needs the GPU")
    dev = torch.device("cuda")
    images, cat_ids = make_episode()
    sizes = [(H, W)] * N_IMAGES
    c = len(cat_ids)
    counts = [[A.rle_from_string(a["segmentation"]["counts"]) for a in anns] for anns in images]        # string parsing is common to both
    slots = [[cat_ids.index(a["category_id"]) for a in anns] for anns in images]
    n_ann = sum(len(a) for a in images)
    runs = sum(int(x.size) for cs in counts for x in cs)
    rles = [[{"size": [H, W], "counts": x} for x in cs] for cs in counts]

    def old_path():
        dense = []
        for cs, sl in zip(counts, slots):
            masks = [numpy_definition_decode(x) for x in cs]
            dense.append({s: (np.stack([m for m, t in zip(masks, sl) if t == s]) if s in sl else np.zeros((0, H, W), dtype=np.uint8)) for s in range(c)})
        return annotations_to_tensor(dense, sizes, "mask", side=SIDE, custom_preprocess=True, device=dev)

    def pack():
        flat = [(r, i, s) for i, (rs, sl) in enumerate(zip(rles, slots)) for r, s in zip(rs, sl)]
        return A.pack_rles([f[0] for f in flat], [f[1] for f in flat], [f[2] for f in flat], sizes, n_classes=c,
                           info=[a for anns in images for a in anns], cat_ids=cat_ids)

    packed = pack()

    def new_path():
        return A.RleBatch(pack(), dev).prompt_masks(None, SIDE, 256, True)

    def new_path_packed():
        return A.RleBatch(packed, dev).prompt_masks(None, SIDE, 256, True)

    batch = A.RleBatch(packed, dev)
    random.seed(1)
    np.random.seed(1)
    plan = A.plan_prompts(packed, ["point"])
    want, wf = old_path()
    got, gf = new_path()
    if not (torch.equal(want, got) and torch.equal(wf, gf)):
        raise SystemExit("the two paths disagree")
    rows = [dict(what="episode", images=N_IMAGES, h=H, w=W, class_slots=c, annotations=n_ann, runs=runs,
                 packed_upload_bytes=int(4 * (packed.runs.size + packed.meta.size + 2 * N_IMAGES * 2 + 2 * N_IMAGES + n_ann)),
                 dense_upload_bytes=int(n_ann * H * W), output_bytes=int(got.numel() * 4), point_draws=len(plan["draws"]),
                 device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip,
                 host_decode="numpy_definition_decode (pycocotools is not installed)")]
    if args.profile:
        for _ in range(5):
            batch = A.RleBatch(packed, dev)
            batch.prompt_masks(None, SIDE, 256, True)
            batch.ground_truths()
            batch.points(plan["draws"], SIDE, True)
            batch.decode(list(range(8)))
        torch.cuda.synchronize()
        return
    if args.mappings:
        for name, env in (("column_lanes_lds_transpose", "0"), ("row_lanes", "1")):
            os.environ["LA_RLE_ROW_LANES"] = env
            t = timed_alternating({"prompt_masks": lambda: batch.prompt_masks(None, SIDE, 256, True), "ground_truths": batch.ground_truths,
                                   "decode_26": lambda: batch.decode(list(range(0, n_ann, max(1, n_ann // 26)))[:26])}, args.reps)
            rows += [dict(what="mapping", mapping=name, call=k, **v) for k, v in t.items()]
    else:
        t = timed_alternating({"old_decode_stack_upload_launch_per_image": old_path, "new_pack_upload_scan_one_launch": new_path,
                               "new_from_packed_runs": new_path_packed}, args.reps)
        old, new = t["old_decode_stack_upload_launch_per_image"], t["new_pack_upload_scan_one_launch"]
        rows += [dict(what="mask_prompts", path=k, **v) for k, v in t.items()]
        rows.append(dict(what="mask_prompts_ratio", old_over_new_median=round(old["median_ms"] / new["median_ms"], 1),
                         old_min_over_new_max=round(old["min_ms"] / new["max_ms"], 1)))
        t = timed_alternating({"prompt_masks_call": lambda: batch.prompt_masks(None, SIDE, 256, True), "ground_truths_call": batch.ground_truths,
                               "points_call": lambda: batch.points(plan["draws"], SIDE, True),
                               "upload_and_scan": lambda: A.RleBatch(packed, dev), "host_pack": pack,
                               "host_plan_prompts": lambda: A.plan_prompts(packed, ["bbox", "mask", "point"])}, args.reps)
        rows += [dict(what="new_path_parts", call=k, **v) for k, v in t.items()]
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
