#!/usr/bin/env python
"""Golden vectors for episodes built from run-length annotations: the REFERENCE's own ``CocoLVISDataset._get_prompts`` and
``compute_ground_truths`` (data/coco.py:397-477,514-544), its ``PromptsProcessor`` (data/transforms.py) and ``annotations_to_tensor`` /
``flags_merge`` / ``collate_gts`` (data/utils.py) are run on seeded synthetic COCO annotations; the annotations, the recorded plan
(prompt type per annotation, boxes, (annotation, rank) draws) and the outputs go to tests/golden/rle_episode.{json,safetensors}.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_rle_episode.py

What is NOT the reference here, because pycocotools and torchvision cannot be installed where this runs: the stubbed
``pycocotools.mask.decode`` / ``frPyObjects`` are the RLE format's definition in numpy (np.repeat of alternating 0 / 1, reshaped (w, h)
and transposed; compressed strings through labelanything_amd.annotations.rle_from_string), and ``torchvision...resize`` on a tensor with
NEAREST is torch's F.interpolate(mode="nearest"), as in oracle/preprocess_oracle.py.  Everything the reference computes ON TOP of a
decoded mask is its own code."""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tools.golden_lib             # noqa: E402,F401  (stub finder, reference first on sys.path)

import numpy as np                        # noqa: E402
import torch                              # noqa: E402
import torch.nn.functional as F           # noqa: E402
from safetensors.torch import save_file   # noqa: E402

from labelanything_amd.annotations import rle_from_mask, rle_from_string, rle_to_string   # noqa: E402

SIZES = [(120, 160), (97, 131), (200, 150), (1, 37), (41, 1)]
CAT_IDS = [-1, 3, 7, 11]
SIDE = 1024
MAX_POINTS_ANNOTATIONS, MAX_POINTS_PER_ANNOTATION = 5, 10
SEEDS = {"custom1": 11, "custom0": 23}


def counts_of(segm):
    c = segm["counts"]
    return rle_from_string(c) if isinstance(c, (str, bytes)) else np.asarray(c, dtype=np.int64)


def decode(rle):
    """The format's definition: runs alternate 0 / 1 from a 0-run, column-major."""
    h, w = rle["size"]
    c = counts_of(rle)
    return np.repeat(np.arange(c.size) & 1, c).astype(np.uint8).reshape(w, h).T.copy()


def fr_py_objects(segm, h, w):
    if isinstance(segm, dict):
        return segm
    raise NotImplementedError("polygons need pycocotools")


def nearest_resize(t, size, interpolation=None):
    return F.interpolate(t.unsqueeze(0), size=tuple(size), mode="nearest")[0]


def blob(rng, h, w):
    """A few overlapping ellipses: a blob with a few hundred runs at most."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), dtype=bool)
    cy, cx = rng.uniform(0, h), rng.uniform(0, w)
    for _ in range(int(rng.integers(1, 4))):
        ry, rx = rng.uniform(0.06, 0.3) * h + 1, rng.uniform(0.06, 0.3) * w + 1
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1
        cy, cx = cy + rng.uniform(-ry, ry), cx + rng.uniform(-rx, rx)
    return m


def make_annotations(rng):
    anns, next_id = [], 1

    def add(img, cat, mask, form, area_scale=1.0):
        nonlocal next_id
        h, w = SIZES[img]
        rle = rle_from_mask(mask)
        if form == "string":
            rle = {"size": rle["size"], "counts": rle_to_string(rle["counts"]).decode("ascii")}
        ys, xs = np.nonzero(mask)
        box = [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)] if ys.size else [0.0, 0.0, 1.0, 1.0]
        anns.append({"id": next_id, "image_id": img, "category_id": cat, "segmentation": rle, "bbox": box,
                     "area": float(mask.sum()) * area_scale, "iscrowd": 0})
        next_id += 1

    # image 0: 6 annotations of category 3 (> MAX_POINTS_ANNOTATIONS: all MASK) and the edge cases, interleaved so that file order matters
    h, w = SIZES[0]
    full = np.ones((h, w), dtype=bool)
    corner = np.zeros((h, w), dtype=bool)
    corner[:9, :7] = True                                         # pixel (0, 0) set: the first run has length 0
    columns = np.zeros((h, w), dtype=bool)
    columns[:, 40:45] = True                                      # one 1-run across five whole columns
    single = np.zeros((h, w), dtype=bool)
    single[77, 101] = True                                        # area 1: rank 0 == area - 1
    empty = np.zeros((h, w), dtype=bool)                          # the (0, 0) fallback
    add(0, 7, full, "list")
    for j in range(6):
        add(0, 3, blob(rng, h, w), "string" if j % 2 else "list", 1.0 + 0.05 * j)
    add(0, 7, corner, "string")
    add(0, 11, columns, "list")
    add(0, 99, blob(rng, h, w), "list")                          # a category outside the episode
    add(0, 11, single, "string")
    add(0, 7, empty, "list")
    add(0, 11, blob(rng, h, w), "string", 0.8)
    add(0, 7, blob(rng, h, w), "list")
    # image 1: no annotation of category 11; image 2: everything
    for img, cats, k in ((1, (3, 7), 12), (2, (3, 7, 11), 16)):
        h, w = SIZES[img]
        for j in range(k):
            add(img, cats[int(rng.integers(len(cats)))], blob(rng, h, w), "string" if rng.random() < 0.5 else "list", float(rng.uniform(0.7, 1.3)))
    # h = 1 and w = 1 images
    row = np.zeros(SIZES[3], dtype=bool)
    row[0, 5:20] = True
    add(3, 3, row, "list")
    row2 = np.zeros(SIZES[3], dtype=bool)
    row2[0, 15:30] = True
    add(3, 11, row2, "string")
    col = np.zeros(SIZES[4], dtype=bool)
    col[10:33, 0] = True
    add(4, 7, col, "string")
    col2 = np.zeros(SIZES[4], dtype=bool)
    col2[0:12, 0] = True
    add(4, 3, col2, "list")
    return anns


def main():
    from label_anything.data import transforms as T
    from label_anything.data import utils as U
    from label_anything.data.coco import CocoLVISDataset
    from label_anything.data.utils import PromptType

    T.mask_utils.decode = decode
    T.mask_utils.frPyObjects = fr_py_objects
    T.mask_utils.merge = lambda rles: rles
    T.resize = nearest_resize

    anns = make_annotations(np.random.default_rng(5))
    image_ids = list(range(len(SIZES)))
    log = []

    class Recording(T.PromptsProcessor):
        def convert_bbox(self, *a, **kw):
            log.append("b")
            return super().convert_bbox(*a, **kw)

        def convert_mask(self, *a, **kw):
            log.append("m")
            return super().convert_mask(*a, **kw)

        def sample_point(self, mask):
            log.append("p")
            return super().sample_point(mask)

    tensors, meta = {}, {"sizes": SIZES, "cat_ids": CAT_IDS, "side": SIDE, "max_points_annotations": MAX_POINTS_ANNOTATIONS,
                         "max_points_per_annotation": MAX_POINTS_PER_ANNOTATION, "annotations": anns, "episodes": {}}
    gts_seen = None
    for tag, seed in SEEDS.items():
        ds = CocoLVISDataset.__new__(CocoLVISDataset)
        ds.images = {i: {"height": h, "width": w} for i, (h, w) in enumerate(SIZES)}
        ds.img_annotations = {i: [a for a in anns if a["image_id"] == i] for i in image_ids}
        ds.img2cat_annotations = {i: {} for i in image_ids}
        for a in anns:
            ds.img2cat_annotations[a["image_id"]].setdefault(a["category_id"], []).append(a)
        ds.max_points_annotations, ds.max_points_per_annotation, ds.add_box_noise = MAX_POINTS_ANNOTATIONS, MAX_POINTS_PER_ANNOTATION, True
        ds.prompts_processor = Recording(long_side_length=SIDE, masks_side_length=256, custom_preprocess=tag == "custom1")
        ranks, choice = [], np.random.choice
        np.random.choice = lambda n: ranks.append(int(choice(n))) or ranks[-1]
        del log[:]
        random.seed(seed)
        np.random.seed(seed)
        try:
            bboxes, masks, points, classes, img_sizes = ds._get_prompts(image_ids, CAT_IDS, [PromptType.BBOX, PromptType.MASK, PromptType.POINT])
        finally:
            np.random.choice = choice
        # the log per annotation, in _get_prompts' (image, category, file order) order: b | m | m p+ (a point annotation always has >= 1 point)
        types, num_points, i = [], [], 0
        while i < len(log):
            j = i + 1
            while j < len(log) and log[j] == "p":
                j += 1
            types.append("bbox" if log[i] == "b" else ("point" if j > i + 1 else "mask"))
            num_points.append(j - i - 1)
            i = j
        assert sum(num_points) == len(ranks)
        order = [a["id"] for img in image_ids for cat in CAT_IDS for a in ds.img2cat_annotations[img].get(cat, [])]
        assert len(order) == len(types), (len(order), len(types))
        pp = ds.prompts_processor
        tb, fb = U.annotations_to_tensor(pp, bboxes, img_sizes, PromptType.BBOX)
        tm, fm = U.annotations_to_tensor(pp, masks, img_sizes, PromptType.MASK)
        tp, fp = U.annotations_to_tensor(pp, points, img_sizes, PromptType.POINT)
        fe = U.flags_merge(fm, fp, fb)
        gts = ds.compute_ground_truths(image_ids, CAT_IDS)
        max_dims = torch.max(torch.tensor(img_sizes), 0).values.tolist()
        stacked = torch.stack([U.collate_gts(x, max_dims) for x in gts])
        for i, (h, w) in enumerate(SIZES):                                   # the padding is 0: only the image's own window is stored
            pad = stacked[i].clone()
            pad[:h, :w] = 0
            assert float(pad.abs().max()) == 0 and torch.equal(stacked[i, :h, :w].long(), gts[i])
        if gts_seen is not None:
            assert all(torch.equal(a, b) for a, b in zip(gts, gts_seen))
        gts_seen = gts
        assert set(tm.unique().tolist()) <= {0.0, 1.0}
        tensors[f"{tag}.prompt_masks_bits"] = torch.from_numpy(np.packbits(tm.numpy().astype(np.uint8).reshape(-1)))
        tensors[f"{tag}.flag_masks"] = fm.contiguous()
        tensors[f"{tag}.prompt_points"], tensors[f"{tag}.flag_points"] = tp.contiguous(), fp.contiguous()
        tensors[f"{tag}.prompt_bboxes"], tensors[f"{tag}.flag_bboxes"] = tb.contiguous(), fb.contiguous()
        tensors[f"{tag}.flag_examples"] = fe.to(torch.uint8).contiguous()
        meta["episodes"][tag] = {
            "seed": seed, "custom_preprocess": tag == "custom1", "annotation_order": order, "types": types, "num_points": num_points, "ranks": ranks,
            "boxes": [[[float(v) for v in b] for b in np.asarray(bboxes[i][cat]).reshape(-1, 4).tolist()] for i in image_ids for cat in CAT_IDS],
            "classes": classes, "prompt_masks_shape": list(tm.shape),
        }
        print(tag, "types", {t: types.count(t) for t in set(types)}, "points", len(ranks), "A_points", tp.shape[2], "A_boxes", tb.shape[2])
    for i, g in enumerate(gts_seen):
        tensors[f"gt.{i}"] = g.to(torch.uint8).contiguous()
    for i in image_ids:                                                       # the numpy definition of the decode, in file order
        dense = np.stack([decode(a["segmentation"]) for a in anns if a["image_id"] == i and a["category_id"] in CAT_IDS])
        tensors[f"decoded_bits.{i}"] = torch.from_numpy(np.packbits(dense.reshape(-1)))
    save_file(tensors, os.path.join(ROOT, "tests", "golden", "rle_episode.safetensors"))
    with open(os.path.join(ROOT, "tests", "golden", "rle_episode.json"), "w") as f:
        json.dump(meta, f, separators=(",", ":"))
    print("written", len(tensors), "tensors,", sum(v.numel() * v.element_size() for v in tensors.values()), "bytes")


if __name__ == "__main__":
    main()
