"""Host restatement (numpy) of the rle.hip kernels, written against the same definitions the kernels use: inclusive run ends, a
pixel's run = number of ends <= x * h + y, the torch "nearest" index rule in fp32, and the closed-form row / column counts of the
point search.  tests/test_rle_cpu.py checks it against the reference-produced fixture; tests/test_rle_gpu.py uses it for the cases
the fixture's random plan does not reach (explicit ranks)."""
import json
import os

import numpy as np
import torch
from safetensors.torch import load_file

from labelanything_amd.image_prep import resize_shape
from tests.helpers import GOLDEN


def load_fixture():
    with open(os.path.join(GOLDEN, "rle_episode.json")) as f:
        meta = json.load(f)
    return meta, load_file(os.path.join(GOLDEN, "rle_episode.safetensors"))


def definition_decode(counts, h, w):
    """The COCO format's definition: runs alternate 0 / 1 from a 0-run, column-major."""
    c = np.asarray(counts, dtype=np.int64)
    return np.repeat(np.arange(c.size) & 1, c).astype(np.uint8).reshape(w, h).T.copy()


def scan(counts):
    c = np.asarray(counts, dtype=np.int64)
    return np.cumsum(c), int(c[1::2].sum())


def covered(ends, pos):
    return (np.searchsorted(ends, pos, side="right") & 1).astype(np.uint8)


def decode(ends, h, w):
    y, x = np.mgrid[0:h, 0:w]
    return covered(ends, x * h + y)


def nearest_src(dst, in_size, out_size):
    dst = np.asarray(dst, dtype=np.int64)
    if out_size == in_size:
        return dst
    if out_size == 2 * in_size:
        return dst >> 1
    scale = np.float32(in_size) / np.float32(out_size)
    return np.minimum(np.floor(dst.astype(np.float32) * scale).astype(np.int64), in_size - 1)


def prompt_mask(ends_list, h, w, side, mask_side, custom):
    """One (image, class slot): fp32 [mask_side, mask_side] and its flag."""
    o = np.arange(mask_side)
    if custom:
        nh, nw = resize_shape(h, w, side, True, False)
        py, px = nearest_src(o, side, mask_side), nearest_src(o, side, mask_side)
        iy, ix = py < nh, px < nw
        sy, sx = nearest_src(np.minimum(py, nh - 1), h, nh), nearest_src(np.minimum(px, nw - 1), w, nw)
    else:
        iy = ix = np.ones(mask_side, dtype=bool)
        sy, sx = nearest_src(o, h, mask_side), nearest_src(o, w, mask_side)
    pos = sx[None, :] * h + sy[:, None]
    v = np.zeros((mask_side, mask_side), dtype=np.uint8)
    for ends in ends_list:
        v |= covered(ends, pos)
    v &= (iy[:, None] & ix[None, :]).astype(np.uint8)
    return v.astype(np.float32), int(v.any())


def ground_truth(anns, h, w, hmax, wmax):
    """anns: (ends, class slot) in file order; the last covering annotation wins."""
    out = np.zeros((hmax, wmax), dtype=np.int64)
    y, x = np.mgrid[0:h, 0:w]
    pos = x * h + y
    done = np.zeros((h, w), dtype=bool)
    for ends, slot in reversed(list(anns)):
        hit = covered(ends, pos).astype(bool) & ~done
        out[:h, :w][hit] = slot
        done |= hit
    return out


def point(ends, h, w, rank):
    """The rank-th set pixel in row-major order as (x, y), by the kernel's two bisections."""
    a, b = np.concatenate(([0], ends[:-1]))[1::2], ends[1::2]           # [start, end) of the 1-runs

    def rows_below(y):
        return int(((b // h) * y + np.minimum(b % h, y) - (a // h) * y - np.minimum(a % h, y)).sum())

    lo, hi = 0, h - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        lo, hi = (lo, mid) if rows_below(mid + 1) > rank else (mid + 1, hi)
    y = lo
    rem = rank - rows_below(y)

    def cols_before(x):
        q = lambda p: np.minimum(x, np.where(p > y, (p - y + h - 1) // h, 0))       # noqa: E731
        return int((q(b) - q(a)).sum())

    lo, hi = 0, w - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        lo, hi = (lo, mid) if cols_before(mid + 1) > rem else (mid + 1, hi)
    return lo, y


def scaled_point(x, y, h, w, side, custom):
    nh, nw = resize_shape(h, w, side, True, False) if custom else (side, side)
    return np.float32(np.float64(x) * (nw / w)), np.float32(np.float64(y) * (nh / h))


def unpack_bits(t: torch.Tensor, shape):
    n = int(np.prod(shape))
    return np.unpackbits(t.numpy())[:n].reshape(shape)


def fixture_packed(meta):
    """The fixture's annotations as a reference dataset holds them (per image, file order) -> PackedRles.  Every other compressed
    string is handed over as ``bytes``, the form pycocotools returns."""
    from labelanything_amd.annotations import pack_episode
    sizes = [tuple(s) for s in meta["sizes"]]
    per_image = [[] for _ in sizes]
    for a in meta["annotations"]:
        a = dict(a)
        c = a["segmentation"]["counts"]
        if isinstance(c, str) and a["id"] % 2:
            a["segmentation"] = {"size": a["segmentation"]["size"], "counts": c.encode("ascii")}
        per_image[a["image_id"]].append(a)
    return pack_episode(per_image, sizes, meta["cat_ids"])


def fixture_plan(meta, tag, packed):
    """The reference's recorded decisions of episode ``tag`` in plan_prompts' form (packed annotation indices)."""
    ep = meta["episodes"][tag]
    index_of = {packed.info[k]["id"]: k for k in range(len(packed))}
    order = [index_of[i] for i in ep["annotation_order"]]
    types = [None] * len(packed)
    draws, ranks = [], iter(ep["ranks"])
    for k, t, n in zip(order, ep["types"], ep["num_points"]):
        types[k] = t
        draws += [(k, next(ranks)) for _ in range(n)]
    boxes, flat = [], iter([b for pair in ep["boxes"] for b in pair])
    for k, t in zip(order, ep["types"]):
        if t == "bbox":
            boxes.append((k, next(flat)))
    return {"types": types, "boxes": boxes, "draws": draws, "classes": ep["classes"]}


def host_episode(packed, plan, side, custom, mask_side=256):
    """prompt masks + flags, points + flags and ground truths of an episode through the restated kernels."""
    n, c = packed.n_images, packed.n_classes
    ends = [scan(packed.runs[m[0]:m[0] + m[1]])[0] for m in packed.meta]
    masks, fm = np.zeros((n, c, mask_side, mask_side), dtype=np.float32), np.zeros((n, c), dtype=np.uint8)
    for i in range(n):
        h, w = (int(v) for v in packed.img_hw[i])
        for s in range(c):
            sel = [ends[k] for k in range(len(packed)) if packed.meta[k, 4] == i and packed.meta[k, 5] == s and plan["types"][k] == "mask"]
            masks[i, s], fm[i, s] = prompt_mask(sel, h, w, side, mask_side, custom)
    filled = {}
    rows = []
    for k, rank in plan["draws"]:
        pair = (int(packed.meta[k, 4]), int(packed.meta[k, 5]))
        rows.append((k, rank, pair, filled.get(pair, 0)))
        filled[pair] = filled.get(pair, 0) + 1
    a = max(filled.values(), default=0)
    pts, fp = np.zeros((n, c, a, 2), dtype=np.float32), np.zeros((n, c, a), dtype=np.uint8)
    for k, rank, (i, s), pos in rows:
        h, w = int(packed.meta[k, 2]), int(packed.meta[k, 3])
        pts[i, s, pos] = scaled_point(*point(ends[k], h, w, rank), h, w, side, custom)
        fp[i, s, pos] = 1
    hmax, wmax = int(packed.img_hw[:, 0].max()), int(packed.img_hw[:, 1].max())
    gts = np.zeros((n, hmax, wmax), dtype=np.int64)
    for i in range(n):
        ks = sorted((k for k in range(len(packed)) if packed.meta[k, 4] == i), key=lambda k: packed.meta[k, 6])
        gts[i] = ground_truth([(ends[k], int(packed.meta[k, 5])) for k in ks], int(packed.img_hw[i, 0]), int(packed.img_hw[i, 1]), hmax, wmax)
    return masks, fm, pts, fp, gts


def fixture_ground_truths(meta, gold):
    sizes = meta["sizes"]
    hmax, wmax = max(s[0] for s in sizes), max(s[1] for s in sizes)
    out = torch.zeros(len(sizes), hmax, wmax, dtype=torch.int64)
    for i, (h, w) in enumerate(sizes):
        out[i, :h, :w] = gold[f"gt.{i}"].long()
    return out
