"""Episode prompts and ground truths built on the device from COCO run-length (RLE) annotations.

The reference decodes every annotation into a dense ``H x W`` array on the host (``PromptsProcessor.convert_mask``,
data/transforms.py:123-150) and derives everything else from it: the per-class mask prompt (``apply_masks``, :203-224), the point
prompts (``sample_point``, :152-157) and the label map (``compute_ground_truths``, data/coco.py:514-544).  Here the runs are packed
into one int32 buffer, uploaded once, and the kernels of csrc/rle.hip answer "is pixel (x, y) of annotation k set" from the runs, so
the dense masks exist nowhere unless ``RleBatch.decode`` is asked for them.

Host side (this module, numpy / plain Python): the RLE string codec, packing with the reference's empty-mask rule, and
``plan_prompts`` - the random decisions of ``_get_prompts`` (data/coco.py:397-477) drawn from the same generators in the same
order.  The decoder and the string codec follow the published COCO format; see DESIGN.md for what is and is not pinned.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .image_prep import resize_shape

BBOX, MASK, POINT = "bbox", "mask", "point"
META = 8          # ints per annotation record: run offset, run count, h, w, image, class slot, order within the image, reserved


# ---- the COCO RLE format ------------------------------------------------------------------------------------------------------
def rle_to_string(counts: Sequence[int]) -> bytes:
    """Compressed form of a count list: from the fourth count on the difference to the count two places earlier is stored; every
    value goes out in 5-bit groups, least significant first, as chr(48 + bits), 0x20 = more groups follow, 0x10 of the last group =
    sign."""
    out = bytearray()
    cnts = [int(c) for c in counts]
    for i, x in enumerate(cnts):
        if i > 2:
            x -= cnts[i - 2]
        more = True
        while more:
            c = x & 0x1F
            x >>= 5
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(c + 48)
    return bytes(out)


def rle_from_string(s) -> np.ndarray:
    """Counts (int64) of a compressed RLE string (``bytes`` or ``str``)."""
    data = s.encode("ascii") if isinstance(s, str) else bytes(s)
    cnts: List[int] = []
    p = 0
    while p < len(data):
        x, k, more = 0, 0, True
        while more:
            if p >= len(data):
                raise ValueError("truncated RLE string")
            c = data[p] - 48
            if not 0 <= c < 64:
                raise ValueError(f"byte {data[p]} at position {p} is outside the RLE alphabet")
            x |= (c & 0x1F) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return np.asarray(cnts, dtype=np.int64)


def rle_from_mask(mask) -> Dict[str, Any]:
    """Uncompressed RLE of a 2-D mask (non-zero = set): column-major runs that start with a (possibly empty) 0-run."""
    m = np.asarray(mask)
    if m.ndim != 2 or m.size == 0:
        raise ValueError("rle_from_mask wants a non-empty [H, W] array")
    f = (m != 0).ravel(order="F")
    edges = np.flatnonzero(f[1:] != f[:-1]) + 1
    counts = np.diff(np.concatenate(([0], edges, [f.size])))
    if f[0]:
        counts = np.concatenate(([0], counts))
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": [int(c) for c in counts]}


def as_rle(segm, h: int, w: int) -> Dict[str, Any]:
    """What ``PromptsProcessor.__ann_to_rle`` (data/transforms.py:74-94) hands to the decoder, as ``{"size", "counts": int64 array}``.
    Both RLE forms are read here; a polygon list goes through pycocotools (boundary tracing on the host, no dense decode) when it is
    importable."""
    if isinstance(segm, dict):
        counts = segm["counts"]
        counts = rle_from_string(counts) if isinstance(counts, (bytes, str)) else np.asarray(counts, dtype=np.int64).reshape(-1)
        size = [int(v) for v in segm.get("size", (h, w))]
        return {"size": size, "counts": counts}
    if isinstance(segm, (list, tuple)):
        try:
            from pycocotools import mask as mask_utils
        except ImportError:
            raise TypeError("a polygon segmentation has to be turned into an RLE first: "
                            "pycocotools.mask.merge(pycocotools.mask.frPyObjects(segmentation, h, w))") from None
        return as_rle(mask_utils.merge(mask_utils.frPyObjects(list(segm), h, w)), h, w)
    raise TypeError(f"unsupported segmentation of type {type(segm).__name__}")


# ---- packing ------------------------------------------------------------------------------------------------------------------
@dataclass
class PackedRles:
    """An episode's annotations laid out for one upload (host arrays).  ``meta[k]`` = (run offset, run count, h, w, image, class slot,
    order within the image, 0); ``area[k]`` = set pixels of annotation k after the empty-mask rule (always >= 1)."""
    runs: np.ndarray
    meta: np.ndarray
    area: np.ndarray
    img_hw: np.ndarray
    n_classes: int
    names: List[str]
    info: List[Optional[Dict[str, Any]]] = field(default_factory=list)
    cat_ids: Optional[List[Any]] = None

    @property
    def n_images(self) -> int:
        return int(self.img_hw.shape[0])

    def __len__(self) -> int:
        return int(self.meta.shape[0])


def pack_rles(rles: Sequence[Any], image_index: Sequence[int], class_slot: Sequence[int], sizes: Sequence[Tuple[int, int]],
              n_classes: Optional[int] = None, order: Optional[Sequence[int]] = None,
              fallbacks: Optional[Sequence[Optional[Tuple[int, int]]]] = None, names: Optional[Sequence[str]] = None,
              info: Optional[Sequence[Optional[Dict[str, Any]]]] = None, cat_ids: Optional[Sequence[Any]] = None) -> PackedRles:
    """rles[k]: RLE dict (either form) of an annotation of image ``image_index[k]`` (size ``sizes[image]`` = (h, w)) and class slot
    ``class_slot[k]``; ``order[k]`` = its place in the image's annotation file order (default: order of appearance).
    An annotation without a set pixel becomes the single pixel ``fallbacks[k]`` = (x, y) clamped into the image, default (0, 0)
    (data/transforms.py:136-149: the reference clamps the first polygon vertex) - the runs are rewritten here, so the kernels never see
    an empty annotation."""
    k_total = len(rles)
    if not (len(image_index) == len(class_slot) == k_total):
        raise ValueError("rles, image_index and class_slot must have one entry per annotation")
    n = len(sizes)
    names = [str(v) for v in names] if names is not None else [f"annotation {k}" for k in range(k_total)]
    c = int(n_classes) if n_classes is not None else (max((int(s) for s in class_slot), default=0) + 1)
    if not 0 < c <= 255:
        raise ValueError(f"{c} class slots: the ground-truth kernel carries a class slot in one byte")
    for i, (h, w) in enumerate(sizes):
        if h <= 0 or w <= 0 or int(h) * int(w) >= 2 ** 31:
            raise ValueError(f"image {i}: size {h} x {w} is not in (0, 2^31) pixels")
    seen = [0] * n
    meta = np.zeros((k_total, META), dtype=np.int32)
    area = np.zeros(k_total, dtype=np.int64)
    chunks, off = [], 0
    for k in range(k_total):
        img, slot = int(image_index[k]), int(class_slot[k])
        if not 0 <= img < n:
            raise ValueError(f"{names[k]}: image index {img} outside [0, {n})")
        if not 0 <= slot < c:
            raise ValueError(f"{names[k]}: class slot {slot} outside [0, {c})")
        h, w = int(sizes[img][0]), int(sizes[img][1])
        rle = as_rle(rles[k], h, w)
        if list(rle["size"]) != [h, w]:
            raise ValueError(f"{names[k]}: RLE size {list(rle['size'])} does not match its image's {[h, w]}")
        counts = rle["counts"]
        if counts.size == 0 or (counts < 0).any():
            raise ValueError(f"{names[k]}: run lengths must be non-negative and not empty")
        if int(counts.sum()) != h * w:
            raise ValueError(f"{names[k]}: run lengths sum to {int(counts.sum())}, the image has {h} x {w} = {h * w} pixels")
        a = int(counts[1::2].sum())
        if a == 0:
            fx, fy = (0, 0) if fallbacks is None or fallbacks[k] is None else fallbacks[k]
            fx, fy = max(min(int(fx), w - 1), 0), max(min(int(fy), h - 1), 0)
            p = fx * h + fy
            counts = np.asarray([p, 1] + ([h * w - p - 1] if h * w - p - 1 else []), dtype=np.int64)
            a = 1
        meta[k] = (off, counts.size, h, w, img, slot, seen[img] if order is None else int(order[k]), 0)
        seen[img] += 1
        area[k] = a
        chunks.append(counts.astype(np.int32))
        off += counts.size
    runs = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.int32)
    return PackedRles(runs=runs, meta=meta, area=area, img_hw=np.asarray(sizes, dtype=np.int32).reshape(n, 2), n_classes=c, names=names,
                      info=list(info) if info is not None else [None] * k_total, cat_ids=list(cat_ids) if cat_ids is not None else None)


def pack_episode(img_annotations: Sequence[Sequence[Dict[str, Any]]], img_sizes: Sequence[Tuple[int, int]], cat_ids: Sequence[Any]) -> PackedRles:
    """From what a reference dataset holds: per image its annotation dicts IN FILE ORDER (``img_annotations[image_id]``: keys
    ``category_id``, ``segmentation``, and - for ``plan_prompts`` - ``bbox`` and ``area``) and the episode's ``cat_ids`` with the
    background (-1) first.  Annotations of other categories are left out, as in ``_get_prompts`` / ``compute_ground_truths``."""
    cat_ids = list(cat_ids)
    rles, imgs, slots, order, fb, names, info = [], [], [], [], [], [], []
    for i, anns in enumerate(img_annotations):
        for j, ann in enumerate(anns):
            if ann["category_id"] not in cat_ids:
                continue
            segm = ann["segmentation"]
            poly = isinstance(segm, (list, tuple))
            rles.append(as_rle(segm, *img_sizes[i]) if poly else segm)
            imgs.append(i)
            slots.append(cat_ids.index(ann["category_id"]))
            order.append(j)
            fb.append((int(segm[0][0]), int(segm[0][1])) if poly else None)
            names.append(f"annotation {ann.get('id', j)} of image {i}")
            info.append(ann)
    return pack_rles(rles, imgs, slots, img_sizes, n_classes=len(cat_ids), order=order, fallbacks=fb, names=names, info=info, cat_ids=cat_ids)


def _by_image_and_slot(packed: PackedRles) -> Dict[Tuple[int, int], List[int]]:
    """(image, class slot) -> annotation indices in file order: the reference's ``img2cat_annotations[image][category]``."""
    groups: Dict[Tuple[int, int], List[int]] = {}
    for k in np.lexsort((packed.meta[:, 6], packed.meta[:, 4])):
        groups.setdefault((int(packed.meta[k, 4]), int(packed.meta[k, 5])), []).append(int(k))
    return groups


# ---- the random decisions of _get_prompts ---------------------------------------------------------------------------------------
def plan_prompts(packed: PackedRles, possible_prompt_types: Sequence[str], max_points_annotations: int = 50,
                 max_points_per_annotation: int = 10, add_box_noise: bool = True) -> Dict[str, Any]:
    """``CocoLVISDataset._get_prompts`` (data/coco.py:397-477) without the masks: the same draws from the same generators (``random``
    and ``np.random`` - seed them like the reference), in the same order, with the same arguments.  Per (image, class) with
    annotations: ``random.choices`` for the prompt types (all MASK above ``max_points_annotations``); per box
    ``PromptsProcessor.convert_bbox`` with 4 x ``np.random.normal`` of noise (transforms.py:96-121); per point annotation
    ``np.random.poisson`` (``_sample_num_points``: the mean uses the annotation FILE's ``area``) and per point
    ``np.random.choice(n)`` with n = the DECODED mask's set pixels (``sample_point``) - the two areas can differ.
    Returns ``types`` (per annotation), ``boxes`` [(annotation, [x1, y1, x2, y2])], ``draws`` [(annotation, rank)], ``classes``."""
    types_in = [str(getattr(t, "value", t)).lower() for t in possible_prompt_types]
    groups = _by_image_and_slot(packed)
    types: List[Optional[str]] = [None] * len(packed)
    boxes: List[Tuple[int, List[float]]] = []
    draws: List[Tuple[int, int]] = []
    classes: List[List[Any]] = [[] for _ in range(packed.n_images)]
    for i in range(packed.n_images):
        h, w = int(packed.img_hw[i, 0]), int(packed.img_hw[i, 1])
        for slot in range(packed.n_classes):
            anns = groups.get((i, slot))
            if not anns:
                continue
            classes[i].append(packed.cat_ids[slot] if packed.cat_ids is not None else slot)
            chosen = [MASK] * len(anns) if len(anns) > max_points_annotations else random.choices(types_in, k=len(anns))
            for k, t in zip(anns, chosen):
                types[k] = t
                ann = packed.info[k]
                if t == BBOX:
                    x, y, wb, hb = ann["bbox"]
                    x1, y1, x2, y2 = x, y, x + wb, y + hb
                    if add_box_noise:
                        n1 = np.clip(np.random.normal(0, 0.1 * wb), -20, 20)
                        n2 = np.clip(np.random.normal(0, 0.1 * hb), -20, 20)
                        n3 = np.clip(np.random.normal(0, 0.1 * wb), -20, 20)
                        n4 = np.clip(np.random.normal(0, 0.1 * hb), -20, 20)
                        x1, y1 = float(np.clip(x1 + n1, 0, w)), float(np.clip(y1 + n2, 0, h))
                        x2, y2 = float(np.clip(x2 + n3, 0, w)), float(np.clip(y2 + n4, 0, h))
                    boxes.append((k, [x1, y1, x2, y2]))
                elif t == POINT:
                    mean = max_points_per_annotation * np.sqrt(ann["area"] / (h * w))
                    for _ in range(int(np.clip(np.random.poisson(mean) + 1, 1, max_points_per_annotation))):
                        draws.append((k, int(np.random.choice(int(packed.area[k])))))
                elif t != MASK:
                    raise ValueError(f"unknown prompt type {t!r}")
    return {"types": types, "boxes": boxes, "draws": draws, "classes": classes}


# ---- the device side ----------------------------------------------------------------------------------------------------------
class RleBatch:
    """A packed episode on the device: one pinned buffer, one non-blocking copy, one ``la_rle_scan``.  After that nothing here reads
    device memory from the host; every method is a thin wrapper over one kernel on the current stream."""

    def __init__(self, packed: PackedRles, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("run-length annotations are rasterised on the device: pass device='cuda'")
        if len(packed) == 0:
            raise ValueError("an RleBatch needs at least one annotation")
        self.packed = packed
        k, n, r = len(packed), packed.n_images, int(packed.runs.size)
        by_image = np.lexsort((packed.meta[:, 6], packed.meta[:, 4])).astype(np.int32)       # per image, file order
        count = np.bincount(packed.meta[:, 4], minlength=n).astype(np.int32)
        first = (np.cumsum(count) - count).astype(np.int32)
        buf = self._upload(np.concatenate([packed.runs, packed.meta.ravel(), packed.img_hw.ravel(), first, count, by_image]))
        parts = torch.split(buf, [r, k * META, 2 * n, n, n, k])
        self.runs, self.meta, self.img_hw, self._gt_first, self._gt_count, self._gt_index = parts
        self.ends = torch.empty(r, dtype=torch.int32, device=self.device)
        self.area = torch.empty(k, dtype=torch.int32, device=self.device)
        self._new_hw: Dict[Tuple[int, bool], torch.Tensor] = {}
        with torch.cuda.device(self.device):
            L.rle_scan(self.runs, self.meta, k, self.ends, self.area)

    def _upload(self, arr: np.ndarray) -> torch.Tensor:
        host = torch.empty(arr.size, dtype=torch.int32).pin_memory()
        host.numpy()[:] = arr
        return host.to(self.device, non_blocking=True)

    def _geometry(self, side: int, custom_preprocess: bool) -> torch.Tensor:
        key = (int(side), bool(custom_preprocess))
        if key not in self._new_hw:
            hw = [resize_shape(int(h), int(w), side, True, False) if custom_preprocess else (side, side) for h, w in self.packed.img_hw]
            self._new_hw[key] = self._upload(np.asarray(hw, dtype=np.int32).ravel())
        return self._new_hw[key]

    def decode(self, indices: Optional[Sequence[int]] = None) -> torch.Tensor:
        """Dense uint8 [k, H, W] masks of the chosen annotations (default: all), which must share one size."""
        idx = list(range(len(self.packed))) if indices is None else [int(i) for i in indices]
        if not idx or not all(0 <= i < len(self.packed) for i in idx):
            raise IndexError(f"annotation indices must be a non-empty subset of [0, {len(self.packed)})")
        sizes = {(int(self.packed.meta[i, 2]), int(self.packed.meta[i, 3])) for i in idx}
        if len(sizes) != 1:
            raise ValueError(f"decode wants annotations of one size, got {sorted(sizes)}")
        (h, w), = sizes
        out = torch.empty(len(idx), h, w, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            L.rle_decode(self.ends, self.meta, self._upload(np.asarray(idx, dtype=np.int32)), len(idx), h, w, out)
        return out

    def prompt_masks(self, select: Optional[Sequence[bool]] = None, side: int = 1024, mask_side: int = 256,
                     custom_preprocess: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """(fp32 [N, C, mask_side, mask_side], uint8 [N, C]): per (image, class slot) the union of its annotations with a true
        ``select`` entry (default: all) through ``apply_masks`` - the whole episode in one launch."""
        p = self.packed
        n, c, k = p.n_images, p.n_classes, len(p)
        keep = np.ones(k, dtype=bool) if select is None else np.asarray(select, dtype=bool).reshape(-1)
        if keep.size != k:
            raise ValueError(f"select has {keep.size} entries for {k} annotations")
        pair = (p.meta[:, 4].astype(np.int64) * c + p.meta[:, 5])[keep]
        index = np.flatnonzero(keep)[np.argsort(pair, kind="stable")].astype(np.int32)
        count = np.bincount(pair, minlength=n * c).astype(np.int32)
        first = (np.cumsum(count) - count).astype(np.int32)
        lists = self._upload(np.concatenate([first, count, index, np.zeros(1, dtype=np.int32)]))
        out = torch.empty(n, c, mask_side, mask_side, dtype=torch.float32, device=self.device)
        flags = torch.zeros(n, c, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            L.rle_prompt_masks(self.ends, self.meta, lists[:n * c], lists[n * c:2 * n * c], lists[2 * n * c:], self.img_hw,
                               self._geometry(side, custom_preprocess), n, c, custom_preprocess, side, mask_side, out, flags)
        return out, flags

    def ground_truths(self) -> torch.Tensor:
        """int64 [N, Hmax, Wmax]: class slot of the last annotation (file order) covering each pixel; 0 elsewhere and in the padding."""
        n = self.packed.n_images
        hmax, wmax = int(self.packed.img_hw[:, 0].max()), int(self.packed.img_hw[:, 1].max())
        out = torch.empty(n, hmax, wmax, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            L.rle_ground_truth(self.ends, self.meta, self._gt_first, self._gt_count, self._gt_index, self.img_hw, n, hmax, wmax, out)
        return out

    def points(self, draws: Sequence[Tuple[int, int]], side: int = 1024, custom_preprocess: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """draws: (annotation, rank) pairs in prompt order; rank counts the annotation's set pixels in ``np.argwhere`` order.  Returns
        (fp32 [N, C, A, 2] of (x, y) in the network input frame, uint8 [N, C, A]), A = most draws any (image, class slot) has; the draws
        of a pair fill its row in the order given."""
        p = self.packed
        n, c = p.n_images, p.n_classes
        filled = np.zeros(n * c, dtype=np.int64)
        rows = []
        for k, rank in draws:
            k, rank = int(k), int(rank)
            if not 0 <= k < len(p):
                raise IndexError(f"draw on annotation {k} outside [0, {len(p)})")
            if not 0 <= rank < int(p.area[k]):
                raise IndexError(f"{p.names[k]}: rank {rank} outside [0, {int(p.area[k])})")
            pair = int(p.meta[k, 4]) * c + int(p.meta[k, 5])
            rows.append((k, rank, pair, int(filled[pair])))
            filled[pair] += 1
        a = int(filled.max()) if rows else 0
        pts = torch.zeros(n, c, a, 2, dtype=torch.float32, device=self.device)
        flags = torch.zeros(n, c, a, dtype=torch.uint8, device=self.device)
        if rows:
            d = np.asarray([(k, rank, pair * a + pos) for k, rank, pair, pos in rows], dtype=np.int32)
            with torch.cuda.device(self.device):
                L.rle_points(self.ends, self.meta, self.area, self._geometry(side, custom_preprocess), self._upload(d.ravel()), len(rows), pts, flags)
        return pts, flags


def episode_from_annotations(batch: RleBatch, plan: Dict[str, Any], side: int = 1024, mask_side: int = 256,
                             custom_preprocess: bool = True) -> Dict[str, Any]:
    """The per-episode dict ``collate_episodes`` takes (without images / embeddings), every tensor on the device: what
    ``CocoLVISDataset.__getitem__`` (data/coco.py:590-643) assembles from ``_get_prompts`` + ``annotations_to_tensor`` +
    ``compute_ground_truths`` + ``flags_merge``.  Boxes keep the host path of ``collate.annotations_to_tensor``."""
    from .collate import annotations_to_tensor
    from .prompts import flags_merge
    p = batch.packed
    n, c = p.n_images, p.n_classes
    masks, flag_masks = batch.prompt_masks([t == MASK for t in plan["types"]], side, mask_side, custom_preprocess)
    points, flag_points = batch.points(plan["draws"], side, custom_preprocess)
    per_pair: List[Dict[int, List[List[float]]]] = [{s: [] for s in range(c)} for _ in range(n)]
    for k, box in plan["boxes"]:
        per_pair[int(p.meta[k, 4])][int(p.meta[k, 5])].append(box)
    sizes = [(int(h), int(w)) for h, w in p.img_hw]
    bboxes, flag_bboxes = annotations_to_tensor([{s: np.asarray(v, dtype=np.float64).reshape(len(v), 4) for s, v in d.items()} for d in per_pair],
                                                sizes, BBOX, side=side, custom_preprocess=custom_preprocess, device=batch.device)
    return {
        "prompt_masks": masks, "flag_masks": flag_masks, "prompt_points": points, "flag_points": flag_points,
        "prompt_bboxes": bboxes, "flag_bboxes": flag_bboxes, "flag_examples": flags_merge(flag_masks, flag_points, flag_bboxes),
        "dims": torch.tensor(sizes, device=batch.device), "classes": plan["classes"], "ground_truths": batch.ground_truths(),
    }
