"""Query substitution (experiment/substitution.py): every image of an episode takes a turn as the query, and after each step one
corrective point per class is sampled from the current prediction's errors and attached to that image's prompts.

``generate_points_from_errors`` replaces the reference's sampler (substitution.py:17-97: one-hot tensors, ``torch.nonzero``,
``torch.unique``, host set arithmetic, one ``torch.randint`` per (image, class)) plus ``PromptsProcessor.torch_apply_coords``
(data/transforms.py:176-191) by two HIP launches (la_error_count, la_error_points in csrc/subst.hip) with no host sync.

Differences from the reference, on purpose:

* Random stream.  Without explicit ``ranks`` the k-th draw of (b, c) is rank = min(floor(u * count), count - 1) with
  u = ``torch.rand(..., generator=generator)`` on the device: uniform over the class's error pixels like the reference's CPU
  ``torch.randint(0, count)``, but a different sequence of numbers.
* Row order.  The reference sorts its rows by ``b * B + c`` where ``b * C + c`` is meant (substitution.py:83).  That key collides
  when B >= 2 and C > B: with C > B + 1 points land on the wrong (b, c); with C = B + 1 they do when class B of an image has no
  errors (its zero row is appended last and sorts after (b + 1, 0)).  Here every (b, c) gets its own k-th error pixel.  Where the
  reference's key is injective the two agree bit for bit.
* Empty classes with ``num_points > 1``.  The reference emits one row for an absent (b, c) and then fails to reshape; here such a
  class gets ``num_points`` zero points with label 0.
* Ground-truth values outside [0, C) other than ``ignore_index`` count as class 0 (``one_hot`` raises on them in the reference).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch

from . import _lib as L

Tensor = torch.Tensor

TILE = 4096          # pixels per tile of la_error_count / la_error_points


def _check_device(*ts: Optional[Tensor]) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("generate_points_from_errors needs device tensors (there is no CPU path)")


def predict_labels(prediction: Tensor, ground_truth: Tensor, out: Optional[Tensor] = None, ignore_index: int = -100) -> Tensor:
    """argmax over dim 1 (first maximal index) of fp32 logits [B, C, H, W] -> int64 [B, H, W], by la_error_count's streaming pass."""
    _check_device(prediction, ground_truth)
    b, c, h, w = prediction.shape
    logits = prediction.float().contiguous()
    gt = ground_truth.to(torch.int64).contiguous()
    counts = torch.empty(b, c, -(-(h * w) // TILE), dtype=torch.int32, device=logits.device)
    out = out if out is not None else torch.empty(b, h, w, dtype=torch.int64, device=logits.device)
    with torch.cuda.device(logits.device):
        L.error_count(logits, gt, b, c, h, w, ignore_index, counts, out)
    return out


def generate_points_from_errors(prediction: Tensor, ground_truth: Tensor, num_points: int, ignore_index: int = -100, *,
                                ranks: Optional[Tensor] = None, u: Optional[Tensor] = None, generator: Optional[torch.Generator] = None,
                                dims: Optional[Tensor] = None, long_side_length: int = 1024, custom_preprocess: bool = True,
                                preds_out: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """prediction fp32 logits [B, C, H, W], ground_truth int64 [B, H, W] (``ignore_index`` read as class 0) -> (points fp32
    [B, C, n, 2] as (x, y), labels fp32 [B, C, n]): for each (b, c) ``num_points`` draws over its error pixels in raster order, +1 for a
    false negative, -1 for a false positive, 0 for the background class and for a class without errors (whose points are zero).

    Rank sources: ``ranks`` int32 [B, C, n] (clamped into [0, count)), else uniforms ``u`` fp32 [B, C, n], else
    ``torch.rand(B, C, n, generator=generator)`` on the device (see the module docstring: not the reference's random stream).
    dims: int64 [B, 2] or [B, K, 2] original (H, W) per image (row 0 is used, as the reference's ``dim[0]``); the points are then
    scaled into the network input frame as ``torch_apply_coords(points, dims[b, 0])`` with ``long_side_length`` /
    ``custom_preprocess``.  Without dims they stay in pixel units.  preds_out: int64 [B, H, W] receives the argmax.
    Two launches, no host sync: capturable in a HIP graph when ``ranks`` or ``u`` is given."""
    _check_device(prediction, ground_truth, ranks, u, preds_out)
    if prediction.dim() != 4 or ground_truth.shape != (prediction.shape[0],) + tuple(prediction.shape[2:]):
        raise ValueError(f"prediction [B, C, H, W] and ground_truth [B, H, W] expected, got {tuple(prediction.shape)} and "
                         f"{tuple(ground_truth.shape)}")
    b, c, h, w = prediction.shape
    n = int(num_points)
    dev = prediction.device
    logits = prediction.float().contiguous()
    gt = ground_truth.to(torch.int64).contiguous()
    if preds_out is not None and (preds_out.dtype != torch.int64 or tuple(preds_out.shape) != (b, h, w) or not preds_out.is_contiguous()):
        raise ValueError("preds_out must be a contiguous int64 [B, H, W] tensor")
    if n <= 0:
        if preds_out is not None:
            predict_labels(logits, gt, preds_out, ignore_index)
        return torch.zeros(b, c, 0, 2, device=dev), torch.zeros(b, c, 0, device=dev)
    if ranks is not None:
        ranks = ranks.to(device=dev, dtype=torch.int32).contiguous()
        if tuple(ranks.shape) != (b, c, n):
            raise ValueError(f"ranks must be [B, C, num_points] = {(b, c, n)}, got {tuple(ranks.shape)}")
    else:
        if u is None:
            u = torch.rand(b, c, n, generator=generator, device=dev)
        u = u.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(u.shape) != (b, c, n):
            raise ValueError(f"u must be [B, C, num_points] = {(b, c, n)}, got {tuple(u.shape)}")
    dims_stride = 0
    if dims is not None:
        dims = dims.to(device=dev, dtype=torch.int64, non_blocking=True).contiguous()
        if dims.dim() not in (2, 3) or dims.shape[0] != b or dims.shape[-1] != 2:
            raise ValueError(f"dims must be [B, 2] or [B, K, 2], got {tuple(dims.shape)}")
        dims_stride = dims[0].numel()
    counts = torch.empty(b, c, -(-(h * w) // TILE), dtype=torch.int32, device=dev)
    points = torch.zeros(b, c, n, 2, device=dev)
    labels = torch.zeros(b, c, n, device=dev)
    with torch.cuda.device(dev):
        L.error_count(logits, gt, b, c, h, w, ignore_index, counts, preds_out)
        L.error_points(logits, gt, b, c, h, w, ignore_index, counts, n, ranks, u if ranks is None else None, dims, dims_stride,
                       int(long_side_length), bool(custom_preprocess), points, labels)
    return points, labels


class Substitutor:
    """Cycles every image of the episode through the query slot (experiment/substitution.py:100-276).

    ``reset((batch, ground_truths))`` takes the dataset's batch: prompts, flags and dims for all M+1 images ([B, M+1, ...]) and
    ground truths [B, M+1, H, W].  Iterating yields (model input, query ground truth) M+2 times - the original query, M rotations,
    the original query again - or once with ``substitute=False``.  Each rotation is applied to the already rotated batch, as in the
    reference, so with M+1 >= 4 the supports end in another order than they started.  ``generate_new_points(logits, gt)`` appends
    ``num_points`` error points per class to the current query's prompts (the other images get zero padding, labels 0).

    generator: the random stream of the device sampler (see ``generate_points_from_errors``)."""

    torch_keys_to_exchange = ["prompt_points", "prompt_masks", "prompt_bboxes", "flag_masks", "flag_bboxes", "flag_points",
                              "flag_examples", "dims"]
    torch_keys_to_separate = ["prompt_points", "prompt_masks", "prompt_bboxes", "flag_masks", "flag_bboxes", "flag_points",
                              "flag_examples"]
    list_keys_to_exchange = ["intended_classes", "classes", "image_ids"]
    list_keys_to_separate: List[str] = []

    def __init__(self, threshold: Optional[float] = None, num_points: int = 1, substitute: bool = True, long_side_length: int = 1024,
                 custom_preprocess: bool = True, *, generator: Optional[torch.Generator] = None) -> None:
        if threshold is not None:
            # the reference's calculate_if_substitute reaches mean_pairwise_j_index, which experiment/substitution.py never imports
            raise NotImplementedError("Substitutor(threshold=...) is not built: the reference's substitution_threshold heuristic "
                                      "cannot run either (mean_pairwise_j_index is undefined there)")
        self.example_classes = None
        self.threshold = threshold
        self.num_points = int(num_points)
        self.substitute = bool(substitute)
        self.long_side_length = int(long_side_length)
        self.custom_preprocess = bool(custom_preprocess)
        self.generator = generator
        self.it = 0
        self.batch: Dict[str, Any] = {}
        self.ground_truths: Optional[Tensor] = None
        self._index_cache: Dict[Tuple[str, int, int], Tensor] = {}

    def reset(self, batch: Tuple[Dict[str, Any], Tensor]) -> None:
        self.it = 0
        data, self.ground_truths = batch
        self.batch = dict(data)
        self.example_classes = self.batch.get("classes")

    @property
    def num_examples(self) -> int:
        if "embeddings" in self.batch:
            if isinstance(self.batch["embeddings"], dict):
                raise NotImplementedError("dict-valued embeddings (feature pyramids) are not supported")
            return int(self.batch["embeddings"].shape[1])
        if "images" in self.batch:
            return int(self.batch["images"].shape[1])
        raise ValueError("the batch needs 'images' or 'embeddings'")

    @property
    def num_steps(self) -> int:
        """Steps one batch yields: M+2, or 1 with substitute=False."""
        return self.num_examples + 1 if self.substitute else 1

    def __iter__(self):
        return self

    def _order(self) -> List[int]:
        m1 = self.num_examples
        if self.it == m1:                                  # the original query becomes the query again
            return [m1 - 1] + list(range(1, m1 - 1)) + [0]
        return [self.it] + list(range(0, self.it)) + list(range(self.it + 1, m1))

    def _index(self, order: List[int], device) -> Tensor:
        key = (str(device), len(order), self.it)
        t = self._index_cache.get(key)
        if t is None:
            t = torch.tensor(order, dtype=torch.long, device=device)
            self._index_cache[key] = t
        return t

    def generate_new_points(self, prediction: Tensor, ground_truth: Tensor, *, ranks: Optional[Tensor] = None,
                            preds_out: Optional[Tensor] = None) -> None:
        """Sample ``num_points`` error points per class of the current query (dim-1 index 0) and concatenate them to
        ``prompt_points`` / ``flag_points`` along the point dimension; every other image gets zeros.  ``flag_examples`` is left as
        it is (as in the reference).  ranks: explicit draws, int32 [B, C, num_points] (tests).
        Keep the batch on the device (``LamTrainer.substitution_steps`` moves it there): the points are made on the logits' device and
        a host-resident ``prompt_points`` / ``flag_points`` costs a device-to-host copy - a host sync - on every call."""
        if not (self.substitute and self.num_points > 0):
            if preds_out is not None:
                predict_labels(prediction, ground_truth, preds_out)
            return
        points, labels = generate_points_from_errors(
            prediction, ground_truth, self.num_points, ranks=ranks, generator=self.generator, dims=self.batch["dims"],
            long_side_length=self.long_side_length, custom_preprocess=self.custom_preprocess, preds_out=preds_out)
        pp, fp = self.batch["prompt_points"], self.batch["flag_points"]
        points, labels = points.to(pp.device), labels.to(fp.device)
        b, c, n = labels.shape
        new_points = torch.zeros(b, pp.shape[1], c, n, 2, device=pp.device)
        new_points[:, 0] = points
        new_labels = torch.zeros(b, fp.shape[1], c, n, device=fp.device)
        new_labels[:, 0] = labels
        self.batch["prompt_points"] = torch.cat([pp, new_points], dim=3)
        self.batch["flag_points"] = torch.cat([fp, new_labels], dim=3)

    def divide_query_examples(self) -> Tuple[Dict[str, Any], Tensor]:
        out: Dict[str, Any] = {}
        for key in self.torch_keys_to_separate:
            if key in self.batch:
                out[key] = self.batch[key][:, 1:]
        for key in self.list_keys_to_separate:
            if key in self.batch:
                out[key] = [elem[1:] for elem in self.batch[key]]
        for key in self.batch.keys() - set(self.torch_keys_to_separate + self.list_keys_to_separate):
            out[key] = self.batch[key]
        return out, self.ground_truths[:, 0]

    def __next__(self) -> Tuple[Dict[str, Any], Tensor]:
        if self.it == 0:
            self.it = 1
            return self.divide_query_examples()
        if not self.substitute or self.it == self.num_examples + 1:
            raise StopIteration
        order = self._order()
        keys = [k for k in self.torch_keys_to_exchange + ["images", "embeddings"] if k in self.batch]
        for key in keys:
            self.batch[key] = torch.index_select(self.batch[key], 1, self._index(order, self.batch[key].device))
        for key in self.list_keys_to_exchange:
            if self.batch.get(key) is None:
                continue
            self.batch[key] = [[elem[i] for i in order] for elem in self.batch[key]]
        self.ground_truths = torch.index_select(self.ground_truths, 1, self._index(order, self.ground_truths.device))
        self.it += 1
        return self.divide_query_examples()
