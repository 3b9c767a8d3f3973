"""The training-free cosine-similarity baseline of the reference (models/similarity.py, registry name ``similarity``; the recipe
parameters/validation/COCO/cosine.yaml) on the device.

logits[b, n, q] = the largest cosine between query pixel q and any support pixel of class n, on a compare_size x compare_size grid.
The reference materialises the [Q, K] similarity matrix per support image and one masked copy of it per class; here
``la_sim_prepare`` resamples, normalises and rounds the embeddings in one pass, ``la_sim_class_bits`` turns the prompt masks into one
class word per support pixel and ``la_sim_max`` keeps the scores in MFMA accumulators (csrc/similarity.hip).  Layout plumbing
(NCHW -> NHWC, reshapes, the query / support split) stays in torch; post-processing is ``la_bilinear`` + ``la_post_final``, the kernels
``LamEngine.postprocess_dev`` launches.

One deliberate deviation: a class without a support pixel comes out as -inf everywhere, where the reference resamples
a channel of -inf into a mix of -inf and NaN.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.nn as nn

from . import _lib as L


def _device_of(t: torch.Tensor) -> torch.device:
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


class SimilarityFewShotSegmenter(nn.Module):
    def __init__(self, encoder: Optional[Callable] = None, similarity: str = "cosine", image_size: Optional[int] = None,
                 custom_preprocess: bool = False, compare_size: Optional[int] = None):
        super().__init__()
        self.encoder = encoder             # any callable images -> (Bn, C, g, g); the model itself has no parameters
        self.similarity = similarity
        self.image_size = image_size
        self.custom_preprocess = custom_preprocess
        # similarity.py:24-26: the image_size default is overwritten at once, so None stays None (compare on the encoder's own grid)
        self.compare_size = compare_size
        if similarity != "cosine":
            raise NotImplementedError(f"Similarity '{similarity}' not implemented. Only cosine is supported.")

    # ---- similarity.py:105-120 ----
    def _embeddings(self, batch: dict) -> torch.Tensor:
        if "embeddings" in batch:
            return batch["embeddings"]                                   # [B, M, D, g, g], index 0 = query
        if self.encoder is None:
            raise ValueError("Encoder is None, but no embeddings provided in batch.")
        images = batch["images"]                                         # [B, M, 3, S, S]
        b, m = images.shape[:2]
        emb = self.encoder(images.reshape(b * m, *images.shape[2:]))     # [(B M), D, g, g]
        return emb.reshape(b, m, *emb.shape[1:])

    # ---- similarity.py:122-192: the logits on the compare grid ----
    def compare_logits(self, batch: dict) -> torch.Tensor:
        """[B, N, cs, cs] fp32 on the device; a class without a support pixel is -inf."""
        emb = self._embeddings(batch)
        dev = _device_of(emb)
        with torch.cuda.device(dev):
            emb = emb.detach().to(dev, torch.float32).contiguous()
            b, m, d, g, g2 = emb.shape
            if g != g2:
                raise ValueError(f"similarity: square embedding grids expected, got {g} x {g2}")
            cs = g if self.compare_size is None else int(self.compare_size)
            masks = batch["prompt_masks"].detach().to(dev, torch.float32).contiguous()         # [B, M1, N, Hm, Wm]
            _, m1, n, hm, wm = masks.shape
            if masks.shape[0] != b or m1 != m - 1:
                raise ValueError(f"similarity: prompt_masks {tuple(masks.shape)} do not go with embeddings {tuple(emb.shape)}")
            rows = torch.empty(b * m, g * g, d, device=dev, dtype=torch.float32)
            L.nchw_to_nhwc(emb, b * m, d, g * g, out32=rows, dt=L.LA_F32)
            e16 = torch.empty(b * m, cs * cs, d, device=dev, dtype=torch.float16)
            L.sim_prepare(rows, g, cs, e16)
            e16 = e16.view(b, m, cs * cs, d)
            q16 = e16[:, 0].contiguous()
            k16 = e16[:, 1:].reshape(b, m1 * cs * cs, d).contiguous()
            bits = torch.empty(b * m1, cs * cs, device=dev, dtype=torch.int32)
            L.sim_class_bits(masks.view(b * m1, n, hm, wm), cs, bits)
            out = torch.empty(b, n, cs * cs, device=dev, dtype=torch.float32)
            L.sim_max(q16, k16, bits.view(b, m1 * cs * cs), n, out)
            return out.view(b, n, cs, cs)

    def postprocess_masks(self, masks: torch.Tensor, original_sizes: torch.Tensor) -> torch.Tensor:
        """similarity.py:33-103 (the arithmetic of Lam.postprocess_masks): bilinear to image_size, crop to the preprocess shape if
        custom_preprocess, bilinear to the query's original size, -inf pad with the background pad 0.  A channel that is -inf (a class
        without a support pixel) stays -inf everywhere."""
        if self.image_size is None:
            raise ValueError("similarity: postprocess_masks needs image_size")
        dev = _device_of(masks)
        with torch.cuda.device(dev):
            masks = masks.detach().to(dev, torch.float32)
            b, n, h, w = masks.shape
            s = int(self.image_size)
            dl = original_sizes.detach().to("cpu").tolist()              # [B][M][2]
            hmax = max(int(hw[0]) for item in dl for hw in item)
            wmax = max(int(hw[1]) for item in dl for hw in item)
            sizes = []
            for item in dl:
                oh, ow = int(item[0][0]), int(item[0][1])
                if self.custom_preprocess:                               # get_preprocess_shape (data/utils.py)
                    sc = s * 1.0 / max(oh, ow)
                    ph, pw = int(oh * sc + 0.5), int(ow * sc + 0.5)
                else:
                    ph, pw = s, s
                sizes.append([oh, ow, ph, pw])
            has = torch.isfinite(masks).flatten(2).any(dim=2)            # [B, N]: the class has a support pixel
            seg = torch.where(has[:, :, None, None], masks, torch.zeros((), device=dev)).contiguous()
            big = torch.empty(b * n, s, s, device=dev, dtype=torch.float32)
            L.bilinear(seg, b * n, h, w, s, s, big)
            logits = torch.empty(b, n, hmax, wmax, device=dev, dtype=torch.float32)
            L.post_final(big, b, n, s, torch.tensor(sizes, dtype=torch.int32).to(dev), has.to(torch.uint8).contiguous(), hmax, wmax, logits, None)
            return logits

    def forward(self, batch: dict) -> dict:
        return {"logits": self.postprocess_masks(self.compare_logits(batch), batch["dims"])}


def build_similarity(encoder: Optional[Callable] = None, similarity: str = "cosine", image_size: Optional[int] = None,
                     custom_preprocess: bool = False, compare_size: Optional[int] = None) -> SimilarityFewShotSegmenter:
    return SimilarityFewShotSegmenter(encoder=encoder, similarity=similarity, image_size=image_size, custom_preprocess=custom_preprocess,
                                      compare_size=compare_size)
