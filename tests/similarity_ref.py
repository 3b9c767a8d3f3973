"""fp64 restatement of the reference's SimilarityFewShotSegmenter.forward up to the compare-grid logits (models/similarity.py:122-192),
step by step, with the class membership as one word per support pixel - what the kernels of csrc/similarity.hip are tested against.
tests/test_similarity_cpu.py pins it to the reference's own output (tests/golden/similarity_*)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def nearest_index(in_size: int, out_size: int) -> torch.Tensor:
    """Source index of every destination index under F.interpolate(mode="nearest", size=out_size): min(floor(dst * scale), in - 1) with
    scale = in / out and the product both rounded to fp32 (ATen nearest_idx)."""
    scale = np.float32(in_size) / np.float32(out_size)
    src = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(src, in_size - 1))


def class_bits(masks: torch.Tensor, cs: int) -> torch.Tensor:
    """masks [P, N, Hm, Wm] -> int64 [P, cs * cs]: bit n (n >= 1) = class n is non-zero at the nearest source pixel, bit 0 = no such bit."""
    p, n, hm, wm = masks.shape
    small = masks[:, :, nearest_index(hm, cs)][:, :, :, nearest_index(wm, cs)].reshape(p, n, cs * cs)
    word = torch.zeros(p, cs * cs, dtype=torch.int64)
    for c in range(1, n):
        word |= (small[:, c] != 0).long() << c
    return torch.where(word == 0, torch.ones_like(word), word)


def prepare(emb: torch.Tensor, cs) -> torch.Tensor:
    """emb [n, D, g, g] -> fp64 rows [n, cs * cs, D]: bicubic to cs x cs (cs None: as it is), L2-normalised over D."""
    x = emb.double()
    if cs is not None:
        x = F.interpolate(x, size=(cs, cs), mode="bicubic", align_corners=False)
    x = F.normalize(x, dim=1)
    return x.flatten(2).transpose(1, 2).contiguous()


def masked_max(q: torch.Tensor, k: torch.Tensor, bits: torch.Tensor, n: int) -> torch.Tensor:
    """q [B, Q, D], k [B, K, D] (any float type, taken to fp64), bits integer [B, K] -> fp64 [B, n, Q], -inf for a class without a key."""
    sim = torch.einsum("bqd,bkd->bqk", q.double(), k.double())
    out = []
    for c in range(n):
        member = ((bits.long() >> c) & 1).bool()[:, None, :]
        out.append(sim.masked_fill(~member, float("-inf")).max(dim=2).values)
    return torch.stack(out, dim=1)


def compare_logits(embeddings: torch.Tensor, prompt_masks: torch.Tensor, compare_size) -> torch.Tensor:
    """embeddings [B, M, D, g, g] (index 0 = query), prompt_masks [B, M1, N, Hm, Wm] -> fp64 [B, N, cs, cs]."""
    b, m, d, g, _ = embeddings.shape
    cs = g if compare_size is None else compare_size
    rows = prepare(embeddings.flatten(0, 1), compare_size).view(b, m, cs * cs, d)
    _, m1, n, hm, wm = prompt_masks.shape
    bits = class_bits(prompt_masks.reshape(b * m1, n, hm, wm), cs).view(b, m1 * cs * cs)
    return masked_max(rows[:, 0], rows[:, 1:].reshape(b, m1 * cs * cs, d), bits, n).view(b, n, cs, cs)
