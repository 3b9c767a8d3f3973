"""Plain torch restatement of the three steps that the per-example family changes (``embeddings_per_example`` /
``segment_example_logits``), for the CPU and GPU tests of tests/test_multi_embedding_*.py:

  pool_examples     prompt_encoder.py:726-729  adaptive_avg_pool2d to k x k and "(b m c) d h w -> b (m h w) c d"
  repeat_flags      prompt_encoder.py:731      "b m c -> b (m h w) c"
  classify_max      mask_decoder.py:309-313    per-example logits, -inf on the invalid examples, maximum over the examples

Works in whatever dtype its inputs have (the GPU tests evaluate it in float64).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F


def pool_side(embeddings_per_example) -> int:
    """int(sqrt(embeddings_per_example)) (prompt_encoder.py:727); 1 when the plain mean is taken."""
    e = embeddings_per_example
    return math.isqrt(int(e)) if e and int(e) > 1 else 1


def bins(g: int, k: int):
    """adaptive_avg_pool's bins along one axis: [(lo, hi)) with lo = floor(i g / k), hi = ceil((i + 1) g / k)."""
    return [((i * g) // k, -((-(i + 1) * g) // k)) for i in range(k)]


def pool_examples(src: torch.Tensor, b: int, m: int, c: int, g: int, k: int) -> torch.Tensor:
    """src [(b m c), g*g, D] NHWC rows (the prompt encoder's stream) -> [b, m*k*k, c, D], example index m*k*k + i*k + j."""
    d = src.shape[-1]
    x = src.reshape(b * m * c, g, g, d).permute(0, 3, 1, 2)                      # (b m c) d h w
    p = F.adaptive_avg_pool2d(x, (k, k))                                           # (b m c) d k k
    return p.reshape(b, m, c, d, k * k).permute(0, 1, 4, 2, 3).reshape(b, m * k * k, c, d)


def repeat_flags(flag_examples: torch.Tensor, k: int) -> torch.Tensor:
    """[b, m, c] -> [b, m*k*k, c]: every bin of a support carries the support's flag."""
    return flag_examples.repeat_interleave(k * k, dim=1)


def per_example_logits(protos: torch.Tensor, feat: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """protos [b, n, c, f], feat [b, npix, f], flags [b, n, c] -> [b, n, c, npix] with -inf on the invalid examples."""
    per = torch.einsum("bncf,bpf->bncp", protos, feat)
    return per.masked_fill((flags == 0).unsqueeze(-1), float("-inf"))


def classify_max(protos: torch.Tensor, feat: torch.Tensor, flags: torch.Tensor):
    """-> (seg [b, c, npix], win [b, c, npix]): maximum over the valid examples and the lowest n that attains it (-1: none valid)."""
    per = per_example_logits(protos, feat, flags)
    seg = per.max(dim=1).values
    n = per.shape[1]
    idx = torch.arange(n).view(1, n, 1, 1).expand_as(per)
    win = torch.where(per == seg.unsqueeze(1), idx, torch.full_like(idx, n)).min(dim=1).values
    win = torch.where(torch.isfinite(seg), win, torch.full_like(win, -1))
    return seg, win
