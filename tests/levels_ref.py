"""Plain torch restatement of the two steps that ``classification_levels=2`` adds (mask_decoder.py:345-346,358-362), in any dtype, for
the CPU and GPU tests of tests/test_levels_*.py:

    coarse_classify   cls1[b, c] = tokens[b, c, :] @ image[b, :, pixels]     (``_classify`` on the transformer's outputs)
    enlarge4          the x4 bilinear enlargement, align_corners=False, with source indices clamped to the plane
    level_reduce      Conv2d(2, 1, 3x3, zero padding) over [fine, enlarge4(coarse)] per (b, c) plane
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def coarse_classify(tokens: torch.Tensor, image_rows: torch.Tensor) -> torch.Tensor:
    """tokens (B, C, D), image_rows (B, Npix, D) NHWC -> (B, C, Npix)."""
    return torch.einsum("bcd,bpd->bcp", tokens, image_rows)


def _axis(n: int, dtype, device):
    """(lo index, hi index, weight of hi) of the 4n fine positions along one axis."""
    y = torch.arange(4 * n, device=device)
    src = (y.to(torch.float64) + 0.5) / 4.0 - 0.5
    lo = torch.floor(src)
    lam = (src - lo).to(dtype)                      # 5/8, 7/8, 1/8, 3/8: exact in every float format
    lo = lo.to(torch.long)
    return lo.clamp(0, n - 1), (lo + 1).clamp(0, n - 1), lam


def enlarge4(x: torch.Tensor) -> torch.Tensor:
    """(..., h, w) -> (..., 4h, 4w)."""
    h, w = x.shape[-2:]
    ya, yb, ly = _axis(h, x.dtype, x.device)
    xa, xb, lx = _axis(w, x.dtype, x.device)
    rows = x[..., ya, :] * (1 - ly)[:, None] + x[..., yb, :] * ly[:, None]
    return rows[..., xa] * (1 - lx) + rows[..., xb] * lx


def level_reduce(cls0: torch.Tensor, cls1: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """cls0 (B, C, 4h, 4w), cls1 (B, C, h, w), weight (1, 2, 3, 3) or 18 values, bias (1,) -> (B, C, 4h, 4w)."""
    b, c, hh, ww = cls0.shape
    planes = torch.stack([cls0, enlarge4(cls1)], dim=2).reshape(b * c, 2, hh, ww)
    out = F.conv2d(planes, weight.reshape(1, 2, 3, 3).to(cls0.dtype), bias.reshape(1).to(cls0.dtype), padding=1)
    return out.reshape(b, c, hh, ww)
