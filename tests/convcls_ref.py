"""Plain torch restatement of the two steps that ``conv_classification`` adds (mask_decoder.py:257-271,299-307), in any dtype, for the CPU
and GPU tests of tests/test_convcls_*.py.  Written from the formulas, with nothing but einsum, pad and slices:

    compose_kernels   k1[n, m, i, j] = sum_in e[n, in] W1[in, m, i, j];  K[n, o, y, x] = sum_m sum_ij k1[n, m, y-i, x-j] W2[m, o, i, j]
    correlate5        seg[b, c, y, x] = sum_d sum_uv feat[b, d, y+u-2, x+v-2] K[b, c, d, u, v], taps outside the map absent
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def first_step(protos: torch.Tensor, w1: torch.Tensor) -> torch.Tensor:
    """protos (N, cf), w1 (cf in, cf out, 3, 3) -> k1 (N, cf, 3, 3)."""
    return torch.einsum("ni,imab->nmab", protos, w1)


def compose_kernels(protos: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """protos (N, cf), w1, w2 (cf in, cf out, 3, 3) -> K (N, cf, 5, 5): channel o of the 5 x 5 kernel of prototype n."""
    k1 = first_step(protos, w1)
    out = None
    for a in range(3):
        for b in range(3):
            term = torch.einsum("nm,moij->noij", k1[:, :, a, b], w2)          # lands at rows a .. a+2, columns b .. b+2
            term = F.pad(term, (b, 2 - b, a, 2 - a))
            out = term if out is None else out + term
    return out


def tap_major(k: torch.Tensor) -> torch.Tensor:
    """(N, cf, 5, 5) -> (N, 25, cf): the layout of la_proto_kernels' output."""
    return k.permute(0, 2, 3, 1).reshape(k.shape[0], 25, k.shape[1])


def from_tap_major(k: torch.Tensor) -> torch.Tensor:
    """(..., 25, cf) -> (..., cf, 5, 5)."""
    return k.reshape(*k.shape[:-2], 5, 5, k.shape[-1]).movedim(-1, -3)


def correlate5(feat: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """feat (B, cf, H, W), k (B, C, cf, 5, 5) -> (B, C, H, W); the kernels of episode b meet episode b only."""
    h, w = feat.shape[-2:]
    pad = F.pad(feat, (2, 2, 2, 2))
    out = None
    for u in range(5):
        for v in range(5):
            term = torch.einsum("bdyx,bcd->bcyx", pad[:, :, u:u + h, v:v + w], k[:, :, :, u, v])
            out = term if out is None else out + term
    return out


def conv_classify(feat: torch.Tensor, protos: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> torch.Tensor:
    """feat (B, cf, H, W), protos (B, C, cf) -> low-resolution logits (B, C, H, W)."""
    b, c, cf = protos.shape
    return correlate5(feat, compose_kernels(protos.reshape(b * c, cf), w1, w2).reshape(b, c, cf, 5, 5))
