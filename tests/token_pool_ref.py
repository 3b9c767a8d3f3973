"""Torch restatement of the TokenPool prompt encoder (``prompt_encoder="TokenPool"``), composed from the oracle's primitives
(oracle/lam_oracle.py) and written from the definition, in any dtype (the dtype of the weights and the episode):

1. sparse tokens and per-pair dense maps as in the plain prompt encoder: ``sparse_embedding_attention`` over the C Ns tokens of a support,
   ``not_a_mask_embed`` where flag_masks == 0, the bilinear resize to the grid (``no_mask_embed`` everywhere without mask prompts);
2. class rows: ``pos_embedding[rows[c]]`` on every token of class c and on every pixel of class c's dense map; then
   src[s, pix, :] = support[s, pix, :] + sum_c (dense[s, c, pix, :] + class_enc[c, :]), one slab per support image s = (b, m);
3. TwoWayTransformer(src, dense_pe, tokens[s] = the C Ns tokens in (c, n) order) over the B M supports; BOTH outputs are used;
4. emb[b, m, c, :] = mean over n of tokens_out[(b m), (c n), :];
5. the three optional merge attentions and the flag-masked mean over M, as in the plain encoder;
6. class_examples_src = the image-side output in rows, (B M, hw, D).
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from oracle import lam_oracle as O


def dense_sum(w, geo, masks, b: int, m: int, c: int, g: int, class_enc: Optional[Tensor]) -> Tensor:
    """sum_c (dense[s, c] + class_enc[c]) -> (B M, D, g, g)."""
    pre, d, p = "prompt_encoder", geo.embed_dim, b * m * c
    if masks is not None:
        mk, mf = masks
        dense = O.mask_downscale(w, mk.reshape(p, 1, mk.shape[-2], mk.shape[-1]))
        missing = (mf.reshape(p) == 0).view(p, 1, 1, 1)
        dense = torch.where(missing, w[pre + ".not_a_mask_embed.weight"].view(1, d, 1, 1).expand_as(dense), dense)
        if dense.shape[-1] != g:
            dense = F.interpolate(dense, size=(g, g), mode="bilinear", align_corners=False)
    else:
        dense = w[pre + ".no_mask_embed.weight"].view(1, d, 1, 1).expand(p, d, g, g)
    dense = dense.reshape(b * m, c, d, g, g)
    if class_enc is not None:
        dense = dense + class_enc.view(1, c, d, 1, 1)
    return dense.sum(dim=1)


def prompt_encoder(w, geo, support_emb: Tensor, points, boxes, masks, flag_examples: Tensor,
                   selected_rows: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """support_emb (B, M, D, g, g) -> class_embeddings (B, C, D), class_examples_embeddings (B, M, C, D), class_examples_src (B M, hw, D)."""
    pre, d, heads = "prompt_encoder", geo.embed_dim, geo.dec_heads
    first = points[0] if points is not None else boxes[0] if boxes is not None else masks[0]
    b, m, c = first.shape[:3]
    g = support_emb.shape[-1]
    sparse = O.embed_sparse(w, geo, b, m, c, points, boxes)                               # (B M, C Ns, D), (c, n) order
    sparse = O.attention_mlp_block(w, pre + ".sparse_embedding_attention", sparse, heads)
    ns = sparse.shape[1] // c
    ce = None
    if geo.class_encoder_bank:
        assert selected_rows is not None, "RandomMatrixEncoder is stochastic; pass selected_rows"
        ce = w[pre + ".class_encoder.pos_embedding"][0, 0, selected_rows]                # (C, D)
        sparse = (sparse.view(b * m, c, ns, d) + ce.view(1, c, 1, d)).reshape(b * m, c * ns, d)
    src = support_emb.reshape(b * m, d, g, g) + dense_sum(w, geo, masks, b, m, c, g, ce)
    toks, keys = O.two_way_transformer(w, pre + ".transformer", src, O.dense_pe(w, g).to(src.dtype), sparse, heads)
    emb = toks.view(b, m, c, ns, d).mean(dim=3)
    if geo.class_attention:
        emb = O.attention_mlp_block(w, pre + ".class_attention", emb.reshape(b * m, c, d), heads).view(b, m, c, d)
    if geo.example_attention:
        e2 = emb.permute(0, 2, 1, 3).reshape(b * c, m, d)
        emb = O.attention_mlp_block(w, pre + ".example_attention", e2, heads).view(b, c, m, d).permute(0, 2, 1, 3)
    if geo.example_class_attention:
        emb = O.attention_mlp_block(w, pre + ".class_example_attention", emb.reshape(b, m * c, d), heads).view(b, m, c, d)
    fe = flag_examples.to(emb.dtype).unsqueeze(-1)
    denom = fe.sum(dim=1)
    denom = torch.where(denom == 0, torch.ones_like(denom), denom)
    return {"flag_examples": flag_examples, "class_embeddings": (emb * fe).sum(dim=1) / denom, "class_examples_embeddings": emb,
            "class_examples_src": keys}


def lam_forward(w, geo, batch, selected_rows: Optional[Tensor] = None) -> Dict[str, Tensor]:
    emb = O.episode_embeddings(w, geo, batch)
    pts, bxs, msk = O.select_prompts(batch)
    pe = prompt_encoder(w, geo, emb[:, 1:], pts, bxs, msk, batch["flag_examples"], selected_rows)
    low = O.mask_decoder(w, geo, emb[:, 0], pe["class_embeddings"])
    return {"logits": O.postprocess(geo, low, batch["dims"], batch.get("flag_gts")), "low_res_logits": low, **pe}


def to_dtype(tree, dtype):
    """Floating tensors of a weight dict / an episode in ``dtype`` (labels, flags and sizes keep theirs)."""
    return {k: (v.to(dtype) if isinstance(v, Tensor) and v.is_floating_point() else v) for k, v in tree.items()}
