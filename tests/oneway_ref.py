"""Torch restatement of the one-way mask decoder (``fusion_transformer="OneWayTransformer"``), composed from the oracle's primitives
(oracle/lam_oracle.py) and written from the definition, in any dtype (the dtype of the weights and the episode):

1. the class tokens pass through the transformer untouched; they are the keys and values of both layers, WITHOUT a positional encoding
   and without a key mask;
2. per layer, on the image stream (B, hw, D):   img = norm1(img + attn(q = img + pe, k = v = tokens));
                                                img = norm2(img + lin2(relu(lin1(img))));      norm3 is a parameter that is never applied;
3. class_mlp on the class embeddings themselves, the upscaler and the spatial convolutions on the image output, as in the plain decoder.
The prompt encoder is the plain one (its two-way transformer is hard-wired in the reference's builder).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from oracle import lam_oracle as O


def one_way_transformer(w, pre: str, image: Tensor, image_pe: Tensor, tokens: Tensor, heads: int, depth: int = 2) -> Tuple[Tensor, Tensor]:
    """image (B, D, h, w); image_pe (B or 1, D, h, w); tokens (B, Nt, D) -> (tokens, image as (B, hw, D))."""
    img = image.flatten(2).transpose(1, 2)
    pe = image_pe.flatten(2).transpose(1, 2)
    for l in range(depth):
        lp = f"{pre}.layers.{l}"
        img = O.layer_norm(w, lp + ".norm1", img + O.dec_attention(w, lp + ".cross_attn_image_to_token", img + pe, tokens, tokens, heads), 1e-5)
        m = O.linear(w, lp + ".mlp.lin2", torch.relu(O.linear(w, lp + ".mlp.lin1", img)))
        img = O.layer_norm(w, lp + ".norm2", img + m, 1e-5)
    return tokens, img


def mask_decoder(w, geo, query_emb: Tensor, class_emb: Tensor) -> Dict[str, Tensor]:
    """query_emb (B, D, g, g), class_emb (B, C, D) -> low_res_logits (B, C, 4g, 4g) and the transformer's image output (B, hw, D)."""
    pre = "mask_decoder"
    b, d, g, _ = query_emb.shape
    toks, img = one_way_transformer(w, pre + ".transformer", query_emb, O.dense_pe(w, g).to(query_emb.dtype), class_emb, geo.dec_heads)
    feat = img.transpose(1, 2).reshape(b, d, g, g)
    pr = torch.relu(O.linear(w, pre + ".class_mlp.layers.0", toks))
    pr = torch.relu(O.linear(w, pre + ".class_mlp.layers.1", pr))
    pr = O.linear(w, pre + ".class_mlp.layers.2", pr)
    up = F.conv_transpose2d(feat, w[pre + ".output_upscaling.0.weight"], w[pre + ".output_upscaling.0.bias"], stride=2)
    up = O.gelu(O.layer_norm_2d(w, pre + ".output_upscaling.1", up))
    up = F.conv_transpose2d(up, w[pre + ".output_upscaling.3.weight"], w[pre + ".output_upscaling.3.bias"], stride=2)
    for i in range(geo.spatial_convs or 0):
        up = F.conv2d(up, w[f"{pre}.spatial_convs.{3 * i}.weight"], w[f"{pre}.spatial_convs.{3 * i}.bias"], padding=1)
        if i < geo.spatial_convs - 1:
            up = O.gelu(O.layer_norm_2d(w, f"{pre}.spatial_convs.{3 * i + 1}", up))
    bb, ch, hh, ww = up.shape
    return {"low_res_logits": (pr @ up.view(bb, ch, hh * ww)).view(bb, -1, hh, ww), "transformer_image": img}


def lam_forward(w, geo, batch, selected_rows: Optional[Tensor] = None) -> Dict[str, Tensor]:
    emb = O.episode_embeddings(w, geo, batch)
    pts, bxs, msk = O.select_prompts(batch)
    pe = O.prompt_encoder(w, geo, emb[:, 1:], pts, bxs, msk, batch["flag_examples"], selected_rows)
    md = mask_decoder(w, geo, emb[:, 0], pe["class_embeddings"])
    return {"logits": O.postprocess(geo, md["low_res_logits"], batch["dims"], batch.get("flag_gts")), **md, **pe}


def to_dtype(tree, dtype):
    """Floating tensors of a weight dict / an episode in ``dtype`` (labels, flags and sizes keep theirs)."""
    return {k: (v.to(dtype) if isinstance(v, Tensor) and v.is_floating_point() else v) for k, v in tree.items()}
