"""Torch restatement of ``embedding_extraction="cross_attention"`` written from the formulas (not from the reference's program text):
two blocks of  E <- norm1(E + attn(E, X));  E <- norm2(E + lin2(relu(lin1(E)))),  with the learned queries as the first E and the
M hw stream rows X of every (episode, class) pair as keys and values.  Eight heads of width D / 16, query positional encoding zero,
norm3 unused, no key masked.

``literal``: project keys and values, softmax(q k^T / sqrt(hd)), weighted sum, out_proj.
``folded``:  qt_h = W_k,h^T q_h / sqrt(hd); p = softmax_l(qt_h . x_l); pooled = sum_l p_l x_l; head = W_v,h pooled + b_v,h.  The key bias is
constant along l and cancels in the softmax.
Both work in the dtype of ``stream`` (weights are cast to it).
"""
import math

import torch
import torch.nn.functional as F

HEADS = 8
PRE = "prompt_encoder.embedding_extraction"


def pair_rows(stream, b, m, c):
    """stream (B M C, hw, D), slabs in (b, m, c) order -> (B C, M hw, D): the rows of pair (b, c) in (m, pixel) order."""
    p, hw, d = stream.shape
    assert p == b * m * c
    return stream.view(b, m, c, hw, d).permute(0, 2, 1, 3, 4).reshape(b * c, m * hw, d)


def folded_queries(e, wq, bq, wk):
    """E (Z, n, D) -> folded queries (Z, 8 n, D), row h n + j."""
    z, n, d = e.shape
    hd = d // 2 // HEADS
    q = (e @ wq.t() + bq).view(z, n, HEADS, hd)
    return torch.einsum("znhe,hef->zhnf", q, wk.view(HEADS, hd, d)).reshape(z, HEADS * n, d) / math.sqrt(hd)


def pool(qt, x):
    """out[z, j] = sum_l softmax_l(qt[z, j] . x[z, l]) x[z, l]"""
    return torch.softmax(qt @ x.transpose(1, 2), dim=-1) @ x


def attention(e, x, w, pre, form, spreads=None, key_flags=None):
    """key_flags (Z, L) bool or None: the reference's key mask.  It is accepted and has NO effect - see the module's docstring and
    common.py:120-124, where a key mask alone yields an all-False score mask."""
    dt = x.dtype
    g = lambda k: w[f"{pre}.{k}"].to(dt)
    z, n, d = e.shape
    hd = d // 2 // HEADS
    if form == "folded":
        qt = folded_queries(e, g("q_proj.weight"), g("q_proj.bias"), g("k_proj.weight"))
        if spreads is not None:
            s = qt @ x.transpose(1, 2)
            spreads.append(s.max(-1).values - s.min(-1).values)
        pooled = pool(qt, x).view(z, HEADS, n, d)
        heads = torch.einsum("zhnf,hef->znhe", pooled, g("v_proj.weight").view(HEADS, hd, d)) + g("v_proj.bias").view(HEADS, hd)
        o = heads.reshape(z, n, d // 2)
    else:
        q = (e @ g("q_proj.weight").t() + g("q_proj.bias")).view(z, n, HEADS, hd).transpose(1, 2)
        k = (x @ g("k_proj.weight").t() + g("k_proj.bias")).view(z, -1, HEADS, hd).transpose(1, 2)
        v = (x @ g("v_proj.weight").t() + g("v_proj.bias")).view(z, -1, HEADS, hd).transpose(1, 2)
        s = q @ k.transpose(2, 3) / math.sqrt(hd)
        if key_flags is not None:
            s = s.masked_fill(torch.zeros_like(key_flags)[:, None, None, :], float("-inf"))       # the all-False score mask
        if spreads is not None:
            spreads.append((s.max(-1).values - s.min(-1).values).reshape(z, HEADS * n))
        o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(z, n, d // 2)
    return o @ g("out_proj.weight").t() + g("out_proj.bias")


def extract(stream, b, m, c, w, form="folded", spreads=None, flag_examples=None):
    """stream (B M C, hw, D) -> class_examples_embeddings (B, n, C, D).  flag_examples (B, M, C): only handed on as the key mask."""
    dt = stream.dtype
    x = pair_rows(stream, b, m, c)
    d = x.shape[-1]
    emb = w[f"{PRE}.embeddings.weight"].to(dt)
    n = emb.shape[0]
    e = emb.expand(b * c, n, d)
    kf = None
    if flag_examples is not None:
        hw = stream.shape[1]
        kf = flag_examples.bool().permute(0, 2, 1).reshape(b * c, m, 1).expand(b * c, m, hw).reshape(b * c, m * hw)
    for l in range(2):
        lp = f"{PRE}.layers.{l}"
        g = lambda k: w[f"{lp}.{k}"].to(dt)
        e = F.layer_norm(e + attention(e, x, w, lp + ".cross_attn_image_to_token", form, spreads, kf), (d,), g("norm1.weight"), g("norm1.bias"))
        h = F.relu(e @ g("mlp.lin1.weight").t() + g("mlp.lin1.bias")) @ g("mlp.lin2.weight").t() + g("mlp.lin2.bias")
        e = F.layer_norm(e + h, (d,), g("norm2.weight"), g("norm2.bias"))
    return e.view(b, c, n, d).permute(0, 2, 1, 3).contiguous()


def example_flags(flag_examples, n):
    """(B, M, C) -> (B, n, C): a class is valid when any support shows it."""
    return (flag_examples != 0).any(dim=1, keepdim=True).expand(-1, n, -1).to(torch.uint8).contiguous()
