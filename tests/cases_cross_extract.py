"""Parity cases of ``embedding_extraction="cross_attention"`` (EmbeddingTransformer, prompt_encoder.py:280-313).

``x4`` and ``x1`` run the ``novit_d256_2w3s`` episode and geometry of tests/cases.py (decoder only, D = 256, 16 x 16 grid, 2-way 3-shot +
background, one missing mask, masks + points, class encoder on), like tests/cases_multi_embedding.py, so that only the extraction differs;
``x5_d64`` runs the D = 64 decoder-only geometry and episode of ``TRAIN_CASE``.  tools/make_golden_cross_extract.py turns them into
tests/golden/cross_extract_<name>{,_stream}.{safetensors,json}; tests/test_cross_extract_*.py read them.
"""
from __future__ import annotations

import dataclasses

from labelanything_amd.config import resolve_examples
from tests.cases import CASES, TRAIN_CASE

_BASE = CASES["novit_d256_2w3s"]


def _case(base, embeddings_per_example, segment_example_logits, stream_stride, weight_seed=None, min_spread=1.5):
    seg, epe = resolve_examples(segment_example_logits, embeddings_per_example)
    cfg = dataclasses.replace(base["cfg"], segment_example_logits=seg, embeddings_per_example=epe, embedding_extraction="cross_attention",
                              class_attention=False, example_attention=False, example_class_attention=False)
    return dict(cfg=cfg, weight_seed=base["weight_seed"] if weight_seed is None else weight_seed, episode=dict(base["episode"]),
                stream_stride=stream_stride, min_spread=min_spread)


# stream_stride: the fixture keeps every stream_stride-th row and column of the stream handed to the extraction (and the reference
# module's output on exactly those rows), which keeps the D = 256 files below 400 KB
#
# min_spread: the generator's fixture condition - in both layers every attention row's score spread (max - min along the keys) is at
# least min_spread and the largest at least 5, so that a wrong softmax cannot hide behind near-uniform weights.  1.5 for the D = 256
# cases.  The D = 64 decoder has heads of width 4: the score scale of a row is the norm of a 4-vector q_h, which is small for some of the
# 2 x 240 rows under every seed tried (10 weight seeds on this episode, 80 on a 16 x 16 grid with six supports: the best smallest spread
# was 1.47; this fixture has 0.95 .. 8.20 in layer 0 and 0.73 .. 8.21 in layer 1), so that case asks for 0.5.
XE_CASES = {
    # the model section of parameters/validation/Pascal/mae_cross.yaml: 4 learned queries, no merge attention; R = 32 folded queries
    "x4": _case(_BASE, 4, False, 4),
    # segment_example_logits alone: one learned query, R = 8 (half an MFMA tile)
    # (weight seed 32: with the geometry's seed 13 the largest spread of layer 1 is 4.88, below the fixture condition)
    "x1": _case(_BASE, None, True, 4, weight_seed=32),
    # five queries - not a square, R = 40 is no multiple of the tile - on the D = 64 decoder (head width 4) behind the 96 -> 64 neck
    "x5_d64": _case(TRAIN_CASE, 5, False, 1, min_spread=0.5),
}
