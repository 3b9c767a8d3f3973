"""Cosine-similarity segmenter parity cases: seeded episodes of embeddings, box prompt masks and original sizes.

Shared by tools/make_golden_similarity.py (the reference's SimilarityFewShotSegmenter -> tests/golden/similarity_*), tests/test_similarity_cpu.py
and tests/test_similarity_model_gpu.py.  The fixtures hold the inputs, so the tests read what the reference read.

The cases stay at three classes or fewer: a support pixel inside two boxes is a key of two classes, its two logits tie exactly wherever it
wins both, and with five overlapping classes 9 - 14 % of the reference's pixels lie inside the margin band.  More classes are covered at the
kernel level (tests/test_similarity_kernels_gpu.py), where logits are compared and not the argmax.
"""
from __future__ import annotations

import torch

MARGIN = 2e-3               # argmax must agree wherever the reference's top-2 margin exceeds this share of its largest logit
MAX_BAND_SHARE = 0.05       # the generator refuses a case with more of the reference's pixels inside the band

# model: the constructor's keywords.  b, m (query + supports), d, g: the embeddings [b, m, d, g, g] ~ N(0, 1).  n classes, masks hm x hm.
# dims: the original (h, w) of every image, [b][m]; the query's is what post-processing resamples to.
CASES = {
    # bicubic 6 -> 16, two supports, three classes, non-square originals cropped by custom_preprocess, masks 37 -> 16 (no integer ratio)
    "b2_cs16": dict(model=dict(image_size=64, compare_size=16, custom_preprocess=True), b=2, m=3, d=64, g=6, n=3, hm=37, seed=401,
                    dims=[[[50, 70], [64, 64], [64, 48]], [[72, 44], [40, 64], [64, 64]]]),
    # compare_size=None: the encoder's own grid, no resample
    "b2_native": dict(model=dict(image_size=48, compare_size=None, custom_preprocess=False), b=2, m=3, d=64, g=6, n=3, hm=37, seed=402,
                      dims=[[[40, 60], [48, 48], [48, 48]], [[60, 40], [48, 48], [48, 48]]]),
    # ViT-B width, one support, 8 -> 24
    "d768_cs24": dict(model=dict(image_size=96, compare_size=24, custom_preprocess=False), b=1, m=2, d=768, g=8, n=2, hm=32, seed=403,
                      dims=[[[80, 100], [96, 96]]]),
}


def make_inputs(case: dict) -> dict:
    """The seeded batch of a case: embeddings, prompt_masks (class 0 is noise: the model replaces it; every other class one box per
    support, value 1), dims."""
    gen = torch.Generator().manual_seed(case["seed"])
    b, m, d, g, n, hm = (case[k] for k in ("b", "m", "d", "g", "n", "hm"))
    emb = torch.randn(b, m, d, g, g, generator=gen)
    masks = torch.zeros(b, m - 1, n, hm, hm)
    masks[:, :, 0] = (torch.rand(b, m - 1, hm, hm, generator=gen) < 0.5).float()
    for i in range(b):
        for j in range(m - 1):
            for c in range(1, n):
                y0, x0 = (int(v) for v in torch.randint(0, hm // 2, (2,), generator=gen))
                h, w = (int(v) for v in torch.randint(hm // 4, hm // 2, (2,), generator=gen))
                masks[i, j, c, y0:y0 + h, x0:x0 + w] = 1.0
    return {"embeddings": emb, "prompt_masks": masks, "dims": torch.tensor(case["dims"], dtype=torch.int64)}
