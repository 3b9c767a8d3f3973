#!/usr/bin/env python
"""Golden vectors of the cosine-similarity segmenter from the reference's ``SimilarityFewShotSegmenter`` (build container only;
tools/golden_lib.py makes the reference importable):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_similarity.py [--only NAME] [--no-write]

For every case of tests/cases_similarity.py the seeded batch runs through the reference on CPU / fp32.
tests/golden/similarity_<case>.safetensors holds the inputs (embeddings, prompt_masks, dims), ``compare_logits`` - the logits on the compare
grid, captured in front of ``postprocess_masks`` -, the final ``logits`` and their ``argmax``; the json the constructor's keywords and the share
of the reference's pixels whose top-two gap lies inside the margin band, which must be at most MAX_BAND_SHARE (otherwise change the case's
seed).  The cases give every class a support pixel, so the reference's logits are finite inside the query's frame.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

import torch                            # noqa: E402
import tests.cases_similarity as C      # noqa: E402


def forward(name, case):
    from label_anything.models.similarity import SimilarityFewShotSegmenter
    model = SimilarityFewShotSegmenter(**case["model"]).eval()
    batch = C.make_inputs(case)
    seen = []
    post = model.postprocess_masks
    model.postprocess_masks = lambda masks, sizes: (seen.append(masks.detach().clone()), post(masks, sizes))[1]
    with torch.no_grad():
        logits = model({k: v.clone() for k, v in batch.items()})["logits"]
    low = seen[0]
    assert bool(torch.isfinite(low).all()), f"{name}: a class has no support pixel"
    assert not bool(torch.isnan(logits).any())
    share = GL.band_share(logits, C.MARGIN)
    assert share <= C.MAX_BAND_SHARE, f"{name}: {share:.3%} of the reference's pixels lie inside the margin band; change the seed"
    meta = {"case": name, "model": case["model"], "seed": case["seed"], "margin": C.MARGIN, "margin_band_share": share,
            "scale": float(low.abs().max())}
    tensors = {**{k: v.contiguous() for k, v in batch.items()}, "compare_logits": low.contiguous(), "logits": logits.contiguous(),
               "argmax": logits.argmax(dim=1).to(torch.uint8).contiguous()}
    size = GL.write_fixture(f"similarity_{name}", tensors, meta)
    print(f"[{name}] compare grid {tuple(low.shape)} logits {tuple(logits.shape)} band share {share:.4f} bytes {size}")


if __name__ == "__main__":
    GL.main(C.CASES, forward)
