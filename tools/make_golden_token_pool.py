#!/usr/bin/env python
"""Golden vectors of the TokenPool prompt encoder from the REFERENCE (build container only; tools/golden_lib.py imports it):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_token_pool.py [--only NAME] [--no-train]

For every case of tests/cases_token_pool.py the seeded weights (``init_state_dict``: TokenPool adds no tensor) are strict-loaded into
``_build_lam(..., prompt_encoder="TokenPool")`` and the seeded episode runs through the reference's ``Lam.forward`` on CPU / fp32, the
class-encoder rows pinned by a seeded draw (tools/golden_lib.py:fixed_rows).  tests/golden/token_pool_<case>.safetensors holds the
reference's OUTPUTS: class_embeddings, class_examples_embeddings, low_res_logits, logits, argmax and every ``SRC_STRIDE``-th pixel row,
pixel column and channel of class_examples_src (the image side of the two-way transformer, one slab per support image).  For the case
of ``TP_TRAIN`` one training step (focal objective, class weighting) is stored as token_pool_<case>_train.{safetensors,json}: loss,
per-tensor gradient norms, the full gradients of ``TP_TRAIN_FULL``, the reference's own fp32-vs-fp64 gradient error and the tensors that
received no gradient.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

import torch                            # noqa: E402
from tests.cases_token_pool import SRC_STRIDE, TP_CASES, TP_TRAIN, TP_TRAIN_FULL   # noqa: E402

FINAL = ("prompt_encoder.transformer.final_attn_token_to_image.", "prompt_encoder.transformer.norm_final_attn.")


def run_forward(name, case):
    lam, sd, batch, rows = GL.reference_episode(case, prompt_encoder="TokenPool")
    plain, _ = GL.build_reference(case, prompt_encoder=None)
    assert list(lam.state_dict()) == list(plain.state_dict()) and sorted(lam.state_dict()) == sorted(sd), "TokenPool must not add or rename a tensor"
    cfg = case["cfg"]
    b, m, c = batch["flag_examples"].shape
    with torch.no_grad():
        seg_low, pe_result = lam._forward(batch)
        ref = lam(batch)
    cee, cls, src = pe_result["class_examples_embeddings"], pe_result["class_embeddings"], pe_result["class_examples_src"]
    g = cfg.grid
    assert tuple(cee.shape) == (b, m, c, cfg.embed_dim) and tuple(cls.shape) == (b, c, cfg.embed_dim)
    assert tuple(src.shape) == (b * m, g * g, cfg.embed_dim), src.shape                     # one slab per support image, in rows
    assert torch.equal(ref["class_examples_embeddings"], cee)
    assert bool(torch.isfinite(seg_low).all())
    st = SRC_STRIDE
    tensors = {
        "class_embeddings": cls.contiguous(),
        "class_examples_embeddings": cee.contiguous(),
        **GL.logit_tensors(seg_low, ref),
        # rows, as the reference returns them and the engine holds the stream: (B M, h' w', D')
        "class_examples_src_sample": src.view(b * m, g, g, -1)[:, ::st, ::st, ::st].flatten(1, 2).contiguous(),
    }
    fin = torch.isfinite(ref["logits"])
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "supports": b * m, "classes": c,
            "src_stride": st, "full_src_shape": list(src.shape), "state_dict_keys_equal_plain": True,
            "embedding_scale": float(cee.abs().max()), "low_res_scale": float(seg_low.abs().max()),
            "finite_logit_fraction": float(fin.double().mean())}
    size = GL.write_fixture(f"token_pool_{name}", tensors, meta, rows)
    print(f"[{name}] supports {b * m} classes {c} bytes {size} scale {meta['embedding_scale']:.3f}")


def train():
    name = TP_TRAIN["case"]
    step = GL.run_train(TP_CASES[name], TP_TRAIN["seed_gt"], prompt_encoder="TokenPool")
    assert not any(k.startswith(FINAL) for k in step.dead), "final_attn / norm_final_attn are live under TokenPool"
    assert all(float(step.g32[k].abs().max()) > 0 for k in step.keys if k.startswith(FINAL))
    GL.write_train(f"token_pool_{name}", step, TP_TRAIN_FULL, "e_ref32", rows=step.rows)


if __name__ == "__main__":
    GL.main(TP_CASES, run_forward, [(TP_TRAIN["case"], train)])
