#!/usr/bin/env python
"""Golden vectors of the one-way mask decoder from the REFERENCE (build container only; tools/golden_lib.py imports it):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_oneway.py [--only NAME] [--no-train]

For every case of tests/cases_oneway.py the seeded weights (``init_state_dict``) are strict-loaded into
``_build_lam(..., fusion_transformer="OneWayTransformer")`` and the seeded episode runs through the reference's ``Lam.forward`` on CPU /
fp32, the class-encoder rows pinned by a seeded draw (tools/golden_lib.py:fixed_rows).  tests/golden/oneway_<case>.json holds the
reference's state-dict keys and shapes IN ITS ORDER; the .safetensors its OUTPUTS: class_embeddings, every ``SRC_STRIDE``-th pixel row,
pixel column and channel of the mask-decoder transformer's image output (a forward hook), low_res_logits, logits and argmax.  The json
also records the share of pixels whose top-two logit gap lies inside the 2e-3 margin band on the reference's own logits; it must be at
most 5 % (otherwise pick another weight seed).  For the case of ``OW_TRAIN`` one training step (focal objective, class weighting) is
stored as oneway_<case>_train.{safetensors,json}: loss, per-tensor gradient norms, the full gradients of ``OW_TRAIN_FULL``, the
reference's own fp32-vs-fp64 gradient error, the tensors that received no gradient and the smallest ReLU pre-activation of the stream MLPs
in the fp64 run relative to the largest, which must lie outside ``KINK_BAND`` (tests/cases_oneway.py says why).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

import torch                            # noqa: E402
from tests.cases_oneway import KINK_BAND, MARGIN, MAX_BAND_SHARE, OW_CASES, OW_TRAIN, OW_TRAIN_FULL, SRC_STRIDE   # noqa: E402


def option(case):
    """What ``_build_lam`` is given beyond the plain model."""
    return {"fusion_transformer": case["cfg"].fusion_transformer}


def band_share(logits, margin):
    """Share of pixels whose top-two gap is within margin * max|finite logit| (the pixels the argmax test does not compare)."""
    top2 = logits.float().topk(2, dim=1).values
    scale = float(logits[torch.isfinite(logits)].abs().max())
    return float(((top2[:, 0] - top2[:, 1]) <= margin * scale).double().mean())


def run_forward(name, case):
    lam, sd, batch, rows = GL.reference_episode(case, **option(case))
    ref_keys = [[k, list(v.shape)] for k, v in lam.state_dict().items()]
    tr = "mask_decoder.transformer."
    assert sorted(k for k, _ in ref_keys) == sorted(sd) and all(list(sd[k].shape) == s for k, s in ref_keys)
    assert [k for k, _ in ref_keys if k.startswith(tr)] == [k for k in sd if k.startswith(tr)], \
        "init_state_dict must give the transformer's keys in the reference's order"
    cfg = case["cfg"]
    b, m, c = batch["flag_examples"].shape
    seen = {}
    hook = lam.mask_decoder.transformer.register_forward_hook(lambda mod, inp, out: seen.update(tokens=out[0], image=out[1]))
    with torch.no_grad():
        seg_low, pe_result = lam._forward(batch)
        hook.remove()
        ref = lam(batch)
    g, d = cfg.grid, cfg.embed_dim
    img = seen["image"]
    assert tuple(img.shape) == (b, g * g, d), img.shape
    assert torch.equal(seen["tokens"], pe_result["class_embeddings"]), "the one-way transformer hands the class tokens back untouched"
    st = SRC_STRIDE
    tensors = {
        "class_embeddings": pe_result["class_embeddings"].contiguous(),
        "transformer_image_sample": img.view(b, g, g, d)[:, ::st, ::st, ::st].flatten(1, 2).contiguous(),
        **GL.logit_tensors(seg_low, ref),
    }
    share = band_share(ref["logits"], MARGIN)
    assert share <= MAX_BAND_SHARE, f"{name}: {share:.3%} of the reference's pixels lie inside the margin band; pick another weight seed"
    assert bool(torch.isfinite(seg_low).all())
    fin = torch.isfinite(ref["logits"])
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "classes": c, "src_stride": st,
            "full_image_shape": list(img.shape), "state_dict": ref_keys, "margin": MARGIN, "margin_band_share": share,
            "image_scale": float(img.abs().max()), "low_res_scale": float(seg_low.abs().max()),
            "finite_logit_fraction": float(fin.double().mean())}
    size = GL.write_fixture(f"oneway_{name}", tensors, meta, rows)
    print(f"[{name}] tensors {len(ref_keys)} classes {c} bytes {size} band share {share:.4f} low-res scale {meta['low_res_scale']:.3f}")


def relu_gaps(lam):
    """ReLU pre-activations of the stream MLPs: how close the step comes to a kink (tests.cases_oneway.KINK_BAND)."""
    pre = []
    for blk in lam.mask_decoder.transformer.layers:
        blk.mlp.lin1.register_forward_hook(lambda mod, inp, out: pre.append(float(out.detach().abs().min() / out.detach().abs().max())))
    return pre


def train():
    name = OW_TRAIN["case"]
    case = OW_CASES[name]
    step = GL.run_train(case, OW_TRAIN["seed_gt"], watch=relu_gaps, **option(case))
    relu_gap = min(step.watched64)
    assert relu_gap >= KINK_BAND, f"{name}: a ReLU pre-activation of the stream MLP lies at {relu_gap:.2e} of the largest; pick another weight seed"
    assert all(f"mask_decoder.transformer.layers.{l}.norm3.{n}" in step.dead for l in range(2) for n in ("weight", "bias"))
    GL.write_train(f"oneway_{name}", step, OW_TRAIN_FULL, "e_ref32", rows=step.rows,
                   meta={"relu_min_gap": relu_gap, "weight_seed": case["weight_seed"]})


if __name__ == "__main__":
    GL.main(OW_CASES, run_forward, [(OW_TRAIN["case"], train)])
