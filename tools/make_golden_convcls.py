#!/usr/bin/env python
"""Golden vectors of ``conv_classification`` / ``classification_layer_downsample_rate=1`` from the REFERENCE (build container only;
tools/golden_lib.py imports it):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_convcls.py [--only NAME] [--no-train]

For every case of tests/cases_convcls.py the seeded weights (``init_state_dict``, including ``mask_decoder.prototype_tconv.*``; the state
dict strict-loads) go into ``_build_lam(..., classification_layer_downsample_rate=r, conv_classification=...)``, the seeded episode runs
through the reference's ``Lam.forward`` on CPU / fp32 and the reference's OUTPUTS are written to tests/golden/<case>.safetensors:
low_res_logits, logits, argmax, selected_rows.  The operands of the final ``_classify`` (the feature map as NHWC rows and the prototypes) go
to <case>_feat.safetensors for the conv cases; at cf = 256 the map is 4 MB, so only its first ``feature_rows`` rows are kept (the json says
how many): they determine the logit rows 0 .. feature_rows - 3.

The json holds the model's key list and shapes, the initialisation scale of prototype_tconv (weights.PROTOTYPE_TCONV_FAN) and the measured
magnitude of the low-resolution logits.

For ``CC_TRAIN`` (and ``CC_TRAIN_PLAIN``, the same step without the two tensors) one decoder-only training step (WrapperModule + focal loss, as tools/make_golden_train.py) is stored as <case>_train:
loss, per-tensor gradient norms, a handful of full gradients (of the two prototype_tconv tensors the first CC_TCONV_ROWS input channels),
and ``e_kink`` - the worst per-tensor difference between the reference's own fp32 and fp64 gradients, relative to the tensor's scale
floored at 1e-2 of the model's largest gradient.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

import torch                            # noqa: E402
from labelanything_amd.weights import PROTOTYPE_TCONV_FAN   # noqa: E402
from tests.cases_convcls import CC_CASES, CC_TRAIN, CC_TRAIN_PLAIN, CC_TRAIN_FULL, CC_TCONV, CC_TCONV_ROWS   # noqa: E402

FEATURE_BYTES = 900_000                 # what <case>_feat.safetensors may spend on feature rows


def option(case):
    """What ``_build_lam`` is given beyond the plain model."""
    cfg = case["cfg"]
    return {"classification_layer_downsample_rate": cfg.classification_layer_downsample_rate, "conv_classification": cfg.conv_classification}


def run_forward(name, case):
    lam, sd, batch, rows = GL.reference_episode(case, **option(case))
    cfg = case["cfg"]
    calls = GL.spy_classify(lam)
    with torch.no_grad():
        seg_low, _ = lam._forward(batch)
        n_calls = len(calls)
        ref = lam(batch)
    assert n_calls == 1, n_calls
    feat, protos, seg = calls[0]
    assert torch.equal(seg, seg_low)
    b, cf, h, w = feat.shape
    assert cf == cfg.class_width
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "grid": int(h // 4),
            **option(case), "class_width": int(cf),
            "reference_shapes": {k: list(v.shape) for k, v in lam.state_dict().items()},
            "scale": {"low_res_logits": float(seg_low.abs().max()), "low_res_logits_rms": float(seg_low.pow(2).mean().sqrt()),
                      "features": float(feat.abs().max()), "prototypes": float(protos.abs().max())},
            "torch": None, "generated_by": None}      # filled in by write_fixture; named here to keep their place before the fields below
    sizes = []
    if cfg.conv_classification:
        keep = min(h, FEATURE_BYTES // (4 * cf * w * b))
        feat_rows = feat[:, :, :keep].permute(0, 2, 3, 1).contiguous()          # (B, rows, W, cf) NHWC
        sizes.append(GL.write_fixture(f"{name}_feat", {"feature_rows": feat_rows, "prototypes": protos.contiguous()}, None))
        meta["feature_rows"] = int(keep)
        meta["prototype_tconv_init"] = {"std": float((PROTOTYPE_TCONV_FAN * cf) ** -0.5), "fan": PROTOTYPE_TCONV_FAN * int(cf),
                                        "measured_std": float(sd["mask_decoder.prototype_tconv.0.weight"].std())}
    sizes.insert(0, GL.write_fixture(name, GL.logit_tensors(seg_low, ref), meta, rows))
    print(f"[{name}] cf {cf} map {h} x {w} bytes {sizes} scale {meta['scale']}")


def train(spec, tconv, tconv_rows):
    """``tconv``: the tensors of which only the first ``tconv_rows`` input channels are stored."""
    name = spec["case"]
    step = GL.run_train(CC_CASES[name], spec["seed_gt"], **option(CC_CASES[name]))
    assert all(k in step.keys for k in tconv)
    tensors = {"grad_max": torch.stack([step.g32[k].abs().max() for k in step.keys])}
    tensors.update({"grad." + k: step.g32[k][:tconv_rows].contiguous() for k in tconv})
    GL.write_train(name, step, CC_TRAIN_FULL, "e_kink", tensors=tensors, meta={"sliced": {k: tconv_rows for k in tconv}})


if __name__ == "__main__":
    GL.main(CC_CASES, run_forward, [(CC_TRAIN["case"], lambda: train(CC_TRAIN, CC_TCONV, CC_TCONV_ROWS)),
                                    (CC_TRAIN_PLAIN["case"], lambda: train(CC_TRAIN_PLAIN, [], 0))])
