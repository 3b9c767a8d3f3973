#!/usr/bin/env python
"""Golden vectors of the two-level classification head (``classification_levels=2``) from the REFERENCE (build container only;
tools/golden_lib.py imports it):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_levels.py [--only NAME] [--no-train]

For every case of tests/cases_levels.py the seeded weights (``init_state_dict``, including ``mask_decoder.level_reducer.*``; the state dict
strict-loads) go into ``_build_lam(..., classification_levels=2)``, the seeded episode runs through the reference's ``Lam.forward`` on
CPU / fp32 and the reference's OUTPUTS are written to tests/golden/levels_<case>.safetensors: both ``_classify`` outputs (cls1 = the coarse
level, cls0 = the fine level), the operands of the first one (the transformer's tokens and image stream), low_res_logits, logits, argmax,
selected_rows.

ONE CALL IS NOT THE REFERENCE'S OWN: mask_decoder.py:359 calls torchvision's ``resize``, and torchvision is not installed where this runs.
The stand-in installed into the reference's ``mask_decoder`` module is what torchvision's ``resize`` does with a float tensor:
``F.interpolate(img, size, mode="bilinear", align_corners=False, antialias=True)``.  The json says so too (``resize_stand_in``).

For ``LV_TRAIN`` one decoder-only training step (WrapperModule + focal loss, as tools/make_golden_train.py) is stored as
levels_<case>_train: loss, per-tensor gradient norms, a handful of full gradients (both level_reducer tensors among them), and ``e_kink`` -
the worst per-tensor difference between the reference's own fp32 and fp64 gradients, relative to the tensor's scale floored at 1e-2 of the
model's largest gradient.

``level_reducer.bias`` is INERT in this step: it is added to every class plane alike and the focal objective is a softmax cross-entropy, so
its gradient - the sum of d loss / d low_res_logits over all classes and pixels - is zero analytically; what the reference stores for it is
rounding noise (1e-7 against a largest gradient of 2e-2, 1e-17 in fp64).  It is therefore left out of ``e_kink`` and of the json's ``keys``
(it is listed under ``inert``), and the json carries what a test needs to bound that noise instead: ``dseg_abs_sum`` = sum |d loss /
d low_res_logits| and ``dseg_numel``, from the fp64 run.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

import torch                            # noqa: E402
import torch.nn.functional as F         # noqa: E402
import label_anything.models.mask_decoder as REF_MD      # noqa: E402  (the reference)
from tests.cases_levels import LV_CASES, LV_TRAIN, LV_TRAIN_FULL   # noqa: E402

INERT = "mask_decoder.level_reducer.bias"      # zero gradient under a softmax objective: see the docstring
RESIZE_STAND_IN = 'F.interpolate(img, size, mode="bilinear", align_corners=False, antialias=True)'


def resize_stand_in(img, size, *a, **kw):
    return F.interpolate(img, size=tuple(size), mode="bilinear", align_corners=False, antialias=True)


REF_MD.resize = resize_stand_in


def run_forward(name, case):
    lam, _, batch, rows = GL.reference_episode(case, classification_levels=case["cfg"].classification_levels)
    calls = GL.spy_classify(lam)
    with torch.no_grad():
        seg_low, _ = lam._forward(batch)
        n_calls = len(calls)
        ref = lam(batch)
    assert n_calls == 2, n_calls
    (img, tok, cls1), (_, _, cls0) = calls[:2]
    b, d, g, _ = img.shape
    tensors = {
        "tokens": tok.contiguous(),                                             # (B, C, D): the transformer's output tokens
        "image_rows": img.flatten(2).transpose(1, 2).contiguous(),              # (B, g*g, D) NHWC: the transformer's image stream
        "cls1": cls1.contiguous(),                                              # (B, C, g, g)
        "cls0": cls0.contiguous(),                                              # (B, C, 4g, 4g)
        **GL.logit_tensors(seg_low, ref),
    }
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "grid": int(g),
            "resize_stand_in": RESIZE_STAND_IN,
            "resize_note": "mask_decoder.py:359 calls torchvision's resize; torchvision is not installed where the fixture was made, this one "
                           "call is the stand-in above and not the reference's own",
            "scale": {"cls1": float(cls1.abs().max()), "cls0": float(cls0.abs().max()), "low_res_logits": float(seg_low.abs().max())}}
    size = GL.write_fixture(f"levels_{name}", tensors, meta, rows)
    print(f"[{name}] grid {g} bytes {size} scale {meta['scale']}")


def reducer_output(lam):
    """The level reducer's output with its gradient retained: d loss / d low_res_logits."""
    seen = []

    def keep(module, inputs, output):
        output.retain_grad()
        seen.append(output)

    lam.mask_decoder.level_reducer.register_forward_hook(keep)
    return seen


def train():
    name = LV_TRAIN["case"]
    step = GL.run_train(LV_CASES[name], LV_TRAIN["seed_gt"], watch=reducer_output,
                        classification_levels=LV_CASES[name]["cfg"].classification_levels)
    assert len(step.watched64) == 1
    dseg64 = step.watched64[0].grad.detach()
    assert float(step.g64[INERT].abs().max()) <= 1e-12 * max(float(step.g64[k].abs().max()) for k in step.keys)     # zero analytically
    inert32, inert64 = step.g32.pop(INERT), step.g64.pop(INERT)               # out of keys, grad_norm and e_kink
    GL.write_train(f"levels_{name}", step, [k for k in LV_TRAIN_FULL if k != INERT], "e_kink", tensors={"grad." + INERT: inert32.contiguous()},
                   meta={"inert": [INERT], "inert_reference_fp32": float(inert32.abs().max()), "inert_reference_fp64": float(inert64.abs().max()),
                         "dseg_abs_sum": float(dseg64.abs().sum()), "dseg_numel": int(dseg64.numel()), "resize_stand_in": RESIZE_STAND_IN})


if __name__ == "__main__":
    GL.main(LV_CASES, run_forward, [(LV_TRAIN["case"], train)])
