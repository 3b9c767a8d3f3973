#!/usr/bin/env python
"""Golden vectors of the TokenPool prompt encoder from the REFERENCE (build container only; builds on tools/make_golden.py's stub finder):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_token_pool.py [--only NAME] [--no-train]

For every case of tests/cases_token_pool.py the seeded weights (``init_state_dict``: TokenPool adds no tensor) are strict-loaded into
``_build_lam(..., prompt_encoder="TokenPool")`` and the seeded episode runs through the reference's ``Lam.forward`` on CPU / fp32, the
class-encoder rows pinned as tools/make_golden_multi_embedding.py:fixed_rows does.  tests/golden/token_pool_<case>.safetensors holds the
reference's OUTPUTS: class_embeddings, class_examples_embeddings, low_res_logits, logits, argmax and every ``SRC_STRIDE``-th pixel row,
pixel column and channel of class_examples_src (the image side of the two-way transformer, one slab per support image).  For the case
of ``TP_TRAIN`` one training step (focal objective, class weighting) is stored as token_pool_<case>_train.{safetensors,json}: loss,
per-tensor gradient norms, the full gradients of ``TP_TRAIN_FULL``, the reference's own fp32-vs-fp64 gradient error and the tensors that
received no gradient.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tools.make_golden as MG          # noqa: E402,F401  (installs the stub finder, puts the reference first on sys.path)

import torch                            # noqa: E402
from safetensors.torch import save_file  # noqa: E402
from label_anything.models.build_lam import _build_lam   # noqa: E402  (the reference)

GOLDEN = os.path.join(ROOT, "tests", "golden")
FINAL = ("prompt_encoder.transformer.final_attn_token_to_image.", "prompt_encoder.transformer.norm_final_attn.")


def build_reference(case, prompt_encoder="TokenPool"):
    from labelanything_amd.weights import init_state_dict
    cfg = case["cfg"]
    assert cfg.encoder_spec is None, "decoder-only cases"
    lam = _build_lam(
        build_vit=None, use_vit=False, image_embed_dim=cfg.image_embed_dim, embed_dim=cfg.embed_dim, image_size=cfg.image_size,
        class_attention=cfg.class_attention, example_attention=cfg.example_attention, example_class_attention=cfg.example_class_attention,
        spatial_convs=cfg.spatial_convs, class_encoder=dict(cfg.class_encoder) if cfg.class_encoder else None,
        custom_preprocess=cfg.custom_preprocess, prompt_encoder=prompt_encoder)
    lam.eval()
    sd = init_state_dict(cfg, case["weight_seed"])
    lam.load_state_dict(sd, strict=True)
    return lam, sd


def run_forward(name, case):
    from labelanything_amd.episodes import make_episode
    from tests.cases_token_pool import SRC_STRIDE
    from tools.make_golden_multi_embedding import fixed_rows
    lam, sd = build_reference(case)
    plain, _ = build_reference(case, prompt_encoder=None)
    assert list(lam.state_dict()) == list(plain.state_dict()) and sorted(lam.state_dict()) == sorted(sd), "TokenPool must not add or rename a tensor"
    cfg = case["cfg"]
    batch = make_episode(**case["episode"])
    b, m, c = batch["flag_examples"].shape
    rows = fixed_rows(lam, case, c)
    with torch.no_grad():
        seg_low, pe_result = lam._forward(batch)
        ref = lam(batch)
    cee, cls, src = pe_result["class_examples_embeddings"], pe_result["class_embeddings"], pe_result["class_examples_src"]
    g = cfg.grid
    assert tuple(cee.shape) == (b, m, c, cfg.embed_dim) and tuple(cls.shape) == (b, c, cfg.embed_dim)
    assert tuple(src.shape) == (b * m, g * g, cfg.embed_dim), src.shape                     # one slab per support image, in rows
    assert torch.equal(ref["class_examples_embeddings"], cee)
    st = SRC_STRIDE
    tensors = {
        "class_embeddings": cls.contiguous(),
        "class_examples_embeddings": cee.contiguous(),
        "low_res_logits": seg_low.contiguous(),
        "logits": ref["logits"].contiguous(),
        "argmax": ref["logits"].argmax(dim=1).to(torch.uint8).contiguous(),
        # rows, as the reference returns them and the engine holds the stream: (B M, h' w', D')
        "class_examples_src_sample": src.view(b * m, g, g, -1)[:, ::st, ::st, ::st].flatten(1, 2).contiguous(),
    }
    if rows is not None:
        tensors["selected_rows"] = rows
    path = os.path.join(GOLDEN, f"token_pool_{name}.safetensors")
    save_file(tensors, path)
    fin = torch.isfinite(ref["logits"])
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "supports": b * m, "classes": c,
            "src_stride": st, "full_src_shape": list(src.shape), "state_dict_keys_equal_plain": True,
            "embedding_scale": float(cee.abs().max()), "low_res_scale": float(seg_low.abs().max()),
            "finite_logit_fraction": float(fin.double().mean()), "torch": torch.__version__,
            "generated_by": "tools/make_golden_token_pool.py"}
    with open(os.path.join(GOLDEN, f"token_pool_{name}.json"), "w") as fh:
        json.dump(meta, fh, indent=1, default=list)
    assert bool(torch.isfinite(seg_low).all())
    print(f"[{name}] supports {b * m} classes {c} bytes {os.path.getsize(path)} scale {meta['embedding_scale']:.3f}")


def grads_of(case, gt, double: bool):
    from label_anything.experiment.utils import WrapperModule
    from label_anything.loss import LabelAnythingLoss
    from labelanything_amd.episodes import make_episode
    from tools.make_golden_multi_embedding import fixed_rows
    lam, sd = build_reference(case)
    lam.train()
    batch = make_episode(**case["episode"])
    if double:
        lam.double()
        batch = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}
    rows = fixed_rows(lam, case, batch["flag_examples"].shape[2])
    model = WrapperModule(lam, LabelAnythingLoss({"focal": {"weight": 1.0}}, class_weighting=True))
    res = model(batch, gt)
    loss = res["loss"]["value"]
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in lam.named_parameters()}
    assert all(k in sd for k in grads)
    return float(loss), grads, rows


def run_train(name, case, seed_gt, full):
    from labelanything_amd.episodes import make_episode
    from tests.helpers import make_gt
    batch = make_episode(**case["episode"])
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=seed_gt)
    loss32, g32, rows = grads_of(case, gt, double=False)
    loss64, g64, _ = grads_of(case, gt, double=True)
    keys = sorted(k for k, g in g32.items() if g is not None)
    assert keys == sorted(k for k, g in g64.items() if g is not None)
    dead = sorted(k for k, g in g32.items() if g is None)
    assert not any(k.startswith(FINAL) for k in dead), "final_attn / norm_final_attn are live under TokenPool"
    assert all(float(g32[k].abs().max()) > 0 for k in keys if k.startswith(FINAL))
    gmax = max(float(g64[k].abs().max()) for k in keys)
    # the reference's own fp32 error on every gradient tensor, in the units of the tests' bound: of the tensor's scale, floored at 1e-2
    # of the largest gradient
    e32 = {k: float((g32[k].double() - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-2 * gmax) for k in keys}
    out = {"loss": torch.tensor([loss32]), "grad_norm": torch.stack([g32[k].norm() for k in keys])}
    if rows is not None:
        out["selected_rows"] = rows
    for k in full:
        out["grad." + k] = g32[k].contiguous()
    path = os.path.join(GOLDEN, f"token_pool_{name}_train.safetensors")
    save_file(out, path)
    with open(os.path.join(GOLDEN, f"token_pool_{name}_train.json"), "w") as fh:
        json.dump({"keys": keys, "dead": dead, "loss": loss32, "loss_fp64": loss64, "e_ref32": max(e32.values()),
                   "e_ref32_worst_tensor": max(e32, key=e32.get), "seed_gt": seed_gt, "torch": torch.__version__,
                   "generated_by": "tools/make_golden_token_pool.py"}, fh, indent=1)
    print(f"[{name} train] loss {loss32:.8f} (fp64 {loss64:.8f}) e_ref32 {max(e32.values()):.3e} at {max(e32, key=e32.get)} "
          f"tensors {len(keys)} dead {dead} bytes {os.path.getsize(path)}")


def main():
    from tests.cases_token_pool import TP_CASES, TP_TRAIN, TP_TRAIN_FULL
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--no-train", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    for name, case in TP_CASES.items():
        if a.only in (None, name):
            run_forward(name, case)
    if not a.no_train and a.only in (None, TP_TRAIN["case"]):
        run_train(TP_TRAIN["case"], TP_CASES[TP_TRAIN["case"]], TP_TRAIN["seed_gt"], TP_TRAIN_FULL)


if __name__ == "__main__":
    main()
