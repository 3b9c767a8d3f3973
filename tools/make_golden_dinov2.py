#!/usr/bin/env python
"""Golden vectors of the DINOv2 ViT encoder from transformers' ``Dinov2Model`` (build container only; tools/golden_lib.py makes the
reference importable for the model case):

    PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dinov2.py [--only NAME] [--no-write]

Encoder cases (tests/cases_dinov2.py ENCODER_CASES): the seeded weights (``init_state_dict``; LayerScale drawn from [0.05, 1.5]) are
strict-loaded into a ``Dinov2Model`` of the case's geometry - its position table is the spec's ``pos_grid``, whatever side the case runs
at - and the seeded images run through it on CPU / fp32.  tests/golden/dinov2_<case>.safetensors holds ``patch_tokens`` =
last_hidden_state without the CLS row, [images, hw, E]; the json the seeds, the geometry and the model's state-dict keys and shapes in
its order.

Model case (MODEL_CASES): the same encoder behind an adapter of this file that drops CLS and reshapes to [B, E, g, g] - what the
reference's ``ViTModelWrapper`` does for a plain ViT - inside the reference's ``_build_lam``; the seeded episode runs through
``Lam.forward``.  The fixture holds low_res_logits, logits and argmax; the json the share of pixels whose top-two logit gap lies inside the
2e-3 margin band on the reference's own logits, which must be at most 5 % (otherwise pick another weight seed).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import tools.golden_lib as GL          # noqa: E402  (makes the reference importable)

import torch                            # noqa: E402
from transformers import Dinov2Config, Dinov2Model    # noqa: E402
from tests.cases_dinov2 import ENCODER_CASES, MARGIN, MAX_BAND_SHARE, MODEL_CASES, encoder_config, encoder_images   # noqa: E402


def hf_model(spec):
    """transformers' model of an EncoderSpec, eval mode."""
    assert spec.mlp % spec.dim == 0
    cfg = Dinov2Config(hidden_size=spec.dim, num_hidden_layers=spec.depth, num_attention_heads=spec.heads, mlp_ratio=spec.mlp // spec.dim,
                       patch_size=spec.patch, image_size=spec.img_size, layer_norm_eps=spec.ln_eps, qkv_bias=True, use_swiglu_ffn=False,
                       hidden_act="gelu")
    return Dinov2Model(cfg).eval()


def load_encoder(model, sd):
    """Strict-load the ``image_encoder.`` tensors of a seeded state dict."""
    pre = "image_encoder."
    model.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}, strict=True)


class PatchGrid(torch.nn.Module):
    """The encoder as the reference's Lam calls one: images -> [B, E, g, g], the CLS row dropped."""

    def __init__(self, model, prefix):
        super().__init__()
        self.model, self.prefix = model, prefix

    def forward(self, pixel_values):
        hs = self.model(pixel_values).last_hidden_state[:, self.prefix:]
        b, hw, e = hs.shape
        g = pixel_values.shape[-1] // self.model.config.patch_size
        return hs.reshape(b, g, g, e).permute(0, 3, 1, 2).contiguous()


def band_share(logits, margin):
    """Share of pixels whose top-two gap is within margin * max|finite logit| (the pixels the argmax test does not compare)."""
    top2 = logits.float().topk(2, dim=1).values
    scale = float(logits[torch.isfinite(logits)].abs().max())
    return float(((top2[:, 0] - top2[:, 1]) <= margin * scale).double().mean())


def run_encoder(name, case):
    from labelanything_amd.weights import init_state_dict
    cfg = encoder_config(case)
    spec = cfg.encoder_spec
    model = hf_model(spec)
    load_encoder(model, init_state_dict(cfg, case["weight_seed"]))
    with torch.no_grad():
        hs = model(encoder_images(case)).last_hidden_state
    t = (case["side"] // spec.patch) ** 2 + spec.prefix_tokens
    assert tuple(hs.shape) == (case["images"], t, spec.dim) and bool(torch.isfinite(hs).all())
    out = hs[:, spec.prefix_tokens:].contiguous()
    meta = {"case": name, **{k: case[k] for k in ("encoder", "side", "images", "weight_seed", "image_seed", "path")}, "tokens": t,
            "state_dict": [[k, list(v.shape)] for k, v in model.state_dict().items()], "scale": float(out.abs().max())}
    size = GL.write_fixture(f"dinov2_{name}", {"patch_tokens": out}, meta)
    print(f"[{name}] tokens {t} output {tuple(out.shape)} scale {meta['scale']:.3f} bytes {size}")


def run_model(name, case):
    from label_anything.models.build_lam import _build_lam
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.weights import init_state_dict
    cfg = case["cfg"]
    spec = cfg.encoder_spec
    vit = PatchGrid(hf_model(spec), spec.prefix_tokens)
    lam = _build_lam(build_vit=(lambda project_last_hidden=True: vit), use_vit=True, use_vit_sam_neck=cfg.use_vit_sam_neck,
                     image_embed_dim=cfg.image_embed_dim, embed_dim=cfg.embed_dim, image_size=cfg.image_size, vit_patch_size=cfg.vit_patch_size,
                     class_attention=cfg.class_attention, example_attention=cfg.example_attention,
                     example_class_attention=cfg.example_class_attention, spatial_convs=cfg.spatial_convs,
                     class_encoder=dict(cfg.class_encoder) if cfg.class_encoder else None, custom_preprocess=cfg.custom_preprocess)
    lam.eval()
    sd = init_state_dict(cfg, case["weight_seed"])
    load_encoder(vit.model, sd)
    res = lam.load_state_dict({k: v for k, v in sd.items() if not k.startswith("image_encoder.")}, strict=False)
    assert all(k.startswith("image_encoder.") for k in res.missing_keys) and not res.unexpected_keys, res
    batch = make_episode(**case["episode"])
    rows = GL.fixed_rows(lam, case, batch["flag_examples"].shape[2])
    with torch.no_grad():
        seg_low, _ = lam._forward(batch)
        ref = lam(batch)
    share = band_share(ref["logits"], MARGIN)
    assert share <= MAX_BAND_SHARE, f"{name}: {share:.3%} of the reference's pixels lie inside the margin band; pick another weight seed"
    assert bool(torch.isfinite(seg_low).all())
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "margin": MARGIN, "margin_band_share": share,
            "low_res_scale": float(seg_low.abs().max())}
    size = GL.write_fixture(f"dinov2_{name}", GL.logit_tensors(seg_low, ref), meta, rows)
    print(f"[{name}] bytes {size} band share {share:.4f} low-res scale {meta['low_res_scale']:.3f}")


def forward(name, case):
    (run_encoder if name in ENCODER_CASES else run_model)(name, case)


if __name__ == "__main__":
    GL.main({**ENCODER_CASES, **MODEL_CASES}, forward)
