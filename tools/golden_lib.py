"""What the fixture generators (tools/make_golden*.py, build container only) share.

Importing this module makes the REFERENCE importable: the real third-party imports first, then a finder that answers the reference's
off-path dependencies with empty stub modules, then the reference's root FIRST on sys.path, so that its
``label_anything`` wins over this repository's same-named shim.  The reference's own modules are imported where they are used, never
here, so a generator may still put a stand-in of its own in place of a stub (tools/make_golden_metrics_iou.py does).

For the generators that build a model it also holds the model (``build_reference``, ``reference_episode``), the reference's training
step in fp32 and fp64 (``run_train``, ``write_train``), the fixture files (``write_fixture``) and the command line (``main``); for the
generators of an encoder family (DINOv2, DINOv3) everything but the transformers model (``encoder_family_main``).
Nothing of the reference travels: fixtures hold seeds and the reference's outputs only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import types
import importlib.abc
import importlib.machinery
from functools import partial

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

# real imports FIRST (a fake torchvision breaks transformers' lazy imports)
import torch
from transformers import ViTModel, AutoModel, AutoBackbone, get_scheduler, ViTConfig  # noqa: F401
from transformers.configuration_utils import PretrainedConfig  # noqa: F401
import transformers.utils.constants  # noqa: F401
import accelerate, huggingface_hub, safetensors.torch  # noqa: F401,E401
from safetensors.torch import save_file

STUB_ROOTS = {"ruamel", "torchvision", "pycocotools", "torchmetrics", "wandb", "easydict", "cv2", "timm",
              "dropblock", "lovely_tensors", "captum", "optuna", "wget", "nicegui", "streamlit", "colorlog",
              "skimage", "kornia", "streamlit_drawable_canvas", "sklearn"}


class _Stub(types.ModuleType):
    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        return type(k, (object,), {"__init__": lambda s, *a, **kw: None, "__call__": lambda s, *a, **kw: None,
                                   "__getattr__": lambda s, k: (lambda *a, **kw: None)})


class _Loader(importlib.abc.Loader):
    def create_module(self, spec):
        m = _Stub(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


class _Finder(importlib.abc.MetaPathFinder):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in STUB_ROOTS:
            return importlib.machinery.ModuleSpec(name, _Loader(), is_package=True)


REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
sys.meta_path.insert(0, _Finder())
# the reference package must win over this repo's same-named shim (label_anything/): its root goes first, the repo last
sys.path[:] = [p for p in sys.path if os.path.abspath(p or ".") != REPO]
sys.path.insert(0, "/root/reference")
sys.path.append(REPO)

WRITE = True            # --no-write: run the reference and the generator's own checks, write nothing


def _hf_4x_to_local(sd, model):
    """Map transformers-4.x ViT key names (ours) onto whatever this container's transformers uses."""
    local = set(model.state_dict().keys())
    out = {}
    for k, v in sd.items():
        cands = [k]
        k5 = (k.replace("encoder.layer.", "layers.")
               .replace("attention.attention.query", "attention.q_proj")
               .replace("attention.attention.key", "attention.k_proj")
               .replace("attention.attention.value", "attention.v_proj")
               .replace("attention.output.dense", "attention.o_proj")
               .replace("intermediate.dense", "mlp.fc1")
               .replace("output.dense", "mlp.fc2"))
        cands.append(k5)
        cands.append(k5.replace("layers.", "encoder.layers."))
        hit = [c for c in cands if c in local]
        if not hit:
            raise KeyError(f"cannot map {k}; e.g. local keys: {sorted(local)[:12]}")
        out[hit[0]] = v
    return out


def build_reference(case, **extra):
    """The reference's model of ``case["cfg"]`` in eval mode with the seeded weights (``init_state_dict``) strict-loaded -> (lam, sd).
    ``extra`` goes to the reference's ``_build_lam`` as it stands: the keyword arguments of the model option a generator is about."""
    from label_anything.models.image_encoder import ImageEncoderViT
    from label_anything.models.build_encoder import ViTModelWrapper
    from label_anything.models.build_lam import _build_lam
    from labelanything_amd.weights import init_state_dict
    cfg = case["cfg"]
    spec = cfg.encoder_spec
    vit = None
    if spec is not None and spec.kind == "sam":
        vit = ImageEncoderViT(
            img_size=spec.img_size, patch_size=spec.patch, embed_dim=spec.dim, depth=spec.depth,
            num_heads=spec.heads, mlp_ratio=spec.mlp / spec.dim, out_chans=spec.out_chans, qkv_bias=True,
            norm_layer=partial(torch.nn.LayerNorm, eps=1e-6), use_rel_pos=True,
            global_attn_indexes=spec.global_idx, window_size=spec.window,
            project_last_hidden=cfg.use_vit_sam_neck)
    elif spec is not None and spec.kind == "hf":
        vit = ViTModelWrapper(ViTConfig(
            hidden_size=spec.dim, num_hidden_layers=spec.depth, num_attention_heads=spec.heads,
            intermediate_size=spec.mlp, patch_size=spec.patch, image_size=spec.img_size,
            layer_norm_eps=1e-12, qkv_bias=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0),
            add_pooling_layer=False)
    lam = _build_lam(
        build_vit=(lambda project_last_hidden=True: vit), use_vit=vit is not None,
        use_vit_sam_neck=cfg.use_vit_sam_neck, image_embed_dim=cfg.image_embed_dim, embed_dim=cfg.embed_dim,
        image_size=cfg.image_size, class_attention=cfg.class_attention, example_attention=cfg.example_attention,
        example_class_attention=cfg.example_class_attention, spatial_convs=cfg.spatial_convs,
        class_encoder=dict(cfg.class_encoder) if cfg.class_encoder else None,
        custom_preprocess=cfg.custom_preprocess, **extra)
    lam.eval()
    sd = init_state_dict(cfg, case["weight_seed"])
    if spec is not None and spec.kind == "hf":
        enc = {k[len("image_encoder."):]: v for k, v in sd.items() if k.startswith("image_encoder.")}
        enc = _hf_4x_to_local(enc, lam.image_encoder)
        missing, unexpected = lam.image_encoder.load_state_dict(enc, strict=False)
        missing = [k for k in missing if "pooler" not in k]
        assert not missing and not unexpected, (missing, unexpected)
        rest = {k: v for k, v in sd.items() if not k.startswith("image_encoder.")}
        res = lam.load_state_dict(rest, strict=False)
        assert all(k.startswith("image_encoder.") for k in res.missing_keys) and not res.unexpected_keys, res
    else:
        lam.load_state_dict(sd, strict=True)
    return lam, sd


def fixed_rows(lam, case, c):
    """Models with a class encoder draw their bank rows at random: put a seeded draw in place of ``sample_rows`` -> the rows, or None."""
    cfg = case["cfg"]
    if not cfg.bank_size:
        return None
    gr = torch.Generator().manual_seed(case["weight_seed"] + 7)
    rows = torch.cat([torch.zeros(1, dtype=torch.long), torch.randperm(cfg.bank_size - 1, generator=gr)[: c - 1] + 1])
    lam.prompt_encoder.class_encoder.sample_rows = lambda C, device, _r=rows: _r.to(device)
    return rows


def reference_episode(case, double=False, **extra):
    """-> (lam, sd, batch, rows): the reference's model, the case's seeded episode (both in fp64 if ``double``) and the pinned rows."""
    from labelanything_amd.episodes import make_episode
    lam, sd = build_reference(case, **extra)
    batch = make_episode(**case["episode"])
    if double:
        lam.double()
        batch = {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}
    return lam, sd, batch, fixed_rows(lam, case, batch["flag_examples"].shape[2])


def spy_classify(lam):
    """Record every call of the mask decoder's ``_classify`` -> the list that fills with (features, prototypes, output)."""
    calls = []
    md = lam.mask_decoder
    orig = md._classify

    def spy(query_embeddings, class_embeddings, flag_examples):
        out = orig(query_embeddings, class_embeddings, flag_examples)
        calls.append((query_embeddings.detach().clone(), class_embeddings.detach().clone(), out.detach().clone()))
        return out

    md._classify = spy
    return calls


def logit_tensors(seg_low, ref):
    """The three tensors every forward fixture holds, from ``lam._forward``'s low-resolution logits and ``lam.forward``'s result."""
    return {"low_res_logits": seg_low.contiguous(), "logits": ref["logits"].contiguous(),
            "argmax": ref["logits"].argmax(dim=1).to(torch.uint8).contiguous()}


def focal_wrapper(lam):
    """The module the reference trains: the model under its focal objective with class weighting (experiment/utils.py:266-303)."""
    from label_anything.experiment.utils import WrapperModule
    from label_anything.loss import LabelAnythingLoss
    return WrapperModule(lam, LabelAnythingLoss({"focal": {"weight": 1.0}}, class_weighting=True))


def grads_of(case, gt, double, watch=None, **extra):
    """One forward and backward of the reference in train mode -> (loss, {name: gradient or None}, rows, watched).  ``watch(lam)`` runs
    before the forward: the caller hangs its hooks on the model there, and whatever it returns is handed back once the backward is done."""
    lam, sd, batch, rows = reference_episode(case, double=double, **extra)
    lam.train()
    watched = watch(lam) if watch else None
    loss = focal_wrapper(lam)(batch, gt)["loss"]["value"]
    loss.backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in lam.named_parameters()}
    assert all(k in sd for k in grads)
    return float(loss), grads, rows, watched


class Step:
    """The reference's training step in fp32 and in fp64: loss32 / loss64, g32 / g64 ({name: gradient or None}), watched32 / watched64,
    rows, seed_gt.  A generator that sets a tensor aside pops it from g32 and g64; ``keys`` and ``dead`` follow."""
    keys = property(lambda s: sorted(k for k, g in s.g32.items() if g is not None))
    dead = property(lambda s: sorted(k for k, g in s.g32.items() if g is None))


def run_train(case, seed_gt, watch=None, **extra):
    """The reference's training step on the case's episode and ``make_gt(seed_gt)``, once in fp32 and once in fp64 -> Step."""
    from labelanything_amd.episodes import make_episode
    from tests.helpers import make_gt
    batch = make_episode(**case["episode"])
    s = Step()
    s.seed_gt = seed_gt
    # (the ground truth is not stored: tests rebuild it with make_gt(seed_gt))
    gt = make_gt(batch, batch["flag_examples"].shape[2], seed=seed_gt)
    s.loss32, s.g32, s.rows, s.watched32 = grads_of(case, gt, False, watch, **extra)
    s.loss64, s.g64, _, s.watched64 = grads_of(case, gt, True, watch, **extra)
    return s


def write_train(stem, step, full, err_name, tensors=None, meta=None, rows=None):
    """Write ``<stem>_train``: loss, per-tensor gradient norms and the full gradients of ``full`` (+ ``tensors``, ``rows``); in the json the
    live and the dead tensors and ``err_name``, the reference's own fp32 error (+ ``meta``)."""
    g32, g64, keys = step.g32, step.g64, step.keys
    assert keys == sorted(k for k, g in g64.items() if g is not None)
    gmax = max(float(g64[k].abs().max()) for k in keys)
    # the reference's own fp32 error on every gradient tensor, in the units of the tests' bound: of the tensor's scale, floored at 1e-2
    # of the largest gradient
    err = {k: float((g32[k].double() - g64[k]).abs().max()) / max(float(g64[k].abs().max()), 1e-2 * gmax) for k in keys}
    worst = max(err, key=err.get)
    out = {"loss": torch.tensor([step.loss32]), "grad_norm": torch.stack([g32[k].norm() for k in keys])}
    out.update({"grad." + k: g32[k].contiguous() for k in full})
    out.update(tensors or {})
    size = write_fixture(stem + "_train", out, {"keys": keys, "dead": step.dead, "loss": step.loss32, "loss_fp64": step.loss64,
                                                err_name: err[worst], err_name + "_worst_tensor": worst, "seed_gt": step.seed_gt,
                                                **(meta or {})}, rows)
    print(f"[{stem} train] loss {step.loss32:.8f} (fp64 {step.loss64:.8f}) {err_name} {err[worst]:.3e} at {worst} tensors {len(keys)} "
          f"dead {step.dead} bytes {size}")


def write_fixture(stem, tensors, meta, rows=None):
    """tests/golden/<stem>.safetensors (+ ``selected_rows`` where the model drew rows) and, if ``meta`` is given, <stem>.json, which
    ends with the torch version and the generator's name -> the bytes of the .safetensors."""
    if not WRITE:
        return 0
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, stem + ".safetensors")
    save_file(tensors if rows is None else {**tensors, "selected_rows": rows}, path)
    if meta is not None:
        by = "tools/" + os.path.basename(sys.modules["__main__"].__file__)
        with open(os.path.join(GOLDEN, stem + ".json"), "w") as fh:
            json.dump({**meta, "torch": torch.__version__, "generated_by": by}, fh, indent=1, default=list)
    return os.path.getsize(path)


# ---- encoder families (tools/make_golden_dinov2.py, tools/make_golden_dinov3.py): transformers' model of the family on the seeded weights.
# A script gives ``hf_model(spec, side)`` - its transformers config and model, eval mode - and, where this transformers spells the keys
# otherwise, ``spell(key, the model's keys)``; ``cases`` is the family's tests/cases_<family>.py. ----
class PatchGrid(torch.nn.Module):
    """The encoder as the reference's Lam calls one: images -> [B, E, g, g], the prefix rows (CLS, registers) dropped - what the
    reference's ``ViTModelWrapper`` does for a plain ViT."""

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


def load_encoder(model, sd, spell=None):
    """Strict-load the ``image_encoder.`` tensors of a seeded state dict, in the key spelling of this transformers."""
    pre, local = "image_encoder.", set(model.state_dict())
    enc = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
    model.load_state_dict({(spell(k, local) if spell else k): v for k, v in enc.items()}, strict=True)


def encoder_fixture(family, cases, hf_model, spell, name, case):
    """<family>_<name>: ``patch_tokens`` = last_hidden_state without the prefix rows, [images, hw, E], on CPU / fp32; the json holds the
    seeds, the geometry and the model's state-dict keys and shapes in its order."""
    from labelanything_amd.weights import init_state_dict
    cfg = cases.encoder_config(case)
    spec = cfg.encoder_spec
    model = hf_model(spec, case["side"])
    load_encoder(model, init_state_dict(cfg, case["weight_seed"]), spell)
    with torch.no_grad():
        hs = model(cases.encoder_images(case)).last_hidden_state
    t = (case["side"] // spec.patch) ** 2 + spec.prefix_tokens
    assert tuple(hs.shape) == (case["images"], t, spec.dim) and bool(torch.isfinite(hs).all())
    out = hs[:, spec.prefix_tokens:].contiguous()
    meta = {"case": name, **{k: case[k] for k in ("encoder", "side", "images", "weight_seed", "image_seed", "path")}, "tokens": t,
            "state_dict": [[k, list(v.shape)] for k, v in model.state_dict().items()], "scale": float(out.abs().max())}
    size = write_fixture(f"{family}_{name}", {"patch_tokens": out}, meta)
    print(f"[{name}] tokens {t} output {tuple(out.shape)} scale {meta['scale']:.3f} bytes {size}")


def encoder_model_fixture(family, cases, hf_model, spell, name, case):
    """<family>_<name>: the family's encoder behind ``PatchGrid`` inside the reference's ``_build_lam``, the seeded episode through
    ``Lam.forward``: low_res_logits, logits, argmax; the json holds the share of the reference's pixels inside the margin band, which must
    be at most ``cases.MAX_BAND_SHARE`` (otherwise pick another weight seed)."""
    from label_anything.models.build_lam import _build_lam
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.weights import init_state_dict
    cfg = case["cfg"]
    spec = cfg.encoder_spec
    vit = PatchGrid(hf_model(spec, cfg.image_size), spec.prefix_tokens)
    lam = _build_lam(build_vit=(lambda project_last_hidden=True: vit), use_vit=True, use_vit_sam_neck=cfg.use_vit_sam_neck,
                     image_embed_dim=cfg.image_embed_dim, embed_dim=cfg.embed_dim, image_size=cfg.image_size, vit_patch_size=cfg.vit_patch_size,
                     class_attention=cfg.class_attention, example_attention=cfg.example_attention,
                     example_class_attention=cfg.example_class_attention, spatial_convs=cfg.spatial_convs,
                     class_encoder=dict(cfg.class_encoder) if cfg.class_encoder else None, custom_preprocess=cfg.custom_preprocess)
    lam.eval()
    sd = init_state_dict(cfg, case["weight_seed"])
    load_encoder(vit.model, sd, spell)
    res = lam.load_state_dict({k: v for k, v in sd.items() if not k.startswith("image_encoder.")}, strict=False)
    assert all(k.startswith("image_encoder.") for k in res.missing_keys) and not res.unexpected_keys, res
    batch = make_episode(**case["episode"])
    rows = fixed_rows(lam, case, batch["flag_examples"].shape[2])
    with torch.no_grad():
        seg_low, _ = lam._forward(batch)
        ref = lam(batch)
    share = band_share(ref["logits"], cases.MARGIN)
    assert share <= cases.MAX_BAND_SHARE, f"{name}: {share:.3%} of the reference's pixels lie inside the margin band; pick another weight seed"
    assert bool(torch.isfinite(seg_low).all())
    meta = {"case": name, "weight_seed": case["weight_seed"], "episode": case["episode"], "margin": cases.MARGIN, "margin_band_share": share,
            "low_res_scale": float(seg_low.abs().max())}
    size = write_fixture(f"{family}_{name}", logit_tensors(seg_low, ref), meta, rows)
    print(f"[{name}] bytes {size} band share {share:.4f} low-res scale {meta['low_res_scale']:.3f}")


def encoder_family_main(family, cases, hf_model, spell=None):
    """The command line of an encoder family's generator: its ENCODER_CASES, then its MODEL_CASES."""
    def forward(name, case):
        (encoder_fixture if name in cases.ENCODER_CASES else encoder_model_fixture)(family, cases, hf_model, spell, name, case)

    main({**cases.ENCODER_CASES, **cases.MODEL_CASES}, forward)


def main(cases, forward, trains=()):
    """The generators' command line: ``forward(name, case)`` for every case of the table, then every (case name, function) of ``trains``."""
    global WRITE
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="this case alone")
    ap.add_argument("--full", action="store_true", help="also run the cases marked slow")
    ap.add_argument("--no-train", action="store_true", help="skip the training steps")
    ap.add_argument("--no-write", action="store_true", help="run every check, write nothing")
    a = ap.parse_args()
    WRITE = not a.no_write
    torch.manual_seed(0)
    for name, case in cases.items():
        if a.only in (None, name) and (a.full or a.only == name or not case.get("slow")):
            forward(name, case)
    for name, train in trains:
        if not a.no_train and a.only in (None, name):
            train()
