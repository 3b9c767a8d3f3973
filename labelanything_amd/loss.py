"""Training objective on the device, first link of SURVEY 8f row 1: the focal term of ``LabelAnythingLoss`` with per-batch
class weighting (reference ``loss/__init__.py:67-89``, ``loss/focal.py:17-26``, ``loss/utils.py:17-43``; the training config
``parameters/trainval/coco20i/mae_noembs.yaml:24-28`` uses exactly ``{focal: {weight: 1.0}}`` with ``class_weighting: True``),
fused with its gradient with respect to the logits (``la_focal_loss``): ``train.LamTrainer`` feeds that gradient into the backward of
the decoder (and, with ``train_encoder=True``, of the image encoder)."""
from __future__ import annotations

import math
from typing import Dict

import torch
from torch.autograd import Function

from . import _lib as L


class FocalLossDevice:
    def __init__(self, gamma: float = 2.0, weight: float = 1.0, class_weighting: bool = True, ignore_index: int = -100):
        self.gamma, self.class_weighting, self.ignore_index = float(gamma), bool(class_weighting), int(ignore_index)
        # LabelAnythingLoss.logits_loss multiplies by the component weight twice (loss/__init__.py:77,86)
        self.scale = float(weight) * float(weight)

    def __call__(self, logits: torch.Tensor, target: torch.Tensor, need_grad: bool = True) -> Dict[str, torch.Tensor]:
        """logits fp32 (B, C, H, W) device, target int64 (B, H, W) -> {"loss": fp32 [1], "dlogits": like logits or None,
        "class_weights": fp32 [C]}."""
        if logits.device.type != "cuda" or target.device.type != "cuda":
            raise RuntimeError("FocalLossDevice needs device tensors (there is no CPU path)")
        if (logits.dtype != torch.float32 or target.dtype != torch.int64 or logits.shape[0] != target.shape[0]
                or logits.shape[2:] != target.shape[1:]):
            raise ValueError("expected fp32 logits (B, C, H, W) and int64 target (B, H, W)")
        dev, c = logits.device, logits.shape[1]
        loss = torch.empty(1, device=dev)
        dlog = torch.empty_like(logits) if need_grad else None
        cw = torch.empty(c, device=dev)
        scratch = torch.empty((c + 2) + 2048, device=dev, dtype=torch.int64)
        L.focal_loss(logits.contiguous(), target.contiguous(), self.gamma, self.class_weighting, self.scale, self.ignore_index, loss, dlog, cw,
                     scratch)
        # "bad_targets": labels outside [0, C) that are not ignore_index (torch raises on those; here they are counted on the device and
        # contribute nothing - check it where a host sync is acceptable)
        return {"loss": loss, "dlogits": dlog, "class_weights": cw, "bad_targets": scratch[c + 1]}


# ---------------------------------------------------------------------------------------------------------------------------------
# The whole LabelAnythingLoss (reference loss/__init__.py): a weighted sum of components.  Logits components (focal, dice, fp) run
# as ONE la_logits_objective call (value, per-component values and d/dlogits); prompt_contrastive runs as la_prompt_contrastive.
# ---------------------------------------------------------------------------------------------------------------------------------
LOGITS_COMPONENTS = ("focal", "dice", "fp")
PROMPT_COMPONENTS = ("prompt_contrastive",)
_NOT_BUILT = ("rmi", "emb_contrastive", "masks")
_MASK = {"focal": 1, "dice": 2, "fp": 4}


class _LogitsObjective(Function):
    @staticmethod
    def forward(ctx, logits, target, crit):
        value, comps, dlog = crit._logits_device(logits, target, need_grad=ctx.needs_input_grad[0])
        ctx.mark_non_differentiable(comps)
        ctx.save_for_backward(dlog)
        return value, comps

    @staticmethod
    def backward(ctx, g, _gc):
        (dlog,) = ctx.saved_tensors
        return dlog * g, None, None


class _PromptContrastive(Function):
    @staticmethod
    def forward(ctx, emb, t_prime, bias, flags_u8):
        b, m, c, d = emb.shape
        x = emb.detach().reshape(b, m * c, d).float().contiguous()
        dev = x.device
        loss = torch.empty(1, device=dev)
        demb, dt, db = torch.empty_like(x), torch.empty(1, device=dev), torch.empty(1, device=dev)
        ws = torch.empty(L.prompt_contrastive_workspace_bytes(b, m * c, d), device=dev, dtype=torch.uint8)
        L.prompt_contrastive(x, flags_u8, c, t_prime.detach().float().contiguous(), bias.detach().float().contiguous(), loss, demb, dt, db, ws)
        ctx.save_for_backward(demb, dt, db)
        ctx.shape, ctx.dtype = emb.shape, emb.dtype
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        demb, dt, db = ctx.saved_tensors
        return (demb * g).view(ctx.shape).to(ctx.dtype), (dt * g).reshape(1), (db * g).reshape(1), None


class PromptContrastiveLoss(torch.nn.Module):
    """loss/prompt.py:10-48 on the device: trainable ``t_prime`` (init log 10) and ``bias`` (init -10), both of shape [1]."""

    def __init__(self):
        super().__init__()
        self.t_prime = torch.nn.Parameter(torch.tensor([math.log(10.0)]))
        self.bias = torch.nn.Parameter(torch.tensor([-10.0]))

    def forward(self, result: Dict[str, torch.Tensor]) -> torch.Tensor:
        emb, flags = result["class_examples_embeddings"], result["flag_examples"]
        if emb.device.type != "cuda":
            raise RuntimeError("prompt_contrastive needs device tensors (there is no CPU path)")
        if emb.dim() != 4 or tuple(flags.shape) != tuple(emb.shape[:3]):
            raise ValueError(f"expected class_examples_embeddings [B, M, C, D] and flag_examples [B, M, C], got {tuple(emb.shape)} and "
                             f"{tuple(flags.shape)}")
        if self.t_prime.device != emb.device:
            raise RuntimeError(f"the loss's parameters live on {self.t_prime.device}, the embeddings on {emb.device}: move the loss first")
        flags = flags.to(emb.device, non_blocking=True)
        f8 = flags if flags.dtype == torch.uint8 else flags.ne(0).to(torch.uint8)
        return _PromptContrastive.apply(emb, self.t_prime, self.bias, f8.reshape(emb.shape[0], -1).contiguous())


class LabelAnythingLoss(torch.nn.Module):
    """``LabelAnythingLoss(components, class_weighting)`` of the reference on the device.  components: ``{name: {"weight": w, **kwargs}}``
    with name in focal (``gamma``), dice (``average="macro"``, ``reduction="mean"``), fp, prompt_contrastive.  A logits component
    enters the value as w^2 L and is reported as w L; prompt_contrastive enters as w L and is reported as L (loss/__init__.py:78,87,
    101).  Component values stay device scalars.  ``__call__(result_or_logits, target)``: logits [B, C, H, W] alone, or the model's
    result dict with ``logits``, ``class_examples_embeddings`` and ``flag_examples``."""

    def __init__(self, components: Dict[str, Dict], class_weighting=None):
        super().__init__()
        comps = {k: dict(v) for k, v in components.items()}
        unknown = set(comps) - set(LOGITS_COMPONENTS) - set(PROMPT_COMPONENTS) - set(_NOT_BUILT)
        if unknown:
            raise ValueError(f"Unknown loss components: {unknown}")
        for k in comps:
            if k in _NOT_BUILT:
                raise NotImplementedError(f"loss component {k!r} is not built on the device (focal, dice, fp and prompt_contrastive are)")
        self.weights = {k: float(v.pop("weight")) for k, v in comps.items()}
        self.ignore_index = -100
        self.gamma = 2.0
        for k, kw in comps.items():
            if k == "focal":
                self.gamma = float(kw.pop("gamma", 2.0))
                self._only(k, kw, reduction="mean")
            elif k == "dice":
                self._only(k, kw, reduction="mean", average="macro", ignore_index=-100)
            elif k == "fp":
                self._only(k, kw, ignore_index=-100)
            elif kw:
                raise TypeError(f"{k} takes no arguments, got {sorted(kw)}")
        self.logits_components = [k for k in comps if k in LOGITS_COMPONENTS]
        self.prompt_components = torch.nn.ModuleDict([[k, PromptContrastiveLoss()] for k in comps if k in PROMPT_COMPONENTS])
        self.class_weighting = class_weighting
        self.bad_targets = None       # device count of targets outside [0, C) other than ignore_index after the last call

    @staticmethod
    def _only(name: str, kw: Dict, **allowed) -> None:
        for key, val in kw.items():
            if key not in allowed:
                raise TypeError(f"{name} got an unexpected argument {key!r}")
            if val != allowed[key]:
                raise NotImplementedError(f"{name} with {key}={val!r} is not built on the device (only {key}={allowed[key]!r})")

    def _logits_device(self, logits: torch.Tensor, target: torch.Tensor, need_grad: bool):
        if logits.device.type != "cuda":
            raise RuntimeError("LabelAnythingLoss needs device tensors (there is no CPU path)")
        target = target.to(logits.device, non_blocking=True)
        if target.dtype != torch.int64:
            target = target.long()
        if logits.dim() != 4 or target.shape[0] != logits.shape[0] or target.shape[1:] != logits.shape[2:]:
            raise ValueError(f"expected logits (B, C, H, W) and target (B, H, W), got {tuple(logits.shape)} and {tuple(target.shape)}")
        x = logits.detach().float().contiguous()
        b, c = x.shape[:2]
        hw = x.numel() // (b * c)
        dev = x.device
        value, comps = torch.empty(1, device=dev), torch.empty(3, device=dev)
        dlog = torch.empty_like(x) if need_grad else None
        ws = torch.empty(L.logits_objective_workspace_bytes(b, c, hw), device=dev, dtype=torch.uint8)
        mask = sum(_MASK[k] for k in self.logits_components)
        w = self.weights
        L.logits_objective(x, target.contiguous(), self.ignore_index, mask, w.get("focal", 0.0), self.gamma, w.get("dice", 0.0),
                           w.get("fp", 0.0), bool(self.class_weighting), value, comps, dlog, None, ws)
        self.bad_targets = ws[:b * (c + 2) * 8].view(torch.int64).view(b, c + 2)[:, c + 1].sum()
        if dlog is not None and logits.dtype != torch.float32:
            dlog = dlog.to(logits.dtype)
        return value.reshape(()), comps, dlog

    def logits_loss(self, logits: torch.Tensor, target: torch.Tensor) -> Dict:
        value, comps = _LogitsObjective.apply(logits, target, self)
        return {"value": value, "components": {k: comps[LOGITS_COMPONENTS.index(k)] for k in self.logits_components}}

    def prompt_loss(self, result: Dict) -> Dict:
        value, out = None, {}
        for k, mod in self.prompt_components.items():
            v = mod(result)
            out[k] = v
            value = self.weights[k] * v if value is None else value + self.weights[k] * v
        return {"value": value, "components": out}

    def forward(self, result, target):
        if isinstance(result, torch.Tensor):
            return self.logits_loss(result, target)
        parts = []
        if self.logits_components:
            parts.append(self.logits_loss(result["logits"], target))
        if len(self.prompt_components):
            parts.append(self.prompt_loss(result))
        if not parts:
            raise ValueError("no loss components")
        value = parts[0]["value"] if len(parts) == 1 else parts[0]["value"] + parts[1]["value"]
        return {"value": value, "components": {k: v for p in parts for k, v in p["components"].items()}}
