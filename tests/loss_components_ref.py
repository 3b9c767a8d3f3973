"""fp64 torch restatement of the reference's LabelAnythingLoss components (loss/__init__.py, focal.py, dice.py, fp.py, prompt.py,
utils.py), written from their formulas: the checker of tools/make_golden_loss_components.py (against the reference itself), of the
CPU / GPU tests (against the committed fixtures and the device kernels) and the eager comparison of tools/loss_components_bench.py.
Autograd gives the gradients.  Every function works on any device."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F

from labelanything_amd.config import LamConfig

IGNORE = -100
LOGITS = ("focal", "dice", "fp")
NAMES = ("focal", "dice", "fp", "prompt_contrastive")       # order of the fixtures' component vectors
# parameters/trainval/other/1_NewTraining.yaml, 2_NewTraining.yaml: loss section
CASE_A = {"focal": {"weight": 0.725}, "dice": {"weight": 0.025}, "prompt_contrastive": {"weight": 0.25}}

# training fixture (tests/golden/train_loss_components.safetensors): a reduced decoder-only model (precomputed embeddings) with the
# class / example attention of the NewTraining configs, three AdamW steps with CASE_A's loss
TRAIN_LC_CASE = dict(
    cfg=LamConfig(encoder=None, use_vit=False, image_size=128, image_embed_dim=96, embed_dim=64, spatial_convs=3, class_attention=True,
                  example_attention=True, class_encoder={"name": "RandomMatrixEncoder", "bank_size": 10, "embed_dim": 64},
                  custom_preprocess=True),
    weight_seed=23,
    episode=dict(batch=2, n_ways=2, k_shots=2, image_size=128, seed=123, prompts=("mask", "point", "box"),
                 embeddings_channels=96, grid=8, dims=[[100, 128]] * 5),
    lr=1e-3, weight_decay=1e-2, steps=3, warmup=2, gt_seed=15,
)


def class_weights(target: torch.Tensor, c: int, weighting: bool) -> torch.Tensor:
    """1 / log(1.1 + count_c / (B*H*W)) for the classes present (ignored pixels count in the denominator), 1 for the others."""
    w = torch.ones(c, dtype=torch.float64, device=target.device)
    if weighting:
        cnt = torch.stack([(target == k).sum() for k in range(c)]).double()
        w = torch.where(cnt > 0, 1.0 / torch.log(1.1 + cnt / target.numel()), w)
    return w


def focal(x: torch.Tensor, t: torch.Tensor, gamma: float, cw: torch.Tensor) -> torch.Tensor:
    valid = t != IGNORE
    tt = torch.where(valid, t, torch.zeros_like(t))
    logp = torch.log_softmax(x.double(), 1).gather(1, tt[:, None]).squeeze(1)
    ce = torch.where(valid, -logp, torch.zeros_like(logp))
    pt = torch.exp(-ce)
    return ((1 - pt) ** gamma * cw[tt] * ce).mean()


def _onehot(t: torch.Tensor, c: int) -> torch.Tensor:
    return (t[:, None] == torch.arange(c, device=t.device)[None, :, None, None]).double()


def dice(x: torch.Tensor, t: torch.Tensor, cw: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    p = torch.softmax(x.double(), 1)
    oh = _onehot(t, x.shape[1])                       # ignored pixels match no class
    inter = (p * oh).sum((2, 3))
    union = p.sum((2, 3)) + oh.sum((2, 3))            # every pixel's p, ignored and padded ones included
    return ((1 - (2 * inter + eps) / (union + eps)) * cw).mean(1).mean()


def false_positive(x: torch.Tensor, t: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    valid = t != IGNORE
    tz = torch.where(valid, t, torch.zeros_like(t))   # ignored targets read as class 0: background is then present
    absent = 1 - _onehot(tz, x.shape[1]).amax((2, 3))
    p = torch.softmax(x.double(), 1)
    per = (p * absent[:, :, None, None]).sum(1) / (absent.sum(1) + eps)[:, None, None]
    return (per * valid).sum() / valid.sum()


def prompt_contrastive(emb: torch.Tensor, flags: torch.Tensor, t_prime: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    b, m, c, d = emb.shape
    e = F.normalize(emb.double().reshape(b, m * c, d), p=2, dim=-1, eps=1e-12)
    z = e @ e.transpose(1, 2) * torch.exp(t_prime.double()) + bias.double()
    cls = torch.arange(m * c, device=emb.device) % c
    y = torch.where(cls[:, None] == cls[None, :], 1.0, -1.0).double()
    loss = F.softplus(-y * z)
    f = flags.reshape(b, m * c) != 0
    pair = torch.triu(f[:, :, None] & f[:, None, :], diagonal=1)
    valid = f.sum(1)
    total = emb.new_zeros((), dtype=torch.float64)
    for i in range(b):
        if int(valid[i]) > 0:
            total = total + loss[i][pair[i]].sum() / valid[i]
    return total / b


def prompt_contrastive_pairs(emb: torch.Tensor, flags: torch.Tensor, t_prime: torch.Tensor, bias: torch.Tensor, y: Optional[torch.Tensor] = None):
    """The per-pair breakdown of ``prompt_contrastive``: -> {"positive", "negative"} the two parts of the loss (their sum is the loss:
    the pairs with y = +1 and with y = -1), {"u"} = -y z of every counted pair (i < j, both flagged, any image) and {"y"} of those
    pairs.  ``y`` [n, n] replaces the class rule (tests/loss_profiles.py: a wrong pair label must show)."""
    b, m, c, d = emb.shape
    e = F.normalize(emb.double().reshape(b, m * c, d), p=2, dim=-1, eps=1e-12)
    z = e @ e.transpose(1, 2) * torch.exp(t_prime.double()) + bias.double()
    if y is None:
        cls = torch.arange(m * c, device=emb.device) % c
        y = torch.where(cls[:, None] == cls[None, :], 1.0, -1.0).double()
    y = y.double().to(emb.device)
    u = -y * z
    loss = F.softplus(u)
    f = flags.reshape(b, m * c) != 0
    pair = torch.triu(f[:, :, None] & f[:, None, :], diagonal=1)
    valid = f.sum(1).clamp_min(1).double()                      # an image without a flag has no pair: its divisor is never used
    per = loss * pair / valid[:, None, None] / b
    return {"positive": (per * (y > 0)).sum(), "negative": (per * (y < 0)).sum(), "u": u[pair], "y": y.expand_as(u)[pair]}


def objective(components: Dict[str, Dict], class_weighting, logits: torch.Tensor, target: torch.Tensor,
              emb: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None, t_prime: Optional[torch.Tensor] = None,
              bias: Optional[torch.Tensor] = None):
    """-> (value, {name: reported value}) with the reference's bookkeeping: a logits component adds w^2 L and reports w L, a prompt
    component adds w L and reports L."""
    cw = class_weights(target, logits.shape[1], bool(class_weighting))
    value, comps = None, {}
    for k, kw in components.items():
        w = float(kw["weight"])
        if k == "focal":
            l = focal(logits, target, float(kw.get("gamma", 2.0)), cw)
        elif k == "dice":
            l = dice(logits, target, cw)
        elif k == "fp":
            l = false_positive(logits, target)
        elif k == "prompt_contrastive":
            if t_prime is None:
                t_prime = torch.tensor([math.log(10.0)], dtype=torch.float64, device=logits.device)
            if bias is None:
                bias = torch.tensor([-10.0], dtype=torch.float64, device=logits.device)
            l = prompt_contrastive(emb, flags, t_prime, bias)
        else:
            raise ValueError(k)
        if k in LOGITS:
            comps[k], add = w * l, w * w * l
        else:
            comps[k], add = l, w * l
        value = add if value is None else value + add
    return value, comps
