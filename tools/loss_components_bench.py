#!/usr/bin/env python
"""Loss components on the MI355X: device time of (1) la_focal_loss alone, (2) la_logits_objective with focal + dice, (3) focal +
dice + fp + prompt_contrastive (la_logits_objective + la_prompt_contrastive), each value + gradient, next to the same math as an eager
fp32 torch sequence on the device (tests/loss_components_ref.py evaluated in fp32, forward + autograd backward).  Also the bytes the
logits objective must move (logits read twice, target three times, dlogits written once) over its kernel time, as a fraction of HBM
peak.  One JSON line per shape is printed; the box line and every shape's line are written to --out (default
profiles/loss_components_bench.jsonl, overwritten).

    python tools/loss_components_bench.py [--iters 50]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                        # noqa: E402

from labelanything_amd import _lib as L             # noqa: E402
from tests import loss_components_ref as R         # noqa: E402

SHAPES = [(2, 2, 1024, 1024), (8, 6, 480, 480), (4, 21, 512, 512)]
HBM_PEAK = 8.0e12                                   # MI355X HBM3E, bytes / s
M, D = 2, 256                                       # class-example rows per class and their width for prompt_contrastive
FULL = {"focal": {"weight": 0.725}, "dice": {"weight": 0.025}, "fp": {"weight": 0.1}, "prompt_contrastive": {"weight": 0.25}}


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def eager(x, t, e, f, tp, bs, comps):
    """The restatement in fp32 on the device: forward + backward through torch autograd."""
    xx = x.detach().requires_grad_(True)
    ee = e.detach().requires_grad_(True)
    cw = R.class_weights(t, x.shape[1], True).float()
    tot = 0.0
    if "focal" in comps:
        valid = t != R.IGNORE
        tt = torch.where(valid, t, torch.zeros_like(t))
        logp = torch.log_softmax(xx, 1).gather(1, tt[:, None]).squeeze(1)
        ce = torch.where(valid, -logp, torch.zeros_like(logp))
        pt = torch.exp(-ce)
        tot = tot + 0.725 ** 2 * ((1 - pt) ** 2 * cw[tt] * ce).mean()
    if "dice" in comps:
        p = torch.softmax(xx, 1)
        oh = (t[:, None] == torch.arange(x.shape[1], device=x.device)[None, :, None, None]).float()
        inter, union = (p * oh).sum((2, 3)), p.sum((2, 3)) + oh.sum((2, 3))
        tot = tot + 0.025 ** 2 * ((1 - (2 * inter + 1e-6) / (union + 1e-6)) * cw).mean(1).mean()
    if "fp" in comps:
        valid = t != R.IGNORE
        tz = torch.where(valid, t, torch.zeros_like(t))
        absent = 1 - (tz[:, None] == torch.arange(x.shape[1], device=x.device)[None, :, None, None]).float().amax((2, 3))
        p = torch.softmax(xx, 1)
        per = (p * absent[:, :, None, None]).sum(1) / (absent.sum(1) + 1e-6)[:, None, None]
        tot = tot + 0.1 ** 2 * (per * valid).sum() / valid.sum()
    if "prompt_contrastive" in comps:
        b, m, c, d = ee.shape
        en = torch.nn.functional.normalize(ee.reshape(b, m * c, d), dim=-1)
        z = en @ en.transpose(1, 2) * torch.exp(tp) + bs
        cls = torch.arange(m * c, device=x.device) % c
        y = torch.where(cls[:, None] == cls[None, :], 1.0, -1.0)
        fl = f.reshape(b, m * c) != 0
        pair = torch.triu(fl[:, :, None] & fl[:, None, :], diagonal=1)
        tot = tot + 0.25 * (torch.nn.functional.softplus(-y * z) * pair / fl.sum(1)[:, None, None]).sum() / b
    tot.backward()
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_components_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    lines = [{"box": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip, "iters": args.iters,
              "hbm_peak_bytes_per_s": HBM_PEAK}]
    for (b, c, h, w) in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(c)
        x = torch.randn(b, c, h, w, device=dev, generator=g) * 4
        t = torch.randint(0, c, (b, h, w), device=dev, generator=g)
        t[torch.rand(b, h, w, device=dev, generator=g) < 0.05] = -100
        e = torch.randn(b, M, c, D, device=dev, generator=g)
        f = torch.ones(b, M, c, dtype=torch.uint8, device=dev)
        tp = torch.tensor([math.log(10.0)], device=dev)
        bs = torch.tensor([-10.0], device=dev)
        hw = h * w
        loss, dl, cw = torch.empty(1, device=dev), torch.empty_like(x), torch.empty(c, device=dev)
        fscratch = torch.empty((c + 2) + 2048, device=dev, dtype=torch.int64)
        val, comps = torch.empty(1, device=dev), torch.empty(3, device=dev)
        ws = torch.empty(L.logits_objective_workspace_bytes(b, c, hw), dtype=torch.uint8, device=dev)
        e2 = e.reshape(b, M * c, D)
        pl, de, dt, db = torch.empty(1, device=dev), torch.empty_like(e2), torch.empty(1, device=dev), torch.empty(1, device=dev)
        pws = torch.empty(L.prompt_contrastive_workspace_bytes(b, M * c, D), dtype=torch.uint8, device=dev)

        def focal():
            L.focal_loss(x, t, 2.0, True, 0.725 ** 2, -100, loss, dl, cw, fscratch)

        def focal_dice():
            L.logits_objective(x, t, -100, 3, 0.725, 2.0, 0.025, 0.0, True, val, comps, dl, None, ws)

        def full():
            L.logits_objective(x, t, -100, 7, 0.725, 2.0, 0.025, 0.1, True, val, comps, dl, None, ws)
            L.prompt_contrastive(e2, f, c, tp, bs, pl, de, dt, db, pws)

        us_f, us_fd, us_full = timed(focal, args.iters), timed(focal_dice, args.iters), timed(full, args.iters)
        us_eager_fd = timed(lambda: eager(x, t, e, f, tp, bs, ("focal", "dice")), max(5, args.iters // 5))
        us_eager_full = timed(lambda: eager(x, t, e, f, tp, bs, tuple(FULL)), max(5, args.iters // 5))
        nbytes = 2 * x.numel() * 4 + 3 * t.numel() * 8 + x.numel() * 4
        line = {"shape": [b, c, h, w], "us_focal": round(us_f, 1), "us_focal_dice": round(us_fd, 1),
                "us_focal_dice_fp_prompt": round(us_full, 1), "us_eager_focal_dice": round(us_eager_fd, 1),
                "us_eager_focal_dice_fp_prompt": round(us_eager_full, 1), "composite_over_focal": round(us_full / us_f, 2),
                "speedup_vs_eager": round(us_eager_full / us_full, 2), "traffic_bytes": nbytes,
                "hbm_fraction_focal_dice": round(nbytes / (us_fd * 1e-6) / HBM_PEAK, 3),
                "hbm_fraction_full": round(nbytes / (us_full * 1e-6) / HBM_PEAK, 3), "prompt_rows": M * c, "prompt_dim": D}
        lines.append(line)
        print(json.dumps(line), flush=True)
        del x, t, e, dl, ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        for ln in lines:
            fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
