#!/usr/bin/env python
"""Query substitution on the MI355X: (1) the error-point sampler alone (la_error_count + la_error_points, device draws) against the
reference's torch sequence restated on the device (one-hot ground truth and prediction, torch.nonzero, torch.unique over (b, c),
one torch.randint per class, gather), at training shapes; (2) one substitution batch (M+2 steps) of decoder-only cfg3-style training
from embeddings through ``LamTrainer.substitution_steps``, next to M+2 plain ``step`` calls on the same batch.

Reports us per sampler call, host synchronisations per sampler call (torch's sync debug mode counts the synchronising calls), and ms
per substitution batch.  One JSON line per measurement on stdout.

    python tools/substitution_bench.py [--iters 50] [--batches 2]
"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                        # noqa: E402
import torch.nn.functional as F                     # noqa: E402

from labelanything_amd.substitution import Substitutor, generate_points_from_errors   # noqa: E402


def torch_sequence(pred, gt, n, ignore_index=-100):
    """The reference's sampler as a sequence of torch ops on the device (experiment/substitution.py:17-97): the part whose cost the
    kernels replace - everything up to the sampled coordinates and labels, without its host-side bookkeeping of absent classes."""
    B, C = pred.shape[:2]
    g = gt.clone()
    g[g == ignore_index] = 0
    err = F.one_hot(g, C).permute(0, 3, 1, 2) - F.one_hot(pred.argmax(1), C).permute(0, 3, 1, 2)
    coords = torch.nonzero(err)
    cls, counts = torch.unique(coords[:, :2], dim=0, return_counts=True, sorted=True)
    idx = torch.cat([torch.randint(0, int(x), (n,), device=pred.device) for x in counts.tolist()])
    idx = idx + torch.cat([counts.new_zeros(1), counts.cumsum(0)])[:-1].repeat_interleave(n)
    pts = coords[idx]
    labels = err[pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3]]
    return pts[:, [0, 1, 3, 2]], labels, cls


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


def count_syncs(fn):
    """(number of synchronising calls torch's sync debug mode reports during fn(), where they came from)."""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    hits = [x for x in w if "synchroniz" in str(x.message).lower()]
    return len(hits), sorted({f"{os.path.basename(x.filename)}:{x.lineno}: {str(x.message)[:80]}" for x in hits})


def sampler(args):
    shapes = [(2, 6, 480, 480), (16, 6, 480, 480), (8, 4, 1024, 1024), (16, 6, 1024, 1024), (16, 3, 427, 640), (16, 6, 612, 640)]
    gen = torch.Generator(device="cuda").manual_seed(0)
    for B, C, H, W in shapes:
        g = torch.Generator(device="cuda").manual_seed(B * C + H)
        gt = torch.randint(0, C, (B, H, W), device="cuda", generator=g)
        gt[:, H * 3 // 4:] = -100                          # COCO-style ragged frames: padding of the batch's largest image
        logits = torch.randn(B, C, H, W, device="cuda", generator=g)
        logits.scatter_add_(1, gt.clamp(min=0).unsqueeze(1), torch.full((B, 1, H, W), 1.0, device="cuda"))
        dims = torch.tensor([[H, W]] * B, device="cuda")
        preds = torch.empty(B, H, W, dtype=torch.int64, device="cuda")
        ours = lambda: generate_points_from_errors(logits, gt, 1, generator=gen, dims=dims, preds_out=preds)   # noqa: E731
        ref = lambda: torch_sequence(logits, gt, 1)                                                           # noqa: E731
        row = dict(what="sampler", B=B, C=C, H=H, W=W, num_points=1,
                   hip_us=round(timed(ours, args.iters), 1), torch_us=round(timed(ref, max(3, args.iters // 5)), 1),
                   logits_mb=round(logits.numel() * 4 / 2**20, 1))
        # two counted calls each: the first counted call of the process was the one that ever reported a sync (see profiles/README.md)
        for tag, fn in (("hip", ours), ("torch", ref)):
            (n1, src1), (n2, _) = count_syncs(fn), count_syncs(fn)
            row[f"{tag}_syncs"] = n2
            row[f"{tag}_syncs_first_call"] = n1
            if tag == "hip" and n1:
                row["hip_first_call_sync_source"] = src1
        row["speedup"] = round(row["torch_us"] / row["hip_us"], 1)
        print(json.dumps(row), flush=True)


def training(args):
    from labelanything_amd.config import LamConfig
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    from labelanything_amd.train import LamTrainer
    cfg = LamConfig(encoder=None, use_vit=False, image_size=480, image_embed_dim=768, embed_dim=256, spatial_convs=3,
                    class_encoder={"name": "RandomMatrixEncoder", "bank_size": 100, "embed_dim": 256}, custom_preprocess=False)
    ep = make_episode(batch=2, n_ways=5, k_shots=5, image_size=480, seed=1, prompts=("mask", "point", "box"), embeddings_channels=768,
                      grid=30)
    batch = dict(ep)
    for k in ("prompt_points", "flag_points", "prompt_bboxes", "flag_bboxes", "prompt_masks", "flag_masks", "flag_examples"):
        batch[k] = torch.cat([ep[k][:, :1], ep[k]], dim=1)            # the dataset's layout: prompts for the query too
    b, m1 = batch["dims"].shape[:2]
    c = batch["flag_examples"].shape[2]
    g = torch.Generator().manual_seed(2)
    gts = torch.randint(0, c, (b, m1, 30, 30), generator=g).repeat_interleave(16, 2).repeat_interleave(16, 3).contiguous()
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    gts = gts.cuda()
    lam = Lam(cfg, seed=3).cuda()
    lam.selected_rows = torch.arange(c)
    tr = LamTrainer(lam, lr=1e-5)
    sub = Substitutor(num_points=1, long_side_length=480, custom_preprocess=False,
                      generator=torch.Generator(device="cuda").manual_seed(4))
    plain_inp, plain_gt = Substitutor(substitute=False), None
    plain_inp.reset(batch=(batch, gts))
    plain_inp, plain_gt = next(plain_inp)

    def one_batch():
        for _ in tr.substitution_steps(batch, gts, sub):
            pass

    def plain():
        for _ in range(m1 + 1):
            tr.step(plain_inp, plain_gt)

    for fn, name in ((one_batch, "substitution_batch"), (plain, "plain_steps")):
        fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.batches):
            fn()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / args.batches
        print(json.dumps(dict(what=name, episodes=b, images=m1, steps=m1 + 1, ms_per_batch=round(ms, 1),
                              ms_per_step=round(ms / (m1 + 1), 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--skip-training", action="store_true")
    args = ap.parse_args()
    p = torch.cuda.get_device_properties(0)
    print(json.dumps(dict(what="box", device=torch.cuda.get_device_name(0), arch=getattr(p, "gcnArchName", ""), cus=p.multi_processor_count,
                          torch=torch.__version__, hip=torch.version.hip)), flush=True)
    sampler(args)
    if not args.skip_training:
        training(args)


if __name__ == "__main__":
    main()
