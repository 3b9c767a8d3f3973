#!/usr/bin/env python
"""``conv_classification`` at the geometry of parameters/trainval/pascal/mae_nodown.yaml on the MI355X: 480 px, 30 x 30 grid, D = 256,
``classification_layer_downsample_rate=1`` (a 120 x 120 x 256 feature map per episode), 8 episodes, 1-way and 2-way 1-shot (C = 2 and 3
with the background).  Device time of

  proto_kernels      la_proto_kernels (prototypes -> 5 x 5 kernels);
  classify_conv      la_classify_conv (the 5 x 5 correlation per episode);
  pair               both - what the engine runs in place of la_classify;
  torch_pair         the same two steps in stock PyTorch eager fp32 on the same GPU: 2 x F.conv_transpose2d, then F.conv2d(padding=2) per
                     episode on the NCHW map (the reference's op sequence, mask_decoder.py:303-307);
  classify_conv_bwd  la_classify_conv_bwd;  proto_kernels_bwd  la_proto_kernels_bwd,

measured in ONE process with the variants' windows interleaved, and ``Lam.forward`` episodes/s from precomputed 768-channel embeddings for
the recipe's model section with the head on and off.  There is no parent commit to compare with: the feature is new.  Every figure is the
median of --repeats windows of --iters launches after a warm-up, with the min - max spread beside it.  The model of la_classify_conv: the
feature map (4 H W cf bytes per episode) read once per class pair, 25 cf C multiply-adds per pixel on the exact-fp32 MFMA.  One JSON line
per measurement goes to --out.

    python tools/bench_convcls.py [--iters 20] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                                        # noqa: E402
import torch.nn.functional as F                     # noqa: E402

from labelanything_amd import _lib as L             # noqa: E402

HBM_PEAK = 8.0e12
F32_MFMA_PEAK = 157.3e12                            # dense fp32 matrix FLOP/s of the MI355X data sheet
EPISODES = 8
RECIPE = dict(image_size=480, image_embed_dim=768, embed_dim=256, spatial_convs=3, class_attention=False, example_attention=False,
              example_class_attention=True, class_encoder={"name": "RandomMatrixEncoder", "bank_size": 100, "embed_dim": 256})


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters        # us per call


def alternate(fns, iters, repeats, warm=3):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return out


def stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "windows": len(us)}


def bench_kernels(c, iters, repeats, b=EPISODES, side=120, cf=256):
    gen = torch.Generator().manual_seed(7)
    feat = torch.randn(b, side, side, cf, generator=gen).cuda()
    nchw = feat.permute(0, 3, 1, 2).contiguous()
    protos = torch.randn(b * c, cf, generator=gen).cuda()
    w1, w2 = ((torch.randn(cf, cf, 3, 3, generator=gen) / (9 * cf) ** 0.5).cuda() for _ in range(2))
    k1 = torch.empty(b * c, cf, 3, 3, device="cuda")
    kern = torch.empty(b, c, 25, cf, device="cuda")
    seg = torch.empty(b, c, side, side, device="cuda")
    dseg = torch.randn(b, c, side, side, generator=gen).cuda()
    dfeat, dkern = torch.empty_like(feat), torch.empty_like(kern)
    dk1, de = torch.empty_like(k1), torch.empty_like(protos)
    dw1, dw2 = torch.zeros_like(w1), torch.zeros_like(w2)
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False

    def torch_pair():
        k = F.conv_transpose2d(F.conv_transpose2d(protos.view(b * c, cf, 1, 1), w1), w2).view(b, c, cf, 5, 5)
        return torch.cat([F.conv2d(nchw[i:i + 1], k[i], padding=2) for i in range(b)])

    L.proto_kernels(protos, w1, w2, b * c, cf, k1, kern)
    L.classify_conv(feat, kern, b, c, side, side, cf, seg)
    agree = float((seg - torch_pair()).abs().max() / seg.abs().max())
    fns = {
        "proto_kernels": lambda: L.proto_kernels(protos, w1, w2, b * c, cf, k1, kern),
        "classify_conv": lambda: L.classify_conv(feat, kern, b, c, side, side, cf, seg),
        "pair": lambda: (L.proto_kernels(protos, w1, w2, b * c, cf, k1, kern), L.classify_conv(feat, kern, b, c, side, side, cf, seg)),
        "torch_pair": torch_pair,
        "classify_conv_bwd": lambda: L.classify_conv_bwd(dseg, feat, kern, b, c, side, side, cf, dfeat, dkern),
        "proto_kernels_bwd": lambda: L.proto_kernels_bwd(dkern, protos, k1, w1, w2, b * c, cf, dk1, de, dw1, dw2),
    }
    t = alternate(fns, iters, repeats)
    med = statistics.median(t["classify_conv"])
    rd = 4 * b * side * side * cf * ((c + 1) // 2)          # once per class group (a pair, or the odd last class)
    macs = 25 * cf * c * b * side * side
    # issued MFMA work over useful: 16 x 16 halo pixels per 12 x 12 outputs, 64 columns per class pair + 32 for an odd last class
    halo = (16 * 16) / (12 * 12) * (64 * (c // 2) + 32 * (c % 2)) / (25 * c)
    return {"what": "kernels", "episodes": b, "classes": c, "map": [side, side, cf], **{k: stats(v) for k, v in t.items()},
            "agreement_with_torch_rel": agree, "torch_pair_over_pair": round(statistics.median(t["torch_pair"]) / statistics.median(t["pair"]), 3),
            "classify_conv_bytes_read": rd, "classify_conv_fraction_of_hbm_peak": round(rd / (med * 1e-6) / HBM_PEAK, 4),
            "classify_conv_useful_macs": macs, "classify_conv_issued_over_useful_macs": round(halo, 3),
            "classify_conv_fraction_of_fp32_mfma_peak_useful": round(2 * macs / (med * 1e-6) / F32_MFMA_PEAK, 4),
            "classify_conv_fraction_of_fp32_mfma_peak_issued": round(2 * macs * halo / (med * 1e-6) / F32_MFMA_PEAK, 4)}


def bench_forward(n_ways, iters, repeats):
    from labelanything_amd.config import config_from_kwargs
    from labelanything_amd.episodes import make_episode
    from labelanything_amd.models import Lam
    batch = make_episode(batch=EPISODES, n_ways=n_ways, k_shots=1, image_size=480, seed=11, prompts=("mask",), embeddings_channels=768, grid=30)
    fns = {}
    for tag, kw in (("recipe", dict(classification_layer_downsample_rate=1, conv_classification=True)),
                    ("nodown_plain", dict(classification_layer_downsample_rate=1)), ("default", {})):
        lam = Lam(config_from_kwargs(encoder=None, use_vit=False, **RECIPE, **kw), seed=3).cuda()
        lam.selected_rows = torch.arange(n_ways + 1)
        lam.use_graphs = True
        fns[tag] = (lambda lam=lam: lam.forward_argmax(batch))
    t = alternate(fns, iters, repeats)
    return {"what": "forward", "episodes": EPISODES, "n_ways": n_ways, **{k: stats(v) for k, v in t.items()},
            "episodes_per_s": {k: round(EPISODES / (statistics.median(v) * 1e-6), 1) for k, v in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convcls_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_convcls needs an MI355X: there is nothing to measure on the CPU")
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats}]
    for c in (2, 3):
        lines.append(bench_kernels(c, a.iters, a.repeats))
        print(json.dumps(lines[-1]), flush=True)
    if not a.no_forward:
        for n_ways in (1, 2):
            lines.append(bench_forward(n_ways, max(a.iters // 4, 3), a.repeats))
            print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
