"""What the encoder-family benchmarks (tools/bench_dinov2.py, tools/bench_dinov3.py) share: seeded batches, the alternating forward
windows of a set of ``ImageEncoder``s, and the command line that prints and writes one JSON line per measurement.

The variants' windows alternate in ONE process, so that all see the same clocks and neighbours; every figure is the median of --repeats
windows of --iters calls after a warm-up, with the min - max spread beside it.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch                                        # noqa: E402

from tools.bench_multi_embedding import alternate, stats   # noqa: E402,F401  (re-exported to the family scripts)


def batch(images, side, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(images, 3, side, side, generator=g).cuda()


def forwards(which, iters, repeats):
    """which: label -> (encoder name, batch).  -> (label -> ImageEncoder, label -> window times): seeded weights, one warm-up call each."""
    from labelanything_amd.models import ImageEncoder
    encs = {k: ImageEncoder(name, image_size=x.shape[-1], seed=3).cuda() for k, (name, x) in which.items()}
    fns = {k: (lambda e=encs[k], x=which[k][1]: e(x)) for k in which}
    for fn in fns.values():
        fn()
    return encs, alternate(fns, iters, repeats)


def main(tool, out, records):
    """The family scripts' command line.  ``records(images, iters, repeats)`` yields one record per measurement; each is printed as it
    comes and all go to --out (default profiles/<out>), behind a line that says where they were taken."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} needs an MI355X: there is nothing to measure on the CPU")
    lines = [{"what": "box", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": a.iters, "repeats": a.repeats}]
    print(json.dumps(lines[0]), flush=True)
    for rec in records(a.images, a.iters, a.repeats):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
