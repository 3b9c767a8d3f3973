"""What the encoder-family test modules (tests/test_dinov2_model_gpu.py, tests/test_dinov3_model_gpu.py) check in the same way, beside
tests/model_checks.py: a fixture case on the driver the engine chooses, the fold case on the plain driver, the tiny encoder inside a
model.  Plain functions of the family's fixture prefix ("dinov2", "dinov3") and its case tables; a module keeps the tests of its own
kernels and its CLI test.

Bounds: 1e-3 max-norm, the project's stage bound for fp16 encoder stages, on the encoder output of every case and on the model case's
logits; argmax exact outside the family's margin band, whose share of the reference's own pixels the generator recorded (re-asserted from
the json).  The 99.9th percentile of the element-wise relative error is printed beside every max-norm figure.
"""
import os

import numpy as np
import torch
from PIL import Image

from labelanything_amd.episodes import make_episode
from labelanything_amd.models import ImageEncoder
from tests import model_checks as MC
from tests.cases_encoder import encoder_images
from tests.helpers import load_golden, pct_rel_err, rel_err

TOL = 1e-3


def tokens(enc, images):
    return enc(images).flatten(2).transpose(1, 2)            # [images, E, g, g] -> [images, hw, E]


def run_encoder(family, cases, name, norm_fold=True):
    """(patch tokens [images, hw, E] of the case on the device path, the fixture's, the block driver taken)."""
    case = cases[name]
    gold, meta = load_golden(f"{family}_{name}")
    assert meta["weight_seed"] == case["weight_seed"] and meta["image_seed"] == case["image_seed"]
    enc = ImageEncoder(case["encoder"], image_size=case["side"], seed=case["weight_seed"]).cuda()
    enc.lam.norm_fold = norm_fold
    out = tokens(enc, encoder_images(case))
    torch.cuda.synchronize()
    return out, gold["patch_tokens"], enc.lam.engine().last_block_path


def check_encoder_case(family, cases, name):
    """The case on the driver the engine chooses for it, which is asserted."""
    got, ref, path = run_encoder(family, cases, name)
    err, p999 = rel_err(got, ref), pct_rel_err(got, ref)
    print(f"[{family} {name}] path {path}: encoder output max-norm {err:.3e} (bound {TOL:.0e}), 99.9th percentile element-wise {p999:.3e}")
    assert path == cases[name]["path"]
    assert err <= TOL


def check_fold_case_on_the_plain_driver(family, cases):
    """The ViT-B-wide case with the LayerNorm kernels (``norm_fold = False``) - against the fixture, and against the folded driver."""
    got, ref, path = run_encoder(family, cases, "fold", norm_fold=False)
    folded, _, fpath = run_encoder(family, cases, "fold")
    err, p999, between = rel_err(got, ref), pct_rel_err(got, ref), rel_err(got, folded)
    print(f"[{family} fold] path {path}: encoder output max-norm {err:.3e} (bound {TOL:.0e}), 99.9th percentile element-wise {p999:.3e}; "
          f"against the folded driver {between:.3e}")
    assert (path, fpath) == ("plain", "fold")
    assert err <= TOL


def check_model_case(family, model_cases, name, margin, max_band_share):
    """Logits of the model case within the bound, argmax exact outside the margin band, graph replay the eager run's bits."""
    lam, case, gold, meta = MC.load_model(model_cases, name, family + "_")
    batch = make_episode(**case["episode"])
    seg, _ = lam._forward(batch)
    out = lam.forward_argmax(batch)
    torch.cuda.synchronize()
    errs = {"low_res_logits": rel_err(seg, gold["low_res_logits"]), "logits": rel_err(out["logits"], gold["logits"])}
    p999 = pct_rel_err(out["logits"], gold["logits"])
    print(f"[{family} {name}] " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f" (bound {TOL:.0e}), 99.9th percentile "
          f"element-wise {p999:.3e}, encoder path {lam.engine().last_block_path}")
    assert all(v <= TOL for v in errs.values()), errs
    MC.check_argmax(name, out, gold, margin, band_share=(meta, max_band_share))
    MC.check_graph_replay(lam, case)


def write_images(d, sizes):
    """Seeded random PNGs of the given (height, width), named as the CLI's datasets name theirs."""
    rng = np.random.default_rng(0)
    os.makedirs(d, exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, f"{i:012d}.png"))
