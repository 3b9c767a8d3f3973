"""GPU: la_focal_loss, la_logits_objective, la_prompt_contrastive and la_adamw_step, called directly, on the inputs of
tests/loss_profiles.py (checked by tests/test_loss_profiles_cpu.py) against plain fp64 references, per component and per image / row.

Measures: the logits gradient of each component alone (mask 1, 2, 4 of la_logits_objective, and la_focal_loss) per image against that
component's own largest fp64 gradient in the image; for the combined masks against the sum of the parts, relative to the smallest
non-zero part; every entry of ``components`` and the total relatively; the contrastive gradient per row, d t' and d bias relatively;
the AdamW outputs element-wise against the magnitudes they are put together from.  Tolerances: the constant of the fp32 restatement of
the same kernel under the same measure, per (component, profile), times loss_profiles.MARGIN - nothing here is taken from a kernel's
own result.

Shapes: (1, 2, 8, 8) one tile below 256 pixels; (2, 5, 32, 36) the float4 path, two tiles; (2, 6, 33, 35) an odd HW, the scalar path;
(3, 64, 24, 44) C = 64, lane c owns class c; (2049, 2, 2, 2) more images than the 2048-workgroup budget; (2, 5, 32, 36) on views that
start one float into their buffers: the misaligned scalar fallback at HW % 4 == 0.  gamma runs over {0, 1, 1.5, 2, 5}; gamma in (0, 1)
is left out on purpose: there d/dce (1 - pt)^gamma ce is unbounded as pt -> 1, which is where fp32 ce rounds to 0.
"""
import math

import pytest
import torch

from labelanything_amd import _lib as L
from tests import loss_components_ref as R
from tests import loss_profiles as P

pytestmark = pytest.mark.gpu
W = P.WEIGHTS


def _objective(x, t, mask, gamma, cwt, dlogits="new"):
    """la_logits_objective on device tensors -> {"grad", "components", "value"}; dlogits: "new", None (no gradient buffer) or a view"""
    b, c = x.shape[:2]
    hw = x.numel() // (b * c)
    ws = torch.empty(L.logits_objective_workspace_bytes(b, c, hw), dtype=torch.uint8, device="cuda")
    value, comps, cw = torch.empty(1, device="cuda"), torch.empty(3, device="cuda"), torch.empty(c, device="cuda")
    dl = torch.empty_like(x) if isinstance(dlogits, str) else dlogits
    L.logits_objective(x, t, R.IGNORE, mask, W["focal"], gamma, W["dice"], W["fp"], cwt, value, comps, dl, cw, ws)
    return {"grad": dl, "components": comps.tolist(), "value": float(value), "bits": torch.cat([value, comps]).cpu()}


def _focal(x, t, gamma, cwt, dlogits="new"):
    """la_focal_loss with scale = w^2 -> {"grad", "value"}"""
    c = x.shape[1]
    loss, cw = torch.empty(1, device="cuda"), torch.empty(c, device="cuda")
    scratch = torch.empty((c + 2) + 2048, device="cuda", dtype=torch.int64)
    dl = torch.empty_like(x) if isinstance(dlogits, str) else dlogits
    L.focal_loss(x, t, gamma, cwt, W["focal"] * W["focal"], R.IGNORE, loss, dl, cw, scratch)
    return {"grad": dl, "value": float(loss), "bits": loss.cpu()}


def _check_case(shape, profile, pattern, worst, x=None, make_dl=None):
    """Every launch of one (shape, profile, pattern) against its reference; ``worst`` collects figure / tolerance per (kind, component).
    x / make_dl: device logits and a gradient-buffer factory of the caller's (the misaligned views)."""
    xc, tc = P.inputs(shape, profile, pattern)
    x = xc.cuda() if x is None else x
    t = tc.cuda()
    for mask, gamma, cwt in P.runs_for(pattern):
        name = P.MASK_NAME[mask]
        got = _objective(x, t, mask, gamma, cwt, make_dl() if make_dl else "new")
        fig = P.logits_figures(shape, profile, pattern, mask, gamma, cwt, got)
        tag = (shape, profile, pattern, name, gamma, cwt)
        for kind in ("grad", "batch", "value"):
            tol = P.logits_tol(kind, mask, profile, shape)
            worst[(kind, name)] = max(worst.get((kind, name), (0.0, 0.0)), (fig[kind] / tol, fig[kind]))
            assert fig[kind] <= tol, (kind, tag, fig[kind], tol)
        nog = _objective(x, t, mask, gamma, cwt, None)
        assert nog["grad"] is None and torch.equal(nog["bits"], got["bits"]), tag      # (NaN-free: these batches have valid pixels)
        if mask == 1:
            ref = P.reference(shape, profile, pattern, 1, gamma, cwt)
            fl = _focal(x, t, gamma, cwt, make_dl() if make_dl else "new")
            f_grad, f_val = P.image_ratio(fl["grad"], [ref["parts"]["focal"]]), P.rel(fl["value"], ref["value"])
            cross = P.pair_ratio(fl["grad"], got["grad"], ref["parts"]["focal"])
            tol_g, tol_v = P.logits_tol("grad", 1, profile, shape), P.logits_tol("value", 1, profile, shape)
            for key, val, tol in ((("grad", "la_focal_loss"), f_grad, tol_g), (("value", "la_focal_loss"), f_val, tol_v),
                                  (("grad", "focal, the two kernels"), cross, tol_g)):
                worst[key] = max(worst.get(key, (0.0, 0.0)), (val / tol, val))
                assert val <= tol, (key, tag, val, tol)
            assert P.rel(fl["value"], got["value"]) <= tol_v, tag
            assert torch.equal(_focal(x, t, gamma, cwt, None)["bits"], fl["bits"]), tag


def _report(what, worst):
    for (kind, name), (ratio, fig) in sorted(worst.items()):
        print(f"observed {what} | {kind} | {name} | worst figure / tolerance {ratio:.3f} | its figure {fig:.3g}")


CASES = [(s, p) for s in P.MAIN_SHAPES + P.EDGE_SHAPES for p in P.profiles_for(s)]


@pytest.mark.parametrize("shape,profile", CASES, ids=[f"{'x'.join(map(str, s))}-{p}" for s, p in CASES])
def test_logits_kernels_per_component_on_every_profile(shape, profile):
    """la_logits_objective (lo_hist_kernel, lo_dice_sums_kernel, lo_coef_kernel, lo_fused_kernel, lo_fold_kernel) with every mask, and
    la_focal_loss (focal_hist_kernel, focal_fwd_bwd_kernel, focal_fold_kernel): every target pattern of the profile, class weighting on
    and off, every gamma; the two focal kernels against each other; need-grad and no-grad values bit for bit."""
    worst = {}
    for pattern in P.patterns_for(profile, shape):
        _check_case(shape, profile, pattern, worst)
    _report(f"{profile} {shape}", worst)


@pytest.mark.parametrize("profile", ["random", "padded", "offset_1024"])
def test_misaligned_views_take_the_scalar_path_and_stay_inside_their_buffers(profile):
    """la_logits_objective / la_focal_loss at HW % 4 == 0 on logits and dlogits views that start one float into their buffers: the
    launcher falls back to lo_fused_kernel<1> / lo_dice_sums_kernel<1>; the floats before and behind dlogits keep their sentinel."""
    shape = P.MAIN_SHAPES[0]
    n = math.prod(shape)
    xc, _ = P.inputs(shape, profile, "base")
    xbuf = torch.full((n + 8,), math.nan, device="cuda")
    x = xbuf[1:1 + n].view(shape)
    x.copy_(xc)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    bufs = []

    def make_dl():
        buf = torch.full((n + 8,), 12345.0, device="cuda")
        bufs.append(buf)
        return buf[1:1 + n].view(shape)

    worst = {}
    _check_case(shape, profile, "base", worst, x=x, make_dl=make_dl)
    assert len(bufs) >= 18
    for buf in bufs:
        assert float(buf[0]) == 12345.0 and bool((buf[1 + n:] == 12345.0).all()) and bool(torch.isfinite(buf[1:1 + n]).all())
    # one side only misaligned: the aligned dlogits with the misaligned logits, and the other way round
    aligned = _objective(xc.cuda(), P.inputs(shape, profile, "base")[1].cuda(), 7, 2.0, True)
    for xx, dl in ((x, torch.empty(shape, device="cuda")), (xc.cuda(), make_dl())):
        got = _objective(xx, P.inputs(shape, profile, "base")[1].cuda(), 7, 2.0, True, dl)
        fig = P.logits_figures(shape, profile, "base", 7, 2.0, True, got)
        assert fig["grad"] <= P.logits_tol("grad", 7, profile, shape) and fig["value"] <= P.logits_tol("value", 7, profile, shape)
        assert P.pair_ratio(got["grad"], aligned["grad"], sum(P.reference(shape, profile, "base", 7, 2.0, True)["parts"].values())) \
            <= P.logits_tol("batch", 7, profile, shape)
    assert float(bufs[-1][0]) == 12345.0 and bool((bufs[-1][1 + n:] == 12345.0).all())
    _report(f"{profile} {shape} misaligned", worst)


def test_a_fully_ignored_batch_gives_what_the_kernels_document():
    """la_logits_objective / la_focal_loss with no valid pixel: the fp component is 0 / 0 as in the reference (lo_fold_kernel), focal is
    0 with an all-zero gradient, dlogits is finite under every mask, and dice - ignored pixels add their p to U - matches fp64."""
    shape = P.MAIN_SHAPES[0]
    xc, _ = P.inputs(shape, "random", "base")
    tc = torch.full((shape[0],) + shape[2:], R.IGNORE)
    x, t = xc.cuda(), tc.cuda()
    for mask in P.MASK_NAME:
        got = _objective(x, t, mask, 2.0, True)
        assert bool(torch.isfinite(got["grad"]).all()), mask
        assert got["components"][0] == 0.0 and (math.isnan(got["components"][2]) if mask & 4 else got["components"][2] == 0.0), mask
        assert math.isnan(got["value"]) == bool(mask & 4)
    for got in (_objective(x, t, 1, 2.0, True), _focal(x, t, 2.0, True), _objective(x, t, 4, 2.0, True)):
        assert got["value"] == 0.0 or math.isnan(got["value"])
        assert float(got["grad"].abs().max()) == 0.0
    cw = R.class_weights(tc, shape[1], True)
    val, grad = P._grad64(lambda v: R.dice(v, tc, cw), xc)
    got = _objective(x, t, 2, 2.0, True)
    assert P.image_ratio(got["grad"], [grad * W["dice"] ** 2]) <= P.logits_tol("grad", 2, "random", shape)
    assert P.rel(got["components"][1], W["dice"] * val) <= P.logits_tol("value", 2, "random", shape)


EMB_CASES = [(p, s) for p in P.EMB_PROFILES for s in P.EMB_SHAPES]


@pytest.mark.parametrize("profile,mcd", EMB_CASES, ids=[f"{p}-{'x'.join(map(str, s))}" for p, s in EMB_CASES])
def test_prompt_contrastive_per_row_on_every_profile(profile, mcd):
    """la_prompt_contrastive (pc_normalize_kernel, pc_pairs_kernel, pc_fold_kernel): every flag pattern; d emb per row - the rows below
    eps, at zero and just above eps included - unflagged rows exactly 0, the loss, d t' and d bias relatively; nothing is NaN."""
    m, c, d = mcd
    worst = {}
    for fp in P.FLAG_PATTERNS:
        case, ref = P.emb_case(profile, mcd, fp)
        e = case["emb"].cuda().reshape(P.EMB_BATCH, m * c, d).contiguous()
        f = case["flags"].cuda().reshape(P.EMB_BATCH, m * c).contiguous()
        ws = torch.empty(L.prompt_contrastive_workspace_bytes(P.EMB_BATCH, m * c, d), dtype=torch.uint8, device="cuda")
        loss, dt, db = (torch.empty(1, device="cuda") for _ in range(3))
        demb = torch.full_like(e, math.nan)
        L.prompt_contrastive(e, f, c, case["t_prime"].cuda(), case["bias"].cuda(), loss, demb, dt, db, ws)
        got = {"loss": float(loss), "demb": demb.reshape(case["emb"].shape), "dt": float(dt), "db": float(db)}
        assert bool(torch.isfinite(demb).all()) and all(math.isfinite(got[k]) for k in ("loss", "dt", "db")), fp
        if bool((f == 0).any()):
            assert float(demb[f == 0].abs().max()) == 0.0, fp
        for k, v in P.contrastive_figures(ref, got).items():
            tol = P.contrastive_tol(k, profile)
            worst[(k, "contrastive")] = max(worst.get((k, "contrastive"), (0.0, 0.0)), (v / tol, v))
            assert v <= tol, (k, profile, mcd, fp, v, tol)
    _report(f"{profile} {mcd}", worst)


@pytest.mark.parametrize("n", P.ADAMW_N)
def test_adamw_step_against_the_documented_update_order(n):
    """la_adamw_step (adamw_kernel) against the fp64 statement of its update order: one element, both sides of a 256-thread block, and
    4096 * 256 + 3 elements - past the grid cap, into the stride loop; step 1 and 1000, weight decay and gradient scale on and off;
    an all-zero gradient on zero moments moves p by the decay alone."""
    hp = P.ADAMW_HYPER
    worst = {}
    for (_, step, wd, gs) in (c for c in P.adamw_cases() if c[0] == n):
        args = P.adamw_inputs(n)
        dev = [a.cuda() for a in args]
        L.adamw_step(*dev, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, step, gs)
        assert torch.equal(dev[1].cpu(), args[1])                        # the gradient is read only
        fig = P.adamw_ratio({"p": dev[0], "m": dev[2], "v": dev[3]}, P.adamw64(*args, step, wd, gs))
        for k, v in fig.items():
            worst[(k, "adamw")] = max(worst.get((k, "adamw"), (0.0, 0.0)), (v / P.adamw_tol(k), v))
            assert v <= P.adamw_tol(k), (k, n, step, wd, gs, v)
    for wd in (0.0, 0.01):
        args = P.adamw_inputs(n, zero=True)
        dev = [a.cuda() for a in args]
        L.adamw_step(*dev, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], wd, 1, 1.0)
        fig = P.adamw_ratio({"p": dev[0], "m": dev[2], "v": dev[3]}, P.adamw64(*args, 1, wd, 1.0))
        assert float(dev[2].abs().max()) == 0.0 and float(dev[3].abs().max()) == 0.0 and fig["p"] <= P.adamw_tol("p"), (n, wd, fig)
        if wd == 0.0:
            assert torch.equal(dev[0].cpu(), args[0])
    _report(f"adamw n = {n}", worst)
