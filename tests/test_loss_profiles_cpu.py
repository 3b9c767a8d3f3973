"""CPU: the inputs of tests/loss_profiles.py have the properties they are named after, its fp64 references are torch's own in fp64 (and a
literal dice / false-positive written from the formulas at the top of csrc/loss_components.hip), the fp32 restatements give the error
constants that tests/test_loss_conditioning_gpu.py holds the kernels to, and eight deliberately wrong variants of the restatements
exceed those tolerances.  No kernel runs here."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import loss_components_ref as R
from tests import loss_profiles as P


@pytest.mark.parametrize("shape", P.MAIN_SHAPES + P.EDGE_SHAPES)
def test_every_logit_profile_and_target_pattern_has_its_stated_properties(shape):
    for profile in P.profiles_for(shape):
        for pattern in P.patterns_for(profile, shape):
            x, t = P.inputs(shape, profile, pattern)                  # checked inside
            assert x.shape == shape and t.shape == (shape[0],) + shape[2:]
        print(f"profile {profile} {shape}: {P.check_profile(profile, *P.inputs(shape, profile, 'base'))}")
    if shape in P.MAIN_SHAPES:
        for pattern in P.TARGET_PATTERNS:
            print(f"pattern {pattern} {shape}: {P.check_pattern(pattern, P.build_target(pattern, shape), shape[1])}")


def test_check_profile_refuses_randn_and_check_pattern_refuses_the_baseline():
    shape = P.MAIN_SHAPES[0]
    t = P.build_target("base", shape)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(5)) * 4
    for profile in P.LOGIT_PROFILES:
        if profile != "random":
            with pytest.raises(AssertionError):
                P.check_profile(profile, x, t)
    for pattern in P.TARGET_PATTERNS:
        if pattern not in ("base", "all_classes"):                    # (a random target of 1152 pixels holds every class already)
            with pytest.raises(AssertionError):
                P.check_pattern(pattern, t, shape[1])


@pytest.mark.parametrize("mcd", P.EMB_SHAPES)
def test_every_embedding_profile_and_flag_pattern_has_its_stated_properties(mcd):
    for profile in P.EMB_PROFILES:
        for fp in P.FLAG_PATTERNS:
            case, _ = P.emb_case(profile, mcd, fp)                    # checked inside
            print(f"emb {profile} {mcd} {fp}: {P.check_emb_profile(profile, fp, case)}")
    # randn rows without the special rows are refused, and so is one profile under another's name
    m, c, d = mcd
    g = torch.Generator().manual_seed(3)
    plain = {"emb": torch.randn(2, m, c, d, generator=g), "flags": torch.ones(2, m, c, dtype=torch.uint8)}
    for profile, (tp, bs) in P.EMB_PROFILES.items():
        with pytest.raises(AssertionError):
            P.check_emb_profile(profile, "all_on", dict(plain, t_prime=torch.tensor([tp]), bias=torch.tensor([bs])))
    default = P.emb_case("default", mcd, "all_on")[0]
    for profile, (tp, bs) in P.EMB_PROFILES.items():
        if profile != "default":
            with pytest.raises(AssertionError):
                P.check_emb_profile(profile, "all_on", default)
    for fp in P.FLAG_PATTERNS[1:]:
        with pytest.raises(AssertionError):
            P.check_emb_profile("default", fp, default)


def _literal_dice(x, t, cw, eps=1e-6):
    """dice from the formula: per (b, c) I = sum p [t == c], U = sum p + sum [t == c] over every pixel; mean_b mean_c w_c (1 - (2I + eps) / (U + eps))"""
    b, c = x.shape[:2]
    p = torch.softmax(x.double(), 1)
    total = 0.0
    for i in range(b):
        for k in range(c):
            hit = t[i] == k
            inter, union = float(p[i, k][hit].sum()), float(p[i, k].sum()) + int(hit.sum())
            total += float(cw[k]) * (1.0 - (2.0 * inter + eps) / (union + eps))
    return total / (b * c)


def _literal_fp(x, t, eps=1e-6):
    """fp from the formula: a[b][c] = class c absent from image b once ignored targets read as 0; per non-ignored pixel
    sum_c p_c a / (A_b + eps); the sum over pixels / number of non-ignored pixels"""
    b, c = x.shape[:2]
    p = torch.softmax(x.double(), 1)
    total, pixels = 0.0, 0
    for i in range(b):
        seen = set(torch.where(t[i] == R.IGNORE, torch.zeros_like(t[i]), t[i]).unique().tolist())
        absent = [k for k in range(c) if k not in seen]
        keep = t[i] != R.IGNORE
        pixels += int(keep.sum())
        for k in absent:
            total += float(p[i, k][keep].sum()) / (len(absent) + eps)
    return total / pixels


@pytest.mark.parametrize("profile", ["random", "padded", "wrong", "offset_1024"])
def test_references_agree_with_torch_in_fp64(profile):
    shape = P.MAIN_SHAPES[1]
    for pattern in P.patterns_for(profile, shape):
        x, t = P.inputs(shape, profile, pattern)
        for cwt in (True, False):
            cw = R.class_weights(t, shape[1], cwt)
            for gamma in (0.0, 2.0):
                xd = x.double().requires_grad_(True)
                ce = F.cross_entropy(xd, t, reduction="none", ignore_index=R.IGNORE)
                wt = torch.where(t == R.IGNORE, torch.zeros(()).double(), cw[t.clamp_min(0)])
                want = ((1 - torch.exp(-ce)) ** gamma * wt * ce).mean()
                (gw,) = torch.autograd.grad(want, xd)
                l, g = P._ref_part(shape, profile, pattern, "focal", gamma, cwt)
                assert abs(l - float(want.detach())) <= 1e-12 * abs(float(want.detach())) and float((g - gw).abs().max()) <= 1e-12 * float(gw.abs().max())
            l, _ = P._ref_part(shape, profile, pattern, "dice", 0.0, cwt)
            assert abs(l - _literal_dice(x, t, cw)) <= 1e-12 * abs(l), (pattern, cwt)
        l, _ = P._ref_part(shape, profile, pattern, "fp", 0.0, False)
        assert abs(l - _literal_fp(x, t)) <= 1e-12 * max(abs(l), 1e-30), pattern
    # the weighted reference of a combined mask is the sum of its parts
    ref = P.reference(shape, profile, "base", 7, 2.0, True)
    assert set(ref["parts"]) == {"focal", "dice", "fp"}
    assert ref["value"] == pytest.approx(sum(P.WEIGHTS[k] * ref["components"][i] for i, k in enumerate(("focal", "dice", "fp"))), rel=1e-14)


def test_the_pair_breakdown_sums_to_the_contrastive_loss():
    for profile in P.EMB_PROFILES:
        case, ref = P.emb_case(profile, P.EMB_SHAPES[0], "most_on")
        whole = R.prompt_contrastive(case["emb"], case["flags"], case["t_prime"], case["bias"])
        assert ref["loss"] == pytest.approx(float(whole), rel=1e-13)
        assert torch.isfinite(ref["demb"]).all()
        rows = ref["demb"].reshape(P.EMB_BATCH, -1, case["emb"].shape[-1])
        assert float(rows[case["flags"].reshape(P.EMB_BATCH, -1) == 0].abs().max()) == 0.0
        # the row below eps and the zero row take the clamp branch of F.normalize: their gradient is the un-projected sum / 1e-12
        assert float(rows[0, P.SPECIAL_ROWS["below_eps"]].abs().max()) > 1e6 * float(rows[1].abs().max())


def test_the_adamw_statement_is_torch_adamw_in_fp64():
    p, g, m, v = P.adamw_inputs(257)
    for wd in (0.0, 0.01):
        hp = P._hyper32(wd)
        q = torch.nn.Parameter(p.double().clone())
        opt = torch.optim.AdamW([q], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["wd"])
        mom, sq = torch.zeros(257, dtype=torch.float64), torch.zeros(257, dtype=torch.float64)
        pp = p.double()
        for step in (1, 2, 3):
            q.grad = g.double() * step
            opt.step()
            ref = P.adamw64(pp, g.double() * step, mom, sq, step, wd, 1.0)
            pp, mom, sq = ref["p"], ref["m"], ref["v"]
            assert float((q.detach() - pp).abs().max()) <= 1e-13, (wd, step)


def test_restatement_constants():
    """The constants the GPU tests are held to (times MARGIN): values below 16 u, gradients below 2^-15 = 512 u for every component and
    profile - the offset profiles included: with the shift-stable ce and sm a common offset costs nothing - except the per-image
    measure on the four-pixel images of (2049, 2, 2, 2), where the whole-batch measure holds instead."""
    lc = P.logits_constants()
    for key in sorted(lc):
        print("logits constant", key, f"{lc[key]:.3g}")
    for (kind, comp, profile, shape), v in lc.items():
        assert v >= P.U
        if shape != (2049, 2, 2, 2) or kind != "grad":
            assert v <= (16 * P.U if kind == "value" else 2.0 ** -15), (kind, comp, profile, shape, v)
    for k in ("offset_64", "offset_1024", "offset_8192"):
        for shape in P.MAIN_SHAPES:
            assert lc[("grad", "focal", k, shape)] <= 2.0 * lc[("grad", "focal", "random", shape)]
    cc = P.contrastive_constants()
    for key in sorted(cc):
        print("contrastive constant", key, f"{cc[key]:.3g}")
    assert all(P.U <= v <= 1e-3 for v in cc.values()), cc
    ac = P.adamw_constants()
    print("adamw constants", {k: f"{v:.3g}" for k, v in ac.items()})
    assert all(P.U <= v <= 16 * P.U for v in ac.values()), ac


def _logit_mutation_caught(mutate, masks, profiles, patterns, stable=True, cwt=True):
    caught = []
    for shape in P.MAIN_SHAPES:
        for profile in profiles:
            for pattern in patterns:
                if pattern not in P.patterns_for(profile, shape):
                    continue
                x, t = P.inputs(shape, profile, pattern)
                for mask in masks:
                    fig = P.logits_figures(shape, profile, pattern, mask, 2.0, cwt, P.logits32(x, t, mask, 2.0, cwt, stable=stable, mutate=mutate))
                    worst = max(fig["grad"] / P.logits_tol("grad", mask, profile, shape), fig["value"] / P.logits_tol("value", mask, profile, shape))
                    if worst > 1.0:
                        caught.append((shape, profile, pattern, P.MASK_NAME[mask], round(worst, 1)))
    print(f"mutation {mutate or 'lse form'}: caught on {len(caught)} cases, e.g. {caught[:2]}")
    return caught


def test_wrong_variants_of_the_logits_restatement_exceed_the_gpu_tolerance():
    """Each mutation is caught - figure / tolerance > 1 under the GPU tests' own measure - and each on the profile written for it."""
    some = ("random", "padded", "ties")
    assert _logit_mutation_caught("dice_u_no_ignored", (2,), some, ("base", "image_ignored"))
    assert _logit_mutation_caught("dice_no_beta", (2, 7), some, ("base", "single_pixel_class"))
    assert _logit_mutation_caught("fp_scale", (4,), some, ("base", "one_class_image"))
    got = _logit_mutation_caught("fp_no_exception", (4,), some, P.TARGET_PATTERNS)
    assert any(c[2] == "no_class0_with_ignore" for c in got)
    got = _logit_mutation_caught("cw_per_image", (1, 2), some, P.TARGET_PATTERNS)
    assert any(c[2] == "class_in_one_image" and c[3] == "focal" for c in got) and any(c[3] == "dice" for c in got)
    # the lse form: inside the tolerance without an offset, outside it from K = 64 on
    assert not _logit_mutation_caught("", (1,), ("random",), P.TARGET_PATTERNS, stable=False)
    for k in ("offset_64", "offset_1024", "offset_8192"):
        got = _logit_mutation_caught("", (1,), (k,), P.TARGET_PATTERNS, stable=False)
        assert got, k
    # and nothing is caught without a mutation (the restatement sits at 1 / MARGIN of its own tolerance by construction)
    assert not _logit_mutation_caught("", (1, 2, 4, 7), P.LOGIT_PROFILES, ("base",))


def test_wrong_variants_of_the_contrastive_restatement_exceed_the_gpu_tolerance():
    for mutate in ("y_flip", "clamp_all"):
        caught = []
        for profile in P.EMB_PROFILES:
            for mcd in P.EMB_SHAPES:
                case, ref = P.emb_case(profile, mcd, "most_on")
                fig = P.contrastive_figures(ref, P.contrastive32(case, mutate))
                worst = max(fig[k] / P.contrastive_tol(k, profile) for k in fig)
                if worst > 1.0:
                    caught.append((profile, mcd, f"{worst:.3g}"))
        print(f"mutation {mutate}: caught on {caught}")
        assert {c[0] for c in caught} == set(P.EMB_PROFILES), (mutate, caught)
    # a flipped label is a different function: the fp64 reference with the same flips is what the mutated restatement computes
    case, _ = P.emb_case("balanced", P.EMB_SHAPES[0], "all_on")
    m, c, _ = P.EMB_SHAPES[0]
    flipped = P.contrastive64(case, P.flipped_labels(m * c, c))
    fig = P.contrastive_figures(flipped, P.contrastive32(case, "y_flip"))
    assert max(fig[k] / P.contrastive_tol(k, "balanced") for k in fig) <= 1.0, fig


def test_the_fully_ignored_batch_has_the_documented_answers_in_the_reference():
    """fp is 0 / 0 (no valid pixel), focal is 0, dice still has a value and a gradient: ignored pixels add their p to U."""
    shape = P.MAIN_SHAPES[0]
    x, _ = P.inputs(shape, "random", "base")
    t = torch.full((shape[0],) + shape[2:], R.IGNORE)
    cw = R.class_weights(t, shape[1], True)
    assert float(R.focal(x, t, 2.0, cw)) == 0.0 and math.isnan(float(R.false_positive(x, t))) and 0.0 < float(R.dice(x, t, cw)) <= 1.0
    got = P.logits32(x, t, 7, 2.0, True)
    assert got["components"][0] == 0.0 and math.isnan(got["components"][2]) and bool(torch.isfinite(got["grad"]).all())
