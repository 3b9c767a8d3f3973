"""CPU: tests/train_ref.py proven before the GPU module relies on it.

  * the float64 references against torch: layernorm_bwd64 against autograd of F.layer_norm (+ F.gelu), adamw64 against torch.optim.AdamW;
  * the allowances against a CLEAN fp32 restatement of every kernel's formula (torch fp32 in the kernel's operation order, once more
    with the columns and the rows summed in a permuted order) on every shape and the data of tests/test_train_kernels_gpu.py: within
    half the allowance - otherwise the derivation misses a term;
  * the allowances against PLANTED faults (a) - (h) in that restatement: each must exceed them at the case named for it;
  * the integer-exact input builder: the 2^24 condition for every case.
"""
import math

import pytest
import torch

from tests import test_train_kernels_gpu as G
from tests import train_ref as R

F32 = torch.float32


def t32(v):
    return torch.tensor(v, dtype=F32)


def gelu_grad_f32(z):
    """gelu_grad of train.hip, fp32."""
    cdf = 0.5 * (1.0 + torch.erf(z * t32(0.70710678118654752440)))
    return cdf + z * t32(0.39894228040143267794) * torch.exp(t32(-0.5) * z * z)


def grid_waves(rows, e):
    """Waves of the generic / vector kernel's capped grid: four rows per workgroup and round."""
    vec = e % 256 == 0 and e <= 1280
    cap = 256 * ((8 if e <= 256 else 5 if e <= 512 else 3 if e <= 1024 else 2) if vec else (8 if e <= 256 else 5 if e <= 512 else 3 if e <= 1024 else 1))
    return 4 * min((rows + 3) // 4, cap)


def ln_model(d, gelu, form="plain", dt16=None, permute=False, fault=None):
    """la_layernorm_bwd(_res) restated in fp32: dict(dx, dgamma, dbeta[, out16]).  fault: one of "a" .. "f" (LN_FAULTS
    below: padded mean, second round lost, 16-bit copy rounded before the skip, gelu' at xhat, eps left out, one wave's dbeta lost)."""
    x, dy, gamma, beta, add = d["x"], d["dy"], d["gamma"], d["beta"], d["add"]
    g0, b0 = d["dgamma0"], d["dbeta0"]
    rows, e = x.shape
    if permute:
        gen = torch.Generator().manual_seed(e)
        cp, rp = torch.randperm(e, generator=gen), torch.randperm(rows, generator=gen)
        x, dy, add, gamma, beta, g0, b0 = x[:, cp], dy[:, cp], add[:, cp], gamma[cp], beta[cp], g0[cp], b0[cp]
    inv_e = t32(1.0) / t32(float(e))
    eps = t32(0.0 if fault == "e" else d["eps"])
    mu = x.sum(1, keepdim=True) * (t32(1.0) / t32(64.0 * ((e + 63) // 64)) if fault == "a" else inv_e)
    dd = x - mu
    rstd = torch.rsqrt((dd * dd).sum(1, keepdim=True) * inv_e + eps)
    xh = dd * rstd
    dz = dy
    if gelu:
        dz = dy * gelu_grad_f32(xh if fault == "d" else xh * gamma + beta)
    tg = dz * xh
    g = dz * gamma
    s1 = g.sum(1, keepdim=True) * inv_e
    s2 = (g * xh).sum(1, keepdim=True) * inv_e
    o = rstd * (g - s1 - xh * s2)
    out = {}
    if form != "plain":
        if fault == "c":
            out["out16"] = (o.to(dt16).float() + add).to(dt16)
        o = o + add
        out.setdefault("out16", o.to(dt16))
    out["dx"] = o
    keep = torch.ones(rows, dtype=torch.bool)
    if fault == "b":
        keep[grid_waves(rows, e):] = False                       # only the first round of the grid-stride loop
    keep_b = keep.clone()
    if fault == "f":
        keep_b[torch.arange(rows) % grid_waves(rows, e) == 1] = False       # wave 1's partial sums
    if permute:
        tg, dz, keep, keep_b = tg[rp], dz[rp], keep[rp], keep_b[rp]
    out["dgamma"] = g0 + tg[keep].sum(0)
    out["dbeta"] = b0 + dz[keep_b].sum(0)
    if permute:
        inv = torch.empty_like(cp)
        inv[cp] = torch.arange(e)
        out = {k: (v[:, inv] if v.dim() == 2 else v[inv]) for k, v in out.items()}
    return out


def ln_ratio(d, gelu, form, dt16, **model):
    """max err / allowance of the fp32 model over dx, dgamma, dbeta, out16, and whether any element is beyond its allowance."""
    add = d["add"] if form != "plain" else None
    ref, al = R.layernorm_bwd_case64(d["x"], d["dy"], d["gamma"], d["beta"], d["eps"], gelu, add, dt16 if form != "plain" else None, d["dgamma0"],
                                     d["dbeta0"])
    got = ln_model(d, gelu, form, dt16, **model)
    res = {k: R.check(got[k], ref[k], al[k]) for k in ref}
    ln_ratio.last16 = res["out16"][0] if "out16" in res else 0.0
    return max(r for k, (r, _) in res.items() if k != "out16" or model.get("fault")), {k: r for k, (r, f) in res.items() if f is not None}


def adamw_model(p, g, m, v, h, step, fault=None):
    """adamw_kernel and its host side restated in fp32.  fault "g": weight decay after the update; "h": bias correction with step - 1."""
    lr, b1, b2, eps, wd, gs = (t32(h[k]) for k in ("lr", "b1", "b2", "eps", "wd", "grad_scale"))
    one = t32(1.0)
    s = t32(float(step - 1 if fault == "h" else step))
    bc1 = one - torch.pow(b1, s)
    bc2s = torch.sqrt(one - torch.pow(b2, s))
    step_size = lr / bc1
    gi = g * gs
    pi = p if fault == "g" else p * (one - lr * wd)
    mi = m + (gi - m) * (one - b1)
    vi = v * b2 + ((one - b2) * gi) * gi
    pi = pi - step_size * (mi / (torch.sqrt(vi) / bc2s + eps))
    if fault == "g":
        pi = pi * (one - lr * wd)
    return pi, mi, vi


def adamw_ratios(n, fault=None, fault_step=None):
    """Per step: (max err / allowance over p, exp_avg, exp_avg_sq, names beyond their allowance), the states carried over as on the GPU."""
    p, m, v, grads = R.adamw_data(n)
    h = R.ADAMW_HYPER
    out = {}
    for step, g in zip(R.ADAMW_STEPS, grads):
        args = (p, g, m, v, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], step, h["grad_scale"])
        ref, al = R.adamw64(*args), R.adamw_bound64(*args)
        clean = adamw_model(p, g, m, v, h, step)
        got = adamw_model(p, g, m, v, h, step, fault) if step == fault_step else clean
        res = [R.check(a, b, c) for a, b, c in zip(got, ref, al)]
        out[step] = (max(r for r, _ in res), [name for name, (_, f) in zip(("p", "exp_avg", "exp_avg_sq"), res) if f is not None])
        p, m, v = clean
    return out


# ---- the references against torch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [3, 160, 768])
@pytest.mark.parametrize("gelu", [False, True])
def test_layernorm_bwd64_equals_float64_autograd(e, gelu):
    d = R.ln_data(11, e)
    x, gamma, beta = (d[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = torch.nn.functional.layer_norm(x, (e,), gamma, beta, d["eps"])
    if gelu:
        y = torch.nn.functional.gelu(y)
    y.backward(d["dy"].double())
    dx, dgamma, dbeta, out16 = R.layernorm_bwd64(d["x"], d["dy"], d["gamma"], d["beta"], d["eps"], gelu)
    assert out16 is None
    for mine, ref in ((dx, x.grad), (dgamma, gamma.grad), (dbeta, beta.grad)):
        assert float((mine - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    dx2, _, _, o16 = R.layernorm_bwd64(d["x"], d["dy"], d["gamma"], d["beta"], d["eps"], gelu, d["add"], torch.float16)
    assert torch.equal(dx2, dx + d["add"].double()) and torch.equal(o16, dx2)


def test_adamw64_equals_torch_adamw_over_three_steps():
    p0, m0, v0, grads = R.adamw_data(257)
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    mine, m, v = p0.double(), torch.zeros(257, dtype=torch.float64), torch.zeros(257, dtype=torch.float64)
    for step, g in enumerate(grads, 1):
        p.grad = 0.25 * g.double()
        opt.step()
        mine, m, v = R.adamw64(mine, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 0.25)
        st = opt.state[p]
        for a, b in ((mine, p.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            assert float((a - b).abs().max()) <= 1e-13 * max(1.0, float(b.abs().max())), step


def test_check_reports_the_first_offender_and_never_skips_non_finite_values():
    ref = torch.zeros(3, 4, dtype=torch.float64)
    got = torch.zeros(3, 4)
    assert R.check(got, ref, 1e-6) == (0.0, None)
    got[1, 2], got[2, 0] = 3e-6, 1e-5
    ratio, first = R.check(got, ref, torch.full((3, 4), 1e-6, dtype=torch.float64))
    assert first == (1, 2) and abs(ratio - 10.0) < 1e-3
    for bad in (float("nan"), float("inf")):
        got = torch.zeros(3, 4)
        got[0, 3] = bad
        assert R.check(got, ref, 1.0) == (math.inf, (0, 3))


# ---- the clean model is inside half the allowance --------------------------------------------------------------------------------------
def ln_forms(kind):
    forms = [("plain", False, None), ("plain", True, None)]
    if kind != "narrow":
        forms += [("res", False, G.F16), ("res", False, G.BF16)]
    return forms


@pytest.mark.parametrize("kind,cases", [("generic", G.LN_GENERIC), ("vector", G.LN_VEC), ("narrow", G.LN_NARROW)], ids=["generic", "vector", "narrow"])
def test_clean_fp32_layernorm_model_is_within_half_the_allowance(kind, cases):
    """dx, dgamma, dbeta - every value the kernel computes in fp32 - within HALF their allowance.  out16 is that dx rounded once more: a correct
    rounding uses up to the whole half ulp its allowance adds (err / allowance reaches 1 just above a power of two whatever the derivation),
    so the rounded copy must be inside its allowance (``not over``) and the half applies to the value that is rounded, which is dx."""
    worst = worst16 = 0.0
    for case in cases:
        d = R.ln_data(case[0], case[1])
        for form, gelu, dt in ln_forms(kind):
            for permute in (False, True):
                ratio, over = ln_ratio(d, gelu, form, dt, permute=permute)
                assert not over and ratio <= 0.5, f"{case} {form} gelu {gelu} {dt} permuted {permute}: err / allowance {ratio:.3g}"
                worst, worst16 = max(worst, ratio), max(worst16, ln_ratio.last16)
    print(f"layernorm_bwd ({kind} cases): worst clean err / allowance {worst:.3g} (fp32 values), {worst16:.3g} (16-bit copy after its rounding)")


def test_clean_fp32_gelu_bwd_and_adamw_models_are_within_half_the_allowance():
    worst = worst16 = 0.0
    for n, _ in G.GELU_BWD:
        for dt in (G.F16, G.BF16):
            pre, dh = R.gelu_data(n, dt)
            g32 = dh * gelu_grad_f32(pre.float())
            ref = R.gelu_bwd64(pre, dh)
            worst = max(worst, R.check(g32, ref, R.gelu_bwd_bound64(pre, dh))[0])
            worst16 = max(worst16, R.check(g32.to(dt), ref, R.gelu_bwd_bound64(pre, dh, dt))[0])
    print(f"gelu_bwd16: worst clean err / allowance {worst:.3g} (d32), {worst16:.3g} (d16 after its rounding)")
    assert worst <= 0.5 and worst16 <= 1.0          # (the 16-bit rounding itself: see the LayerNorm test)
    worst = 0.0
    for n in G.ADAMW_N:
        for step, (ratio, over) in adamw_ratios(n).items():
            assert not over, (n, step, over)
            worst = max(worst, ratio)
    print(f"adamw_step: worst clean err / allowance {worst:.3g}")
    assert worst <= 0.5


# ---- planted faults are caught -----------------------------------------------------------------------------------------------------------
LN_FAULTS = [("a", (37, 72), "plain", False, None, "mean over the padded column count"),
             ("b", (1029, 1100), "plain", False, None, "dgamma / dbeta lose the second grid-stride round"),
             ("c", (13, 160), "res", False, torch.float16, "out16 rounded before add is added"),
             ("d", (13, 160), "plain", True, None, "gelu' evaluated at xhat"),
             ("e", (13, 160), "plain", False, None, "eps left out"),
             ("f", (37, 72), "plain", False, None, "one wave's dbeta partial dropped")]


@pytest.mark.parametrize("fault", LN_FAULTS, ids=lambda f: f[0])
def test_planted_layernorm_fault_exceeds_the_allowance(fault):
    letter, case, form, gelu, dt, what = fault
    assert case in [c[:2] for c in G.LN_GENERIC + G.LN_VEC + G.LN_NARROW]
    d = R.ln_data(*case)
    ratio, over = ln_ratio(d, gelu, form, dt, fault=letter)
    print(f"fault ({letter}) {what} at {case}: caught in {sorted(over)} at {ratio:.3g} x the allowance")
    assert over, f"fault ({letter}) {what} stays inside the allowance at {case} ({ratio:.3g})"
    expected = {"a": "dx", "b": "dbeta", "c": "out16", "d": "dx", "e": "dx", "f": "dbeta"}[letter]
    assert expected in over
    if letter in "bf":
        assert "dx" not in over                          # the fault is in the column sums alone
    if letter == "c":
        assert sorted(over) == ["out16"]


def test_a_lost_second_round_is_caught_at_every_case_that_has_one():
    """Fault (b) once more, at every (rows, E) of the generic and the vector kernel whose rows exceed one pass of the capped grid."""
    cases = [c[:2] for c in G.LN_GENERIC + G.LN_VEC if c[0] > grid_waves(c[0], c[1])]
    assert len(cases) == 11
    for case in cases:
        _, over = ln_ratio(R.ln_data(*case), False, "plain", None, fault="b")
        assert "dgamma" in over and "dbeta" in over and "dx" not in over, case


@pytest.mark.parametrize("fault", [("g", 1000, "weight decay applied after the update"), ("h", 2, "bias correction with step - 1")], ids=lambda f: f[0])
def test_planted_adamw_fault_exceeds_the_allowance(fault):
    letter, step, what = fault
    ratio, over = adamw_ratios(G.ADAMW_N[0], fault=letter, fault_step=step)[step]
    print(f"fault ({letter}) {what} at n = {G.ADAMW_N[0]}, step {step}: caught in {over} at {ratio:.3g} x the allowance")
    assert "p" in over and "exp_avg" not in over and "exp_avg_sq" not in over


# ---- integer inputs -----------------------------------------------------------------------------------------------------------------------
def test_integer_inputs_keep_every_partial_sum_exact_in_fp32():
    reductions = [c[0] for c in G.GEMM_TN] + [c[0] for c in G.COLSUM] + [c[0] for c in G.TRANSPOSE_SHAPES] + G.TN16_ROWS + [577]
    assert max(reductions) == R.MAX_REDUCTION
    for r in sorted(set(reductions)):
        t = R.ints(5, 7, seed=r, reduce=r, device="cpu")                     # asserts reduce * 64 + 8 < 2^24
        assert t.dtype == F32 and float(t.abs().max()) <= 8 and torch.equal(t, t.round())
    for dt in (G.F16, G.BF16):
        t = R.ints(64, 64, seed=1, reduce=64, dtype=dt, device="cpu")
        assert torch.equal(t.float(), R.ints(64, 64, seed=1, reduce=64, device="cpu"))       # every value exact in the 16-bit types
    for rows, _ in [c[:2] for c in G.LN_GENERIC + G.LN_VEC + G.LN_NARROW]:
        R.ints(1, seed=0, reduce=rows, factor=1, device="cpu")                # the plain row sums of the exact dbeta test
    with pytest.raises(AssertionError):
        R.ints(2, 2, seed=0, reduce=2 ** 18, device="cpu")                    # 2^18 products of 64
    with pytest.raises(AssertionError):
        R.ints(2, 2, seed=0, reduce=2 ** 21, factor=1, device="cpu")
    dy, x = R.ints(300, 5, seed=1, reduce=300, device="cpu"), R.ints(300, 6, seed=2, reduce=300, device="cpu")
    dw, db = R.gemm_tn_exact(dy, x, torch.ones(5, 6), torch.ones(5))
    assert torch.equal(dw, 1 + dy.t() @ x) and torch.equal(db, 1 + dy.sum(0))
