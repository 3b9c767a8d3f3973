"""CPU: the rows of tests/norm_profiles.py have the properties they are named after at every E the GPU tests use, its fp64 references
are torch's LayerNorm in fp64, and fp32 restatements of the two variance forms give the error constants that
tests/test_layernorm_forward_gpu.py and tests/test_normfold_conditioning_gpu.py hold the kernels to.  No kernel runs here."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import norm_profiles as NP

ALL_E = sorted(set(NP.E_DIRECT) | set(NP.E_FOLD))


@pytest.mark.parametrize("e", ALL_E)
def test_every_profile_has_its_stated_properties(e):
    for kind in NP.ALL_KINDS:
        x = NP.build(kind, 140 if kind != "mixed" else 299, e)
        fig = NP.check_profile(kind, x)
        if kind != "mixed":
            print(f"profile {kind} E={e}: {fig}")
    # the rows of the mixed matrix are the rows of the single profiles
    x = NP.build("mixed", 299, e)
    for k, kind in enumerate(NP.KINDS):
        rows = NP.rows_of_kind("mixed", 299, kind)
        assert rows.tolist() == list(range(k, 299, len(NP.KINDS)))
        assert torch.equal(x[rows], NP.build(kind, rows.numel(), e))


def test_check_profile_refuses_benign_rows():
    x = torch.randn(40, 256, generator=torch.Generator().manual_seed(5)) * 2.0 + 0.5
    for kind in NP.KINDS:
        with pytest.raises(AssertionError):
            NP.check_profile(kind, x)


def test_the_instance_table_is_launch_ln():
    """One E per reachable (LPR, NVT, EXACT); EXACT = false cannot be reached at LPR 1 and 2 (E = 4 and 8 are the only widths there)."""
    seen = {e: NP.ln_instance(e) for e in NP.E_DIRECT}
    assert seen[4] == (1, 1, True) and seen[8] == (2, 1, True) and seen[12] == (4, 1, False) and seen[132] == (64, 1, False)
    assert seen[512] == (64, 2, True) and seen[1280] == (64, 5, True) and seen[1284] == (64, 8, False) and seen[2048] == (64, 8, True)
    reachable = {NP.ln_instance(e) for e in range(4, 2049, 4)}
    assert set(seen.values()) == reachable and len(reachable) == 22          # (1284 and 2044: both ends of the predicated LN_MAXV instance)
    assert not any(lpr <= 2 and not exact for lpr, _, exact in reachable)


@pytest.mark.parametrize("e", [4, 36, 132, 768])
def test_references_agree_with_torch_in_fp64(e):
    g = torch.Generator().manual_seed(e)
    rows, h, w, ws = 2 * 7 * 9, 7, 9, 4
    x = NP.build("mixed", rows, e)
    x2 = 0.25 * torch.randn(rows, e, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(e, generator=g), 0.1 * torch.randn(e, generator=g)
    pe = torch.randn(50, e, generator=g)
    for eps in NP.EPS_VALUES:
        r = NP.layernorm64(x, gamma, beta, eps)
        want = F.layer_norm(x.double(), (e,), gamma.double(), beta.double(), eps)
        live = torch.tensor([k != "constant" for k in NP.kinds_of_rows("mixed", rows)])
        # (torch's fp64 kernel takes the variance in one pass too: on constant rows it is off by 1e-16 rho, see the next test)
        assert float(((r["out"] - want).abs() / (1e-9 * (r["z"].abs() + r["rho"].sqrt()[:, None] * 1e-3 + 1)))[live].max()) <= 1.0
        mu, rstd = NP.stats64(x, eps)
        assert torch.equal(mu, r["mu"]) and torch.equal(rstd, r["rstd"])
        r2 = NP.layernorm64(x, gamma, beta, eps, x2=x2, gelu=True, pe=pe, pe_mod=50)
        xin = x + x2
        assert torch.equal(r2["xin"], xin)
        want = F.gelu(F.layer_norm(xin.double(), (e,), gamma.double(), beta.double(), eps))
        assert float(((r2["out"] - want).abs() / (1e-9 * (r2["z"].abs() + r2["rho"].sqrt()[:, None] * 1e-3 + 1)))[live].max()) <= 1.0
        assert torch.equal(r2["pe"], r2["out"] + pe.double().repeat(3, 1)[:rows])
        xg = 0.25 * torch.randn(-(-rows // 33), e, generator=g)
        r3 = NP.layernorm64(x, gamma, beta, eps, x2=xg, x2_group=33)
        assert torch.equal(r3["xin"], x + xg.repeat_interleave(33, 0)[:rows])
    # row maps: window partition against an explicit pad-and-permute, the padded maps against F.pad
    idx = torch.arange(rows, dtype=torch.float64).view(2, h, w)
    nwy, nwx = -(-h // ws), -(-w // ws)
    padded = F.pad(idx, (0, nwx * ws - w, 0, nwy * ws - h), value=-1.0)
    part = padded.view(2, nwy, ws, nwx, ws).permute(0, 1, 3, 2, 4).reshape(-1)
    dest = NP.window_rows(rows, h, w, ws)
    assert part.numel() == NP.window_rows_total(rows, h, w, ws)
    assert torch.equal(part[dest], torch.arange(rows, dtype=torch.float64)) and int((part >= 0).sum()) == rows
    maps = F.pad(idx, (1, 1, 1, 1), value=-1.0).reshape(-1)
    assert torch.equal(maps[NP.padded_rows(rows, h, w)], torch.arange(rows, dtype=torch.float64))
    rm = NP.layernorm64(torch.randn(2 * (h + 2) * (w + 2), e, generator=g), gamma, beta, 1e-6, window=-2, H=h, W=w)
    assert rm["out"].shape == (rows, e)
    # the pair of the split output
    v = torch.randn(1000, generator=g) * 3.0
    hi, lo = NP.split16(v)
    assert float(((hi.double() + lo.double() - v.double()).abs() - torch.maximum(2.0 ** -22 * v.double().abs(), torch.tensor(2.0 ** -25))).max()) <= 0


def test_consumer_and_chain_references_are_the_same_function_in_exact_arithmetic():
    """consumer64 with UNROUNDED operands is fold_chain64: rstd (x W'^T - mean c) + b' = LayerNorm(x) W^T + b."""
    g = torch.Generator().manual_seed(11)
    m, e, n = 70, 512, 64
    x = NP.build("offset", m, e).double()
    gamma, beta = 1.0 + 0.1 * torch.randn(e, generator=g, dtype=torch.float64), 0.1 * torch.randn(e, generator=g, dtype=torch.float64)
    w, b = torch.randn(n, e, generator=g, dtype=torch.float64) / math.sqrt(e), torch.randn(n, generator=g, dtype=torch.float64)
    mu, rstd = NP.stats64(x, 1e-6)
    wf = w * gamma
    got = NP.consumer64(x, wf, wf.sum(1), b + w @ beta, mu, rstd)
    want = NP.fold_chain64(x, None, gamma, beta, 1e-6, w, b)
    assert float(((got - want).abs() / NP.consumer_scale64(x, wf, wf.sum(1), mu, rstd)).max()) <= 1e-13
    wf16, ncol, bf = NP.fold_operands(w.float(), b.float(), gamma.float(), beta.float())
    assert wf16.dtype == torch.float16 and torch.equal(ncol, wf16.double().sum(1).float())


def test_restatement_constants_and_the_edge_of_the_one_pass_domain():
    """The constants the GPU tests are held to come from here (norm_profiles.constants): C_mean, C_two and C_one are below 8, and on
    offset_out the one-pass form has left its error model - u (1 + rho) C_one would allow < 1e-2 at |mu| / sigma = 2048 and < 0.2 at
    8192, the restatement is off by O(1).  On a constant row of 1000.3 it returns an rstd of order 1 where the two-pass form stays near
    1 / sqrt(eps)."""
    c = NP.constants()
    print("restatement constants:", {k: (round(v, 3) if isinstance(v, float) else v) for k, v in c.items()})
    assert 0.5 <= c["C_mean"] < 8 and 0.5 <= c["C_two"] < 8 and 0.5 <= c["C_one"] < 8
    assert 0 < c["C_slot"] <= 6.5 / 64            # a balanced tree of depth 6 (+ the rounding of the squares)
    for ratio, err in c["left_model"].items():
        model = 8 * NP.U * (1 + ratio * ratio)
        print(f"offset_out |mu|/sigma = {ratio:g}: one-pass rstd error {err:.3g}, the model's bound with C = 8 would be {model:.3g}")
        assert err > 4 * model and err >= 0.25, (ratio, err, model)
    x = NP.build("constant", 4, 768)[3:4]
    assert float(x[0, 0]) == float(torch.tensor(1000.3, dtype=torch.float32))
    for eps in NP.EPS_VALUES:
        _, r1 = NP.onepass32(x, eps)
        _, r2 = NP.twopass32(x, eps)
        print(f"constant 1000.3, eps {eps:g}: one-pass rstd {float(r1):.4g}, two-pass {float(r2):.4g}, exact {eps ** -0.5:.4g}")
        assert 0 < float(r1) <= eps ** -0.5 * (1 + 4 * NP.U)
        assert float(r2) <= eps ** -0.5 * (1 + 4 * NP.U)


def test_faults_of_the_finalize_step_show_on_the_profiles_and_not_on_benign_rows():
    """Dropping the clamp, or adding the slots in another order, leaves rows like those of tests/test_normfold_gpu.py (mean ~ N(0, 1),
    sigma 1 .. 3) inside 2 C_one u (1 + rho) - and without NaN - while the profiles catch both: no clamp turns negative differences
    into NaN on offset_out / constant rows, and a reversed slot order changes bits of (mean, rstd) on the outlier rows."""
    c = NP.constants()
    e, eps = 768, 1e-6
    g = torch.Generator().manual_seed(3)
    benign = torch.randn(512, e, generator=g) * (1.0 + torch.randn(512, 1, generator=g).abs()) + torch.randn(512, 1, generator=g)
    s1, s2 = NP.slot_sums32(benign)
    f = NP.row_figures(benign, eps)
    for clamp, flip in ((False, False), (True, True)):
        _, r = NP.finalize32(s1.flip(1) if flip else s1, s2.flip(1) if flip else s2, e, eps, clamp)
        assert float(((r.double() / f["rstd"] - 1).abs() / (NP.U * (1 + f["rho"]))).max()) <= 2 * c["C_one"]
    nan = 0
    for kind in NP.OUT_OF_DOMAIN:
        x = NP.build(kind, 140, e)
        _, r = NP.finalize32(*NP.slot_sums32(x), e, 1e-12, clamp=False)
        nan += int(torch.isnan(r).sum())
        _, r = NP.finalize32(*NP.slot_sums32(x), e, 1e-12)
        assert bool(torch.isfinite(r).all())
    assert nan > 0
    x = NP.build("outlier", 140, e)
    s1, s2 = NP.slot_sums32(x)
    a, b = NP.finalize32(s1, s2, e, eps), NP.finalize32(s1.flip(1), s2.flip(1), e, eps)
    assert not (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
