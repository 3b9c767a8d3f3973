"""GPU: the LayerNorm folded into its neighbour GEMMs - producer epilogue (LaGemmEpilogue.nstat_out), la_norm_finalize, consumer epilogue
(nstat_in) - on the ill-conditioned rows of tests/norm_profiles.py, against fp64 on the CPU.

The partial sums come out of the REAL producer: A = 0, residual = the profile rows, so the stream the kernel stores is the profile
itself (bit for bit in the fp32 forms; the plane-pair form is fed the rows rounded to an fp16 pair, which it stores back unchanged).
Statistics are then judged against fp64 moments of THAT stored stream.

Bounds, all from tests/norm_profiles.py (constants of the fp32 restatements, tests/test_norm_profiles_cpu.py, doubled for the other
summation order and 1 / sqrtf):
    partial sums   per 64-column slot, 2 C_slot 64 u (slot's sum |x|, resp. sum x^2)
    finalize       in domain (centred, offset, outlier, two_level, near_range): |d mean| <= 2 C_mean u (|mu| + sigma),
                   |d rstd| / rstd <= 2 C_one u (1 + rho) - DESIGN.md's model;  out of domain (offset_out, constant): the mean bound,
                   0 < rstd <= (1 + 4 u) / sqrt(eps), nothing NaN; the padding rows of mr are zero
    consumer       mr given (fp64 statistics rounded to fp32): 2 C u rstd (sum_k |x_k| |w_jk| + |mean c_j|) + ulp32(ref) (the last add)
                   + half an ulp16, C per profile from an fp32 restatement of the same product on the same operands; with GELU x 1.13 + the stated
                   error of the epilogue's GELU polynomial (csrc/la_common.h: 4.6e-5, 1.1e-5 |x| beyond its clamp)
    chain          the consumer bound + the finalize bounds propagated: |d rstd| / rstd |ref - b'| + rstd |d mean| |c_j|
Out of domain the chain is only held to produce no NaN, and a finite value wherever the documented formula, evaluated in fp64 on the
kernel's own stream and its own (mean, rstd), stays inside the fp16 range; how far it is from the true LayerNorm there is recorded
(``[fold] record``), not asserted.  Measured figures: profiles/norm_conditioning.md."""
import functools
import math

import pytest
import torch

from tests import norm_profiles as NP
from tests.helpers import L, check_guards, guarded, pct_rel_err       # noqa: F401  (L: the module's fixture)

pytestmark = pytest.mark.gpu

U = NP.U
M_FULL, M_RAGGED, RPG, K_PROD = 256, 3 * 128 + 5, 128, 128
FORMS = ("out32+out16", "plane pair in place", "periodic residual")
F16_MAX = 65504.0


def eps32(eps):
    return float(torch.tensor(eps, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def rows_of(kind, m, e):
    return NP.build(kind, m, e)


def judge(tag, got, ref64, allow, rows=None):
    if rows is not None:
        if rows.numel() == 0:
            return 0.0
        got, ref64, allow = got[rows], ref64[rows], allow[rows]
    ratio, first = NP.worst(got, ref64, allow)
    print(f"  [fold] {tag}: max err / allowance {ratio:.3g}")
    assert first is None, f"{tag}: element {first} is {ratio:.3g} x its allowance away from the fp64 value (or not finite)"
    return ratio


def producer(L, form, x, rpg=0):
    """x: fp32 CPU rows [m, n] -> (stored stream fp64 CPU [M, n], x16 device [M, n], part device [M, n / 64, 2]).  M = 2 m for the
    periodic form (the rows are the period)."""
    m, n = x.shape
    big = 2 * m if form == "periodic residual" else m
    a = torch.zeros(big, K_PROD, device="cuda", dtype=torch.float16)
    w = (torch.randn(n, K_PROD, generator=torch.Generator().manual_seed(n)) / 8).half().cuda()
    pbuf, part = guarded(big, n // 64, 2)
    kw = {}
    if rpg:
        kw = dict(rvec=torch.zeros(-(-big // rpg), n, device="cuda"), rvec_rpg=rpg)
    if form == "plane pair in place":
        hi, lo = NP.split16(x)
        xbuf, xs = guarded(big, 2 * n, dtype=torch.float16)
        xs[:, :n] = hi.cuda()
        xs[:, n:] = lo.cuda()
        L.gemm(a, w, out16=xs[:, :n], aux16=xs[:, n:], nstat_out=part, **kw)
        check_guards(xbuf, xs)
        stored = xs[:, :n].double().cpu() + xs[:, n:].double().cpu()
        assert torch.equal(stored, hi.double() + lo.double()), "a zero product moved the plane-pair stream"
        x16 = xs[:, :n]
    else:
        obuf, o32 = guarded(big, n)
        hbuf, x16 = guarded(big, n, dtype=torch.float16)
        if form == "periodic residual":
            L.gemm(a, w, res=x.cuda(), res_mod=m, out32=o32, out16=x16, nstat_out=part, **kw)
        else:
            o32.copy_(x.cuda())
            L.gemm(a, w, res=o32, out32=o32, out16=x16, nstat_out=part, **kw)
        check_guards(obuf, o32)
        check_guards(hbuf, x16)
        assert torch.equal(o32.cpu(), x.repeat(big // m, 1)), "a zero product moved the fp32 stream"
        assert torch.equal(x16, o32.clamp(-F16_MAX, F16_MAX).half())
        stored = o32.double().cpu()
    check_guards(pbuf, part)
    return stored, x16, part


def check_partials(tag, stored, part):
    c = NP.constants()
    m, n = stored.shape
    xd = stored.view(m, n // 64, 64)
    p = part.double().cpu()
    judge(tag + " slot sum x", p[..., 0], xd.sum(2), 2 * c["C_slot"] * 64 * U * xd.abs().sum(2) + 1e-300)
    judge(tag + " slot sum x^2", p[..., 1], xd.pow(2).sum(2), 2 * c["C_slot"] * 64 * U * xd.pow(2).sum(2) + 1e-300)


def finalize(L, part, m, e, eps, **kw):
    mpad = -(-m // 256) * 256
    mbuf, mr = guarded(mpad, 2)
    L.norm_finalize(part, m, e, eps, mr, **kw)
    check_guards(mbuf, mr)                       # (nothing NaN, nothing unwritten)
    assert torch.equal(mr[m:], torch.zeros_like(mr[m:])), "padding rows of mr are not zero"
    return mr


def stat_bounds(f):
    c = NP.constants()
    return 2 * c["C_mean"] * U * (f["mu"].abs() + f["sigma"]) + 1e-300, 2 * c["C_one"] * U * (1 + f["rho"])


def check_documented_order(tag, part, mr, e, eps):
    """norm_finalize_kernel documents its order - slots added in index order, mean = s1 / E, var = max(s2 / E - mean^2, 0) - and the
    encoder's bit-reproducibility rests on it.  From the kernel's OWN partials that order gives the mean bit for bit (IEEE adds and one
    division); rstd is held to 4 u of 1 / sqrt(var + eps) with var either as two roundings or as one fused multiply-add (the compiler's
    choice).  Another slot order moves the last bits of s1 and s2, which rho magnifies in var: the offset rows see it."""
    m = part.shape[0]
    p = part.cpu()
    s1, s2 = torch.zeros(m), torch.zeros(m)
    for j in range(p.shape[1]):
        s1, s2 = s1 + p[:, j, 0], s2 + p[:, j, 1]
    mean = s1 / e
    assert torch.equal(mr[:m, 0].cpu(), mean), f"{tag}: the mean is not the slots added in index order, divided by E"
    q = s2 / e
    plain = (q - mean * mean).clamp_min(0.0).double()
    fused = (q.double() - mean.double() ** 2).float().clamp_min(0.0).double()
    got = mr[:m, 1].double().cpu()
    err = torch.minimum(*(((got * (v + eps32(eps)).float().double().sqrt()) - 1).abs() for v in (plain, fused)))
    print(f"  [fold] {tag} documented order: rstd within {float(err.max()) / U:.3g} u of 1 / sqrt(var + eps)")
    assert float(err.max()) <= 4 * U, f"{tag}: rstd is not 1 / sqrt(max(s2 / E - mean^2, 0) + eps) of the slots added in index order"


def check_statistics(tag, stored, mr, eps, kinds, part=None):
    """-> {profile: (worst mean ratio, worst rstd ratio)} of the in-domain rows"""
    m = stored.shape[0]
    f = NP.row_figures(stored, eps32(eps))
    mean, rstd = mr[:m, 0].double().cpu(), mr[:m, 1].double().cpu()
    amean, arel = stat_bounds(f)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(rstd).all()), f"{tag}: non-finite statistics"
    assert bool((rstd > 0).all()) and bool((rstd <= (1 + 4 * U) / math.sqrt(eps32(eps))).all()), f"{tag}: rstd outside (0, 1 / sqrt(eps)]"
    if part is not None:
        check_documented_order(tag, part, mr, stored.shape[1], eps)
    fig = {}
    for name in NP.KINDS:
        rows = torch.tensor([i for i in range(m) if kinds[i] == name], dtype=torch.long)
        if rows.numel() == 0:
            continue
        rm = judge(f"{tag} {name} mean", mean, f["mu"], amean, rows)
        if name in NP.IN_DOMAIN:
            fig[name] = (rm, judge(f"{tag} {name} rstd", rstd, f["rstd"], arel * f["rstd"], rows))
        else:
            off = float((rstd[rows] / f["rstd"][rows] - 1).abs().max())
            print(f"  [fold] record {tag} {name}: rstd off by up to {off:.3g} (relative), rho up to {float(f['rho'][rows].max()):.3g}")
    return fig


# =========================================================================================================================
# producer partials and la_norm_finalize from them
# =========================================================================================================================
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", NP.E_FOLD)
def test_producer_partials_and_finalize(L, n, form):
    """Every profile (and the mixed matrix) through the producer form: M = 256 (one tile; the periodic form repeats the 256 rows twice)
    and M = 3 x 128 + 5 with rvec_rpg = 128 (two groups inside one tile, ragged last tile); finalize with both eps values."""
    for kind in NP.ALL_KINDS:
        for m in (M_FULL,) if form == "periodic residual" else (M_FULL, M_RAGGED):
            rpg = RPG if m == M_RAGGED else 0
            stored, _, part = producer(L, form, rows_of(kind, m, n), rpg)
            kinds = NP.kinds_of_rows(kind, m) * (stored.shape[0] // m)
            tag = f"N={n} {form} M={stored.shape[0]} {kind}"
            check_partials(tag, stored, part)
            for eps in NP.EPS_VALUES:
                mr = finalize(L, part, stored.shape[0], n, eps)
                check_statistics(f"{tag} eps={eps:g}", stored, mr, eps, kinds, part)


@pytest.mark.parametrize("rpg", [128, 133])
@pytest.mark.parametrize("e", [512, 1280])
def test_finalize_column_sums(L, e, rpg):
    """The column-sum phase at E = 512 (four row lanes) and 1280 (one): two groups of 128 / 133 rows of the mixed matrix, every 128-row
    chunk against fp64 of rstd (x16 - mean) with the kernel's own (mean, rstd); the same sums from ready-made statistics (part = None)."""
    m = 2 * rpg
    stored, x16, part = producer(L, "out32+out16", rows_of("mixed", m, e))
    chunks = L.norm_cs_chunks(rpg)
    for eps in NP.EPS_VALUES:
        cbuf, cs = guarded(2 * chunks, e)
        mr = finalize(L, part, m, e, eps, x16=x16, rpg=rpg, cs_part=cs)
        check_guards(cbuf, cs)
        check_statistics(f"E={e} rpg={rpg} eps={eps:g}", stored, mr, eps, NP.kinds_of_rows("mixed", m), part)
        t = (x16.double().cpu() - mr[:m, 0:1].double().cpu()) * mr[:m, 1:2].double().cpu()
        r = torch.arange(m)
        owner = (r // rpg) * chunks + (r % rpg) // 128
        want = torch.zeros(2 * chunks, e, dtype=torch.float64).index_add_(0, owner, t)
        mass = torch.zeros(2 * chunks, e, dtype=torch.float64).index_add_(0, owner, t.abs())
        n = torch.zeros(2 * chunks, dtype=torch.float64).index_add_(0, owner, torch.ones(m, dtype=torch.float64))
        judge(f"E={e} rpg={rpg} eps={eps:g} column sums", cs, want, (n[:, None] + 2) * U * mass + 1e-300)
        before = mr.clone()
        cbuf2, cs2 = guarded(2 * chunks, e)
        L.norm_finalize(None, m, e, eps, mr, x16=x16, rpg=rpg, cs_part=cs2)
        check_guards(cbuf2, cs2)
        assert torch.equal(cs2, cs) and torch.equal(mr, before)


# =========================================================================================================================
# consumer
# =========================================================================================================================
@functools.lru_cache(maxsize=None)
def linear(n, k):
    g = torch.Generator().manual_seed(17 * n + k)
    w = torch.randn(n, k, generator=g) / math.sqrt(k)
    b = 0.02 * torch.randn(n, generator=g)
    gamma, beta = 1.0 + 0.1 * torch.randn(k, generator=g), 0.1 * torch.randn(k, generator=g)
    return (w, b, gamma, beta) + NP.fold_operands(w, b, gamma, beta)


def consumer_allowance(x16, wf, ncol, bf, mean32, rstd32, gelu, kinds):
    """(ref64, allowance before the 16-bit rounding, {profile: C of the fp32 restatement on that profile's rows}).  C is taken per
    profile: one outlier early in k leaves its magnitude in every later partial sum (C ~ 15 there, ~ 2 on the other profiles)."""
    pre = NP.consumer64(x16, wf, ncol, bf, mean32, rstd32)
    scale = NP.consumer_scale64(x16, wf, ncol, mean32, rstd32)
    restated = rstd32[:, None] * (x16.float() @ wf.float().t() - mean32[:, None] * ncol[None, :]) + bf[None, :]
    ratio = ((restated.double() - pre).abs() / (U * scale + 1e-300)).amax(1)
    c_row, c = torch.zeros_like(ratio), {}
    for name in set(kinds):
        rows = torch.tensor([i for i, k in enumerate(kinds) if k == name], dtype=torch.long)
        c[name] = float(ratio[rows].max())
        c_row[rows] = c[name]
    allow = 2 * c_row[:, None] * U * scale + NP.ulp32(pre)
    if gelu:
        allow = 1.13 * allow + torch.maximum(torch.tensor(4.6e-5, dtype=torch.float64), 1.1e-5 * pre.abs())
    return (NP.gelu64(pre) if gelu else pre), allow, c


def run_consumer(L, x16, mr, n, k, gelu):
    _, _, _, _, wf, ncol, bf = linear(n, k)
    m = x16.shape[0]
    obuf, out = guarded(m, n, dtype=torch.float16)
    L.gemm(x16, wf.cuda(), bias=bf.cuda(), out16=out, act=L.ACT_GELU if gelu else L.ACT_NONE, nstat_in=mr, ncol=ncol.cuda())
    torch.cuda.synchronize()
    return obuf, out


def judge_fp16(tag, out, ref, allow, rows=None):
    """elements whose fp64 value (plus allowance) leaves the fp16 range are only held to be no NaN"""
    got = out.double().cpu()
    assert not bool(torch.isnan(got).any()), f"{tag}: NaN"
    full = allow + 0.5 * NP.ulp16(ref.abs() + allow, torch.float16)
    inside = ref.abs() + full < F16_MAX
    got = torch.where(inside, got, ref)
    return judge(tag, got, ref, full, rows)


@pytest.mark.parametrize("gelu", [False, True], ids=["linear", "gelu"])
@pytest.mark.parametrize("k", [512, 768])
@pytest.mark.parametrize("m", [256, 261])
def test_consumer_applies_given_statistics(L, m, k, gelu):
    """nstat_in on the mixed matrix with fp64 statistics rounded to fp32 (M = 261: the padding rows of mr hold NaN - they are read
    unpredicated and must not reach a stored row).  At |mu| / sigma = 512 the allowance is 512 x the centred one: x16 is un-normalised."""
    n = 256
    x = rows_of("mixed", m, k)
    x16 = x.half()
    kinds = NP.kinds_of_rows("mixed", m)
    _, _, _, _, wf, ncol, bf = linear(n, k)
    for eps in NP.EPS_VALUES:
        mu, rstd = NP.stats64(x, eps32(eps))
        mr = torch.full((-(-m // 256) * 256, 2), float("nan"), device="cuda")
        mr[:m, 0], mr[:m, 1] = mu.float().cuda(), rstd.float().cuda()
        obuf, out = run_consumer(L, x16.cuda(), mr, n, k, gelu)
        check_guards(obuf, out, may_hold_fill=True)
        ref, allow, c = consumer_allowance(x16, wf, ncol, bf, mu.float(), rstd.float(), gelu, kinds)
        print(f"  [fold] consumer M={m} K={k} eps={eps:g}: C of the fp32 restatement", {a: round(v, 2) for a, v in c.items()})
        for name in NP.KINDS:
            rows = torch.tensor([i for i in range(m) if kinds[i] == name], dtype=torch.long)
            judge_fp16(f"consumer M={m} K={k} eps={eps:g} {'gelu ' if gelu else ''}{name}", out, ref, allow, rows)


# =========================================================================================================================
# chain: producer -> finalize -> consumer, and the record of its distance to the true LayerNorm -> Linear
# =========================================================================================================================
def direct_path(L, x, n, e, eps, gelu):
    """la_layernorm -> plain la_gemm on the same rows (the form Lam.norm_fold = False keeps)"""
    w, b, gamma, beta, _, _, _ = linear(n, e)
    y16 = torch.empty(x.shape[0], e, device="cuda", dtype=torch.float16)
    L.layernorm(x.cuda(), gamma.cuda(), beta.cuda(), eps, out16=y16, dt=L.LA_F16)
    out = torch.empty(x.shape[0], n, device="cuda", dtype=torch.float16)
    L.gemm(y16, w.half().cuda(), bias=b.cuda(), out16=out, act=L.ACT_GELU if gelu else L.ACT_NONE)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("form", FORMS[:2])
@pytest.mark.parametrize("e", NP.E_FOLD)
def test_fold_chain(L, e, form):
    """Every profile through producer -> la_norm_finalize -> consumer (N = 256, with and without GELU, both eps values)."""
    n, m = 256, M_FULL
    w, b, gamma, beta, wf, ncol, bf = linear(n, e)
    for kind in NP.KINDS:
        x = rows_of(kind, m, e)
        stored, x16, part = producer(L, form, x)
        for eps in NP.EPS_VALUES:
            mr = finalize(L, part, m, e, eps)
            f = NP.row_figures(stored, eps32(eps))
            amean, arel = stat_bounds(f)
            for gelu in (False, True):
                obuf, out = run_consumer(L, x16, mr, n, e, gelu)
                check_guards(obuf, out, may_hold_fill=True)
                tag = f"chain E={e} {form} eps={eps:g} {'gelu ' if gelu else ''}{kind}"
                got = out.double().cpu()
                assert not bool(torch.isnan(got).any()), f"{tag}: NaN"
                if kind in NP.IN_DOMAIN:
                    ref, allow, _ = consumer_allowance(x16.cpu(), wf, ncol, bf, f["mu"].float(), f["rstd"].float(), gelu, [kind] * m)
                    pre = NP.consumer64(x16.cpu(), wf, ncol, bf, f["mu"].float(), f["rstd"].float())
                    # (statistics as fp32 operands of the reference: their rounding, u relative, is inside the finalize bounds)
                    spread = arel[:, None] * (pre - bf.double()[None, :]).abs() + f["rstd"][:, None] * amean[:, None] * ncol.double().abs()[None, :]
                    judge_fp16(tag, out, ref, allow + (1.13 if gelu else 1.0) * spread)
                else:
                    own = NP.consumer64(x16.cpu(), wf, ncol, bf, mr[:m, 0].cpu(), mr[:m, 1].cpu(), gelu)
                    inside = own.abs() < 6.0e4
                    assert bool(torch.isfinite(got[inside]).all()), f"{tag}: non-finite output where the formula's own value is in range"
                    print(f"  [fold] record {tag}: {int((~torch.isfinite(got)).sum())} of {got.numel()} outputs saturate to inf")
                true = NP.fold_chain64(stored, None, gamma, beta, eps32(eps), w, b, gelu)
                fin = torch.isfinite(got)
                direct = direct_path(L, stored.float(), n, e, eps, gelu).double().cpu()
                scale = float(true.abs().max())
                print(f"  [fold] record {tag}: folded max-norm {float((got - true)[fin].abs().max()) / scale:.3g} pct "
                      f"{pct_rel_err(torch.where(fin, got, true), true):.3g} | direct max-norm {float((direct - true).abs().max()) / scale:.3g} pct "
                      f"{pct_rel_err(direct, true):.3g} | inf {int((~fin).sum())}")
                if kind == "offset" and not gelu:      # the same per |mu| / sigma: the fold's 16-bit operand is the un-normalised row
                    for j in range(0, len(NP.OFFSET_RATIO), 2):
                        rows = torch.tensor([i for i in range(m) if i % len(NP.OFFSET_RATIO) in (j, j + 1)])
                        print(f"  [fold] record {tag} |mu|/sigma={NP.OFFSET_RATIO[j]:g}: folded max-norm "
                              f"{float((got - true)[rows].abs().max()) / scale:.3g} | direct max-norm {float((direct - true)[rows].abs().max()) / scale:.3g}")
