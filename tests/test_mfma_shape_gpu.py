"""GPU: do the two 16-bit MFMA shapes of gfx950 round alike?

``la_mfma_shape_probe`` computes one 32 x 32 x K product on a single wave, K ascending in 64-deep tiles as the GEMM main loops walk it,
with ``v_mfma_f32_32x32x16`` (what every ``la_gemm`` kernel issues) or with ``v_mfma_f32_16x16x32``.  Whether the fp32 accumulators of
the two come out equal bit for bit decides whether a main loop may change its MFMA shape without moving results
(profiles/r12_mfma_shape.md).  They do: so ``gemm_t256w`` runs its main loop on 16x16x32 where ``LaGemmPlan.mfma`` says so, and every output of
``la_gemm`` must equal, bit for bit, what the 32x32x16 main loop writes (``gemm_variant(2 | GEMM_VARIANT_MFMA32)``) - and the fp64 product
within the tolerance the other GEMM tests use.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.helpers import L, rel_err

pytestmark = pytest.mark.gpu

KS = (64, 128, 768, 3072)
DTYPES = (torch.float16, torch.bfloat16)


def _operands(k, dt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(32, k, generator=g).cuda().to(dt), torch.randn(32, k, generator=g).cuda().to(dt)


@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_probe_computes_the_product(L, dt):
    """Both shapes of the probe against the fp64 product of the same 16-bit operands: fp32 accumulation of K N(0, 1) products of
    magnitude sqrt(K) carries a relative error of a few 2^-24 sqrt(K) - 1e-5 of the largest output leaves a factor of ten."""
    for k in KS:
        a, w = _operands(k, dt, 1200 + k)
        ref = a.double() @ w.double().t()
        for shape in (0, 1):
            got = L.mfma_shape_probe(a, w, shape).double()
            err = float((got - ref).abs().max() / ref.abs().max())
            print(f"probe {dt} K={k} shape={shape}: max err / max |ref| = {err:.3e}")
            assert err < 1e-5, (k, shape, err)


@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_mfma_shapes_round_alike(L, dt):
    """32 x 32 x K for K = 64, 128, 768, 3072 on N(0, 1) data: every accumulator of the 16x16x32 walk equals the 32x32x16 walk's."""
    for k in KS:
        a, w = _operands(k, dt, 1200 + k)
        c32, c16 = L.mfma_shape_probe(a, w, 0), L.mfma_shape_probe(a, w, 1)
        torch.cuda.synchronize()
        ndiff = int((c32 != c16).sum())
        rel = float((c32 - c16).abs().max() / c32.abs().max())
        print(f"shapes {dt} K={k}: {ndiff} of 1024 accumulators differ, max |diff| / max |c| = {rel:.3e}")
        assert torch.equal(c32, c16), (k, ndiff, rel)


# ---- la_gemm with the 16x16x32 main loop on and off ---------------------------------------------------------------------------------------
TOL16 = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2}          # (tests/test_ops_gpu.py)
T256W = 6
NS = (256, 768)
# two k-tiles (the minimum), an odd count, the encoder's depth - and 1536, from where the plan gives the residual epilogues (EPI 3, 7, 11)
# the 16x16x32 main loop too (gemm_plan.h, w4_mfma_shape)
KS_GEMM = (128, 192, 768, 1536)
# the plain epilogues (EPI 1 - 3) reach gemm_t256w from K = 256 only (gemm_plan.h, plan_t256: K / 32 >= 8;
# tests/test_gemm_plan_mfma_cpu.py::test_plain_epilogues_reach_the_four_wave_kernel_from_k256_only): K = 256 (the minimum there) and
# 320 (an odd count) stand in for 128 and 192
KS_PLAIN = (256, 320, 768, 1536)
_G = {}


def _rn(*shape, seed, scale=1.0):
    g = _G.setdefault("g", torch.Generator(device="cuda"))
    g.manual_seed(seed)
    return torch.randn(*shape, device="cuda", generator=g) * scale


def _smallest_w4_rows(L, n, k, dt, ncu=0):
    """The smallest multiple of 256 rows whose plain 16-bit call the plan sends to the four-wave kernel (one round of 256 x 256 tiles
    over the chip)."""
    for t in range(1, 1025):
        if L.gemm_plan(0x1000, k, 0x2000, k, 256 * t, n, k, L._DT[dt], ncu, bias=0x3000, out16=0x4000).kernel == T256W:
            return 256 * t
    raise AssertionError(f"no row count sends N={n} K={k} to gemm_t256w")


def _on_off(L, plan_args, fn, outs, reset=None):
    """fn() with the plan's MFMA shape and with 32x32x16 forced: the outputs of both, bit-identical; returns (outputs, plan.mfma when on)."""
    res, mfma = {}, {}
    try:
        for v in (2, 2 | L.GEMM_VARIANT_MFMA32):
            L.gemm_variant(v)
            pl = L.gemm_plan(*plan_args[0], **plan_args[1])
            assert pl.kernel == T256W and pl.direct == 1
            mfma[v] = pl.mfma
            for o in outs:
                o.fill_(3.0)
            if reset is not None:
                reset()
            fn()
            torch.cuda.synchronize()
            res[v] = [o.clone() for o in outs]
    finally:
        L.gemm_variant(2)
    assert mfma[2 | L.GEMM_VARIANT_MFMA32] == 0
    for x, y in zip(res[2], res[2 | L.GEMM_VARIANT_MFMA32]):
        assert torch.equal(x, y)
    return res[2], mfma[2]


@pytest.mark.parametrize("ragged", (0, 1), ids=("whole", "ragged"))
@pytest.mark.parametrize("k", KS_PLAIN)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dt", DTYPES, ids=("f16", "bf16"))
def test_gemm_plain_epilogues_on_both_shapes(L, dt, n, k, ragged):
    """bias -> 16 bit, bias -> GELU -> 16 bit, fp32 residual in place, at the smallest row count the plan gives the four-wave kernel
    (+ 100 rows: a ragged last row tile)."""
    m = _smallest_w4_rows(L, n, k, dt) + 100 * ragged
    a = _rn(m, k, seed=1).to(dt)
    w = (_rn(n, k, seed=2) / math.sqrt(k)).to(dt)
    bias, res0 = _rn(n, seed=3), _rn(m, n, seed=4)
    prod = (a.double() @ w.double().t() + bias.double())
    o16 = torch.empty(m, n, device="cuda", dtype=dt)
    o32 = torch.empty(m, n, device="cuda")
    dti = L._DT[dt]
    used = []
    (g16,), on = _on_off(L, ((a, k, w, k, m, n, k, dti), dict(bias=bias, out16=o16)), lambda: L.gemm(a, w, bias=bias, out16=o16), [o16])
    used.append(on)
    assert rel_err(g16, prod.float()) < TOL16[dt]
    (gg,), on = _on_off(L, ((a, k, w, k, m, n, k, dti), dict(bias=bias, out16=o16, act=L.ACT_GELU)),
                        lambda: L.gemm(a, w, bias=bias, out16=o16, act=L.ACT_GELU), [o16])
    used.append(on)
    assert rel_err(gg, F.gelu(prod).float()) < TOL16[dt]
    (g32,), on = _on_off(L, ((a, k, w, k, m, n, k, dti), dict(bias=bias, res=o32, out32=o32)),
                         lambda: L.gemm(a, w, bias=bias, res=o32, out32=o32), [o32], reset=lambda: o32.copy_(res0))
    used.append(on)
    assert rel_err(g32, (prod + res0.double()).float()) < TOL16[dt]
    print(f"plain {dt} m={m} n={n} k={k}: LaGemmPlan.mfma of EPI 1, 2, 3 = {used}")
    assert used == [1, 1, int(k >= 1536)]          # (both shapes really ran: the comparison above is not one kernel against itself)


@pytest.mark.parametrize("ragged", (0, 1), ids=("whole", "ragged"))
@pytest.mark.parametrize("k", KS_GEMM)
@pytest.mark.parametrize("n", NS)
def test_gemm_normfold_epilogues_on_both_shapes(L, n, k, ragged):
    """The producer and consumer epilogues of the folded LayerNorm with the argument sets of tests/test_normfold_gpu.py: EPI 7 (fp32 stream,
    group vector on tile edges), 8 / 9 (consumer, + GELU), 11 (plane-pair stream in place) and 12 (the same with groups of 128 rows)."""
    m = 512 + 100 * ragged
    a = _rn(m, k, seed=11).half()
    w = (_rn(n, k, seed=12) / math.sqrt(k)).half()
    bias, res0 = _rn(n, seed=13), _rn(m, n, seed=14)
    prod = a.double() @ w.double().t()
    used = {}
    # EPI 7
    rvec = _rn(-(-m // 256), n, seed=15, scale=0.3)
    o32 = torch.empty(m, n, device="cuda")
    o16 = torch.empty(m, n, device="cuda", dtype=torch.float16)
    part = torch.empty(m, n // 64, 2, device="cuda")
    kw = dict(bias=bias, res=o32, out32=o32, out16=o16, nstat_out=part, rvec=rvec, rvec_rpg=256)
    (g32, g16, gp), used[7] = _on_off(L, ((a, k, w, k, m, n, k, L.LA_F16), kw), lambda: L.gemm(a, w, **kw), [o32, o16, part], reset=lambda: o32.copy_(res0))
    ref = prod + bias.double() + res0.double() + rvec.double().repeat_interleave(256, dim=0)[:m]
    assert rel_err(g32, ref.float()) < TOL16[torch.float16]
    assert torch.equal(g16, g32.half())
    assert rel_err(gp[..., 0].sum(1), g32.sum(1)) < 1e-5
    # EPI 8 / 9
    x = a.float()
    mr = torch.zeros(-(-m // 256) * 256, 2, device="cuda")
    mr[:m, 0] = x.mean(1)
    mr[:m, 1] = (x.var(1, unbiased=False) + 1e-6).rsqrt()
    ncol = w.float().sum(1).contiguous()
    pre = mr[:m, 1:2].double() * (prod - mr[:m, 0:1].double() * ncol.double()) + bias.double()
    for epi, act in ((8, L.ACT_NONE), (9, L.ACT_GELU)):
        kw = dict(bias=bias, out16=o16, act=act, nstat_in=mr, ncol=ncol)
        (g,), used[epi] = _on_off(L, ((a, k, w, k, m, n, k, L.LA_F16), kw), lambda: L.gemm(a, w, **kw), [o16])
        assert rel_err(g, (F.gelu(pre) if act else pre).float()) < TOL16[torch.float16]
    # EPI 11 / 12
    x0 = _rn(m, n, seed=16) * 3.0
    xs0 = torch.empty(m, 2 * n, device="cuda", dtype=torch.float16)
    xs0[:, :n] = x0.half()
    xs0[:, n:] = (x0 - x0.half().float()).half()
    before = xs0[:, :n].double() + xs0[:, n:].double()
    xs = torch.empty_like(xs0)
    for epi, rpg in ((11, 256), (12, 128)):
        rv = _rn(-(-m // rpg), n, seed=17, scale=0.3)
        kw = dict(bias=bias, out16=xs[:, :n], aux16=xs[:, n:], nstat_out=part, rvec=rv, rvec_rpg=rpg)
        (gx, gp), used[epi] = _on_off(L, ((a, k, w, k, m, n, k, L.LA_F16), dict(kw, ld16=2 * n, ldaux=2 * n)), lambda: L.gemm(a, w, **kw), [xs, part],
                                      reset=lambda: xs.copy_(xs0))
        ref = before + prod + bias.double() + rv.double().repeat_interleave(rpg, dim=0)[:m]
        got = gx[:, :n].float() + gx[:, n:].float()
        assert rel_err(got, ref.float()) < TOL16[torch.float16]
        assert rel_err(gp[..., 0].sum(1), got.sum(1)) < 1e-5
    print(f"normfold m={m} n={n} k={k}: LaGemmPlan.mfma by EPI = {used}")
    assert used == {7: int(k >= 1536), 8: 1, 9: 1 - ragged, 11: int(k >= 1536), 12: 0}
