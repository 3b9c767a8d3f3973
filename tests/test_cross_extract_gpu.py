"""GPU: the kernels of ``embedding_extraction="cross_attention"`` called directly - la_extract_pool (with la_extract_pool_plan),
la_extract_fold and la_extract_unfold (csrc/extract.hip) - with the conventions of tests/test_multi_embedding_gpu.py: outputs sit between
NaN guards, assertions are bit-exact where the arithmetic allows and otherwise a bound derived from fp64 quantities on the CPU, evaluated
from the same fp32 inputs; refused arguments leave NaN-filled outputs untouched.

la_extract_pool computes out[z, j, :] = sum_l softmax_l(qt[z, j] . x[z, l]) x[z, l] over the L = M hw rows of pair z = (b, c).

Bound of the normal-data case.  U = 2^-24.  A score is a D-term fp32 fmaf chain: |s^ - s| <= (D + 1) U sum_f |qt_f x_lf|; with
Delta = max_l of that, every weight exp(s^_l - m^) differs from exp(s_l - m) by a factor within e^(+-2 Delta) (the score and the maximum
each move by Delta), by the exponential's relative error eps_e and its factors, and numerator and denominator are L-term fp32 sums:
    |out - ref| <= (4 Delta + 4 eps_e + 2 (L + 3) U) sum_l p_l |x_lf|     per element.
eps_e: the kernel calls expf, whose documented error on this target is 1 ulp: eps_e = 2^-23.
"""
import math

import pytest
import torch
from tests.helpers import GUARD, L, check_guards, guarded, untouched, within_1ulp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS_E = 2.0 ** -23
HEADS = 8

# (B, M, C), g, n, D: g = 30 with M = 3 (2700 rows, 11 pieces), g = 5 (25 rows: less than one tile; 75 rows: three slabs inside one tile),
# g = 16 (256 rows: exactly one piece; 768: slabs that end where pieces end), every n (R = 8, 32, 40), both D
SHAPES = [((1, 3, 2), 30, 4, 256), ((2, 1, 3), 5, 1, 64), ((2, 1, 3), 16, 5, 256), ((1, 3, 2), 16, 5, 64), ((2, 1, 3), 30, 1, 64),
          ((1, 3, 2), 5, 4, 256)]
IDS = [f"B{b}M{m}C{c}-g{g}-n{n}-D{d}" for (b, m, c), g, n, d in SHAPES]


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def pair_rows(x, b, m, c):
    """x (B M C, hw, D), slabs in (b, m, c) order -> (B C, M hw, D)"""
    _, hw, d = x.shape
    return x.view(b, m, c, hw, d).permute(0, 2, 1, 3, 4).reshape(b * c, m * hw, d)


def run_pool(L, x, qt, b, m, c, hw, d, n):
    """-> out (B C, 8 n, D) on the device, computed between NaN guards (output and scratch)."""
    r = HEADS * n
    split, ns, per = L.extract_pool_plan(m, hw, d, r)
    sbuf, scratch = guarded(b * c * per)
    buf, out = guarded(b * c, r, d)
    L.extract_pool(x.cuda(), qt.cuda(), b, m, c, hw, d, n, scratch, out)
    check_guards(buf, out)
    assert bool(torch.isnan(torch.cat([sbuf[:GUARD], sbuf[GUARD + scratch.numel():]])).all()), "scratch guards were overwritten"
    return out


@pytest.mark.parametrize("m,hw,d,n", [(3, 900, 256, 4), (1, 25, 64, 1), (1, 256, 256, 5), (3, 256, 64, 5), (10, 900, 256, 16)])
def test_plan_depends_on_the_four_sizes_and_covers_the_rows(L, m, hw, d, n):
    split, ns, per = L.extract_pool_plan(m, hw, d, HEADS * n)
    assert split >= 1 and ns == -(-m * hw // split)
    tiles = -(-HEADS * n // 16)
    assert per >= ns * 16 * tiles * (d + 2) and per <= ns * 16 * (tiles + 1) * (d + 2)
    assert (split, ns, per) == L.extract_pool_plan(m, hw, d, HEADS * n)
    for bad in ((m, hw, 96, HEADS * n), (m, hw, d, HEADS * 17), (m, hw, d, 0), (m, hw, d, 12), (0, hw, d, HEADS * n)):
        with pytest.raises(RuntimeError, match="la_extract_pool_plan"):
            L.extract_pool_plan(*bad)


@pytest.mark.parametrize("bmc,g,n,d", SHAPES, ids=IDS)
def test_zero_queries_give_the_plain_mean_of_an_integer_stream(L, bmc, g, n, d):
    """All scores are 0, every weight is exactly 1 and the sums of integers are exact: the output is the mean over the M hw rows of the
    pair within 1 ulp.  A dropped, doubled or misplaced row, or a pair that reads another pair's slabs, is a whole-integer error.  The
    queries are handed over in the broadcast form (one [R, D] block for every pair)."""
    (b, m, c), hw, r = bmc, g * g, HEADS * n
    x = torch.randint(-8, 9, (b * m * c, hw, d), generator=torch.Generator().manual_seed(40 + g + d)).float()
    out = run_pool(L, x, torch.zeros(r, d), b, m, c, hw, d, n)
    ref = pair_rows(x.double(), b, m, c).mean(dim=1, keepdim=True).expand(b * c, r, d)
    assert within_1ulp(out, ref)


def hot_rows(split, hw, m):
    """Row indices worth a one-hot: the first and last row, the ends of slabs and the ends of pieces."""
    rows_total = m * hw
    cand = [0, rows_total - 1, hw - 1, hw, (m - 1) * hw, split - 1, split, (rows_total - 1) // split * split, (rows_total - 1) // split * split - 1,
            15, 16, 63, 64, rows_total // 2]
    return sorted({v for v in cand if 0 <= v < rows_total})


@pytest.mark.parametrize("bmc,g,n,d", SHAPES, ids=IDS)
def test_one_hot_rows_come_back_bit_for_bit(L, bmc, g, n, d):
    """Query j looks at channel j only (qt[z, j, j] = 1), where the stream holds an ASCENDING ramp l / 64 - the running maximum is updated
    in every tile - plus 300 in the one hot row of (pair, query): that row scores at least 250 above every other, the fp32 weights of
    the others underflow to exactly 0 and the output is the hot row bit for bit.  The hot rows sit at the first and last row, at the
    first and last rows of slabs and of pieces (the piece length comes from la_extract_pool_plan) and cycle over pairs and queries."""
    (b, m, c), hw, r = bmc, g * g, HEADS * n
    rows_total = m * hw
    split, ns, _ = L.extract_pool_plan(m, hw, d, r)
    assert r <= d
    x = rnd(b * m * c, hw, d, seed=50 + g + d + n)
    xp = pair_rows(x, b, m, c).clone()                               # (B C, L, D)
    xp[:, :, :r] = (torch.arange(rows_total).float() / 64)[None, :, None]
    cand = hot_rows(split, hw, m)
    hot = torch.tensor([[cand[(z * r + j) % len(cand)] for j in range(r)] for z in range(b * c)])
    for z in range(b * c):
        for j in range(r):
            xp[z, hot[z, j], j] += 300.0
    x = xp.view(b, c, m, hw, d).permute(0, 2, 1, 3, 4).reshape(b * m * c, hw, d).contiguous()
    qt = torch.zeros(b * c, r, d)
    qt[:, torch.arange(r), torch.arange(r)] = 1.0
    out = run_pool(L, x, qt, b, m, c, hw, d, n).cpu()
    want = torch.stack([xp[z, hot[z]] for z in range(b * c)])
    bad = (out != want).any(dim=-1).nonzero()
    assert bad.numel() == 0, f"(pair, query) {bad[:8].tolist()} with hot rows {[int(hot[z, j]) for z, j in bad[:8].tolist()]} (piece {split})"


@pytest.mark.parametrize("bmc,g,n,d", SHAPES, ids=IDS)
def test_normal_data_within_the_derived_bound_and_batch_invariant(L, bmc, g, n, d):
    """Score spread around 30 at the largest shape; float64 on the CPU from the same fp32 inputs; the bound of the module docstring.  Then
    every pair alone (B = C = 1) gives bit-identical rows: the split depends on (M, hw, D, R) only."""
    (b, m, c), hw, r = bmc, g * g, HEADS * n
    lrows = m * hw
    x = rnd(b * m * c, hw, d, seed=60 + g + d)
    qt = rnd(b * c, r, d, seed=61 + g + n) * (4.3 / math.sqrt(d))
    out = run_pool(L, x, qt, b, m, c, hw, d, n)
    xp, q64 = pair_rows(x.double(), b, m, c), qt.double()
    s = q64 @ xp.transpose(1, 2)
    p = torch.softmax(s, dim=-1)
    ref = p @ xp
    delta = (d + 1) * U * (q64.abs() @ xp.abs().transpose(1, 2)).max(dim=-1, keepdim=True).values
    bound = (4 * delta + 4 * EPS_E + 2 * (lrows + 3) * U) * (p @ xp.abs())
    err = (out.double().cpu() - ref).abs()
    spread = (s.max(-1).values - s.min(-1).values)
    print(f"[derived] extract_pool {bmc} g={g} n={n} D={d}: spread {float(spread.min()):.1f}..{float(spread.max()):.1f} err {float(err.max()):.3e} "
          f"bound {float(bound.max()):.3e} worst ratio {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    xv = x.view(b, m, c, hw, d)
    for z in range(b * c):
        one = run_pool(L, xv[z // c, :, z % c].contiguous(), qt[z:z + 1].contiguous(), 1, m, 1, hw, d, n)
        assert torch.equal(one[0], out[z]), f"pair {z} alone differs from the pair in the batch"


def test_refused_arguments_leave_the_output_untouched(L):
    b, m, c, hw = 1, 2, 2, 25
    for d, n in ((96, 4), (64, 17), (64, 0)):
        r = HEADS * max(n, 1)
        x = rnd(b * m * c, hw, d, seed=70).cuda()
        qt = rnd(b * c, HEADS * n, d, seed=71).cuda() if n else torch.zeros(0, device="cuda")
        buf, out = guarded(b * c, HEADS * n, d) if n else guarded(1)
        out = out if n else out[:0]
        sbuf, scratch = guarded(b * c * 4 * 48 * (d + 2))
        with pytest.raises(RuntimeError, match="la_extract_pool"):
            L.extract_pool(x, qt, b, m, c, hw, d, n, scratch, out)
        assert untouched(buf) and untouched(sbuf), (d, n, r)
    x, qt = rnd(4, 25, 64, seed=72).cuda(), rnd(4, 8, 64, seed=73).cuda()
    buf, out = guarded(4, 8, 64)
    with pytest.raises(ValueError, match="scratch"):
        L.extract_pool(x, qt, 2, 1, 2, 25, 64, 1, torch.empty(16, device="cuda"), out)
    with pytest.raises(ValueError, match="extract_pool"):
        L.extract_pool(x, qt[:3].contiguous(), 2, 1, 2, 25, 64, 1, torch.empty(1 << 16, device="cuda"), out)
    assert untouched(buf)


@pytest.mark.parametrize("bc,n,d", [(3, 1, 64), (2, 4, 256), (5, 5, 128), (1, 16, 256)])
def test_fold_and_unfold_against_float64(L, bc, n, d):
    """la_extract_fold: qt[z, h n + j] = W_k,h^T q[z n + j, head h] / sqrt(hd), an hd-term fmaf chain and one product: (hd + 2) U sum|terms|.
    la_extract_unfold: o[z n + j, h hd + e] = W_v[h hd + e] . pooled[z, h n + j] + b_v: D terms in any order and the bias: (D + 2) U
    (sum|terms| + |b|).  Integer inputs come back exactly."""
    di, hd, r = d // 2, d // 2 // HEADS, HEADS * n
    for kind in ("int", "normal"):
        mk = (lambda *s, seed: torch.randint(-4, 5, s, generator=torch.Generator().manual_seed(seed)).float()) if kind == "int" else rnd
        q, wk = mk(bc * n, di, seed=80 + d), mk(di, d, seed=81 + d)
        buf, qt = guarded(bc, r, d)
        L.extract_fold(q.cuda(), wk.cuda(), bc, n, d, qt)
        check_guards(buf, qt)
        q4, w3 = q.double().view(bc, n, HEADS, hd), wk.double().view(HEADS, hd, d)
        ref = torch.einsum("znhe,hef->zhnf", q4, w3).reshape(bc, r, d) / math.sqrt(hd)
        mag = torch.einsum("znhe,hef->zhnf", q4.abs(), w3.abs()).reshape(bc, r, d) / math.sqrt(hd)
        err = (qt.double().cpu() - ref).abs()
        if kind == "int" and hd in (4, 16):                          # 1 / sqrt(hd) is a power of two
            assert torch.equal(qt.cpu(), ref.float())
        else:
            print(f"[derived] extract_fold bc={bc} n={n} D={d}: err {float(err.max()):.3e} bound {float(((hd + 2) * U * mag).max()):.3e}")
            assert bool((err <= (hd + 2) * U * mag).all())
        pooled, wv, bv = mk(bc, r, d, seed=82 + d), mk(di, d, seed=83 + d), mk(di, seed=84 + d)
        buf, o = guarded(bc * n, di)
        L.extract_unfold(pooled.cuda(), wv.cuda(), bv.cuda(), bc, n, d, o)
        check_guards(buf, o)
        p4, v3 = pooled.double().view(bc, HEADS, n, d), wv.double().view(HEADS, hd, d)
        ref = (torch.einsum("zhnf,hef->znhe", p4, v3) + bv.double().view(HEADS, hd)).reshape(bc * n, di)
        mag = (torch.einsum("zhnf,hef->znhe", p4.abs(), v3.abs()) + bv.double().abs().view(HEADS, hd)).reshape(bc * n, di)
        err = (o.double().cpu() - ref).abs()
        if kind == "int":
            assert torch.equal(o.cpu(), ref.float())
        else:
            print(f"[derived] extract_unfold bc={bc} n={n} D={d}: err {float(err.max()):.3e} bound {float(((d + 2) * U * mag).max()):.3e}")
            assert bool((err <= (d + 2) * U * mag).all())
    for bad_d, bad_n in ((96, 4), (64, 17), (64, 0)):
        buf, out = guarded(4096)
        z = torch.zeros(1 << 16, device="cuda")
        with pytest.raises((RuntimeError, ValueError)):
            L.extract_fold(z[: bc * bad_n * (bad_d // 2)], z[: (bad_d // 2) * bad_d], bc, bad_n, bad_d, out[: bc * HEADS * bad_n * bad_d] if bad_n else out[:0])
        with pytest.raises((RuntimeError, ValueError)):
            L.extract_unfold(z[: bc * HEADS * bad_n * bad_d], z[: (bad_d // 2) * bad_d], z[: bad_d // 2], bc, bad_n, bad_d, out[: bc * bad_n * (bad_d // 2)] if bad_n else out[:0])
        assert untouched(buf)
