"""GPU: the training kernels of ``embedding_extraction="cross_attention"`` called directly - la_extract_pool_lse, la_extract_pool_bwd (with
la_extract_pool_bwd_plan), la_extract_fold_bwd and la_extract_unfold_bwd (csrc/extract.hip, csrc/extract_bwd.hip) - with the conventions of
tests/test_cross_extract_gpu.py: outputs and scratch sit between NaN guards, assertions are bit-exact where the arithmetic allows and
otherwise a bound derived from fp64 quantities on the CPU, evaluated from the same fp32 inputs; refused arguments leave NaN-filled
outputs untouched.

For pair z with stream rows x_l (L = M hw of them) and folded queries j (R = 8 n):  s_jl = qt_j . x_l,  p_jl = exp(s_jl - lse_j),
t_jl = dout_j . x_l,  delta_j = dout_j . out_j,  ds_jl = p_jl (t_jl - delta_j),  dx_l = sum_j (p_jl dout_j + ds_jl qt_j),
dqt_j = sum_l ds_jl x_l.  The backward's inputs are x, qt, out, lse and dout, and the closed form is evaluated in fp64 AT THOSE fp32 INPUTS
(out and lse as la_extract_pool_lse left them); the lse test ties lse itself to the fp64 logsumexp.

Bounds.  U = 2^-24 (a rounding), eps_e = 2^-23 (expf and logf: 1 ulp on this target).  All first order; the factor SECOND = 1.01 covers the
products of two error terms (each below 1e-3).
  s, t     D-term fp32 fmaf chains: |s^ - s| <= Delta_jl = (D + 1) U sum_f |qt_jf x_lf|,  |t^ - t| <= tau_jl = (D + 1) U sum_f |dout_jf x_lf|.
  lse      logsumexp moves by at most max_l Delta_jl when the scores do.  The sum of the weights: every term carries the exponential of
           its weight, up to three rescalings inside its wave, one when the waves merge and one when the pieces merge - six expf and six
           products - and the sum has L terms: relative (6 eps_e + (L + 6) U).  logf of a value in [1, L]: eps_e log L.  The final add: U |lse|.
               |lse^ - lse| <= max_l Delta_jl + 6 eps_e + (L + 6) U + eps_e log L + U |lse|.
  p        exp(s^ - lse) with the subtraction rounded and expf at 1 ulp: relative rho_jl = Delta_jl + U |s_jl - lse_j| + eps_e.  A weight
           (or a product with one) below the smallest normal fp32 number may come out as zero: ETA = 2^-126 absolute, wherever p rho stands.
  delta    a D-term fp32 sum in any order: eps_d_j = (D + 1) U sum_f |dout_jf out_jf|.
  ds       p^ (t^ - delta^), two roundings: |ds^ - ds| <= (p (rho + 2 U) + ETA) |t - delta| + p (tau + eps_d) + ETA.
  dqt      an L-term sum of products in a fixed order (16 keys a chain, four waves, the tiles in index order):
               |dqt^ - dqt|_jf <= sum_l {(p_jl (rho_jl + (L + 3) U) + ETA) |t_jl - delta_j| + p_jl (tau_jl + eps_d_j) + ETA} |x_lf|.
           Broadcast form: the sum over the B C pairs in z order adds (B C) U sum_z |dqt_z| to the sum of the pairs' bounds.
  dx       a 2 R-term sum of products:
               |dx^ - dx|_lf <= sum_j {(p_jl (rho_jl + (2 R + 1) U) + ETA) |dout_jf|
                                       + [(p_jl (rho_jl + (2 R + 3) U) + ETA) |t_jl - delta_j| + p_jl (tau_jl + eps_d_j) + ETA] |qt_jf|}.
  fold / unfold backward: (terms + 2) U sum |terms| like their forwards (a chain or a butterfly of `terms` products, the scale, the add into
  the destination).
"""
import math

import pytest
import torch
from tests.helpers import GUARD, L, check_guards, guarded, guarded_zero, untouched, within_1ulp
from tests.test_cross_extract_gpu import SHAPES as FWD_SHAPES

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS_E = 2.0 ** -23
SECOND = 1.01
ETA = 2.0 ** -126
HEADS = 8

# (B, M, C), hw, n, D: the forward file's shapes (2700 rows: 11 pieces / 43 tiles; 25 rows: less than a tile; 75: three slabs inside a tile;
# 256: one piece, four whole tiles; 768: slabs that end where pieces end; R = 8, 32, 40), R = 128 on two slabs of 16 rows, and 257 rows: a
# second piece (and a fifth tile) of one row, at D = 128
SHAPES = [(bmc, g * g, n, d) for bmc, g, n, d in FWD_SHAPES] + [((1, 2, 2), 16, 16, 256), ((1, 1, 2), 257, 2, 128)]
IDS = [f"B{b}M{m}C{c}-hw{hw}-n{n}-D{d}" for (b, m, c), hw, n, d in SHAPES]
# zero queries need L = M hw a power of two: 32 (R = 128), 256 (one piece), 512 and 1024 (pieces and slabs end together)
POW2_SHAPES = [((1, 2, 2), 16, 16, 256), ((2, 1, 3), 256, 5, 256), ((1, 2, 2), 256, 4, 64), ((2, 4, 1), 256, 1, 128)]
POW2_IDS = [f"B{b}M{m}C{c}-hw{hw}-n{n}-D{d}" for (b, m, c), hw, n, d in POW2_SHAPES]


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def ints(lo, hi, *shape, seed=0):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def pair_rows(x, b, m, c):
    """x (B M C, hw, D), slabs in (b, m, c) order -> (B C, M hw, D)"""
    _, hw, d = x.shape
    return x.view(b, m, c, hw, d).permute(0, 2, 1, 3, 4).reshape(b * c, m * hw, d)


def slab_rows(xp, b, m, c, hw):
    """(B C, M hw, D) -> (B M C, hw, D): the inverse of pair_rows"""
    d = xp.shape[-1]
    return xp.view(b, c, m, hw, d).permute(0, 2, 1, 3, 4).reshape(b * m * c, hw, d).contiguous()


def scratch_ok(sbuf, scratch):
    torch.cuda.synchronize()
    return bool(torch.isnan(torch.cat([sbuf[:GUARD], sbuf[GUARD + scratch.numel():]])).all())


def run_lse(L, x, qt, b, m, c, hw, d, n):
    """-> (out (B C, 8 n, D), lse (B C, 8 n)) on the device, computed between NaN guards (outputs and scratch)."""
    r = HEADS * n
    sbuf, scratch = guarded(b * c * L.extract_pool_plan(m, hw, d, r)[2])
    obuf, out = guarded(b * c, r, d)
    lbuf, lse = guarded(b * c, r)
    L.extract_pool_lse(x.cuda(), qt.cuda(), b, m, c, hw, d, n, scratch, out, lse)
    check_guards(obuf, out)
    check_guards(lbuf, lse)
    assert scratch_ok(sbuf, scratch), "scratch guards were overwritten"
    return out, lse


def run_bwd(L, x, qt, out, lse, dout, b, m, c, hw, d, n):
    """-> (dx in the layout of x, dqt in the layout of qt) on the device, computed between NaN guards (outputs and scratch)."""
    r = HEADS * n
    rows, nt, per = L.extract_pool_bwd_plan(m, hw, d, r)
    assert rows >= 1 and nt == -(-m * hw // rows) and per >= nt * r * d and (rows, nt, per) == L.extract_pool_bwd_plan(m, hw, d, r)
    sbuf, scratch = guarded(b * c * per)
    xbuf, dx = guarded(b * m * c, hw, d)
    qbuf, dqt = guarded(*qt.shape)
    L.extract_pool_bwd(x.cuda(), qt.cuda(), out.cuda(), lse.cuda(), dout.cuda(), b, m, c, hw, d, n, scratch, dx, dqt)
    check_guards(xbuf, dx)
    check_guards(qbuf, dqt)
    assert scratch_ok(sbuf, scratch), "scratch guards were overwritten"
    return dx, dqt


def closed_form(x, qt, out, lse, dout, b, m, c):
    """fp64 at the kernel's fp32 inputs -> (dx (B M C, hw, D), dqt (B C, R, D), bound_dx, bound_dqt, p (B C, R, L)): the module docstring.
    qt: per pair (B C, R, D) or the broadcast block (R, D)."""
    hw, d = x.shape[1], x.shape[2]
    xp = pair_rows(x.double(), b, m, c)
    lrows = xp.shape[1]
    q = qt.double().expand(b * c, *qt.shape[-2:]) if qt.dim() == 2 else qt.double()
    r = q.shape[1]
    g, o, ls = dout.double(), out.double().cpu(), lse.double().cpu()
    xa, xt = xp.abs(), xp.transpose(1, 2)
    s = q @ xt
    p = torch.exp(s - ls[..., None])
    t = g @ xt
    delta = (g * o).sum(-1, keepdim=True)
    ds = p * (t - delta)
    dxp = p.transpose(1, 2) @ g + ds.transpose(1, 2) @ q
    dqt = ds @ xp
    big_delta = (d + 1) * U * (q.abs() @ xa.transpose(1, 2))
    tau = (d + 1) * U * (g.abs() @ xa.transpose(1, 2))
    rho = big_delta + U * (s - ls[..., None]).abs() + EPS_E
    eps_d = (d + 1) * U * (g * o).abs().sum(-1, keepdim=True)
    td = (t - delta).abs()
    b_dqt = SECOND * (((p * (rho + (lrows + 3) * U) + ETA) * td + p * (tau + eps_d) + ETA) @ xa)
    a1 = p * (rho + (2 * r + 1) * U) + ETA
    a2 = (p * (rho + (2 * r + 3) * U) + ETA) * td + p * (tau + eps_d) + ETA
    b_dx = SECOND * (a1.transpose(1, 2) @ g.abs() + a2.transpose(1, 2) @ q.abs())
    return slab_rows(dxp, b, m, c, hw), dqt, slab_rows(b_dx, b, m, c, hw), b_dqt, p


# ---- la_extract_pool_lse ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bmc,hw,n,d", SHAPES, ids=IDS)
def test_lse_comes_with_the_forward_s_bits(L, bmc, hw, n, d):
    """la_extract_pool_lse: `out` is la_extract_pool's bit for bit (the same kernels), in both qt forms; lse is within the derived bound of
    the fp64 logsumexp of the scores."""
    (b, m, c), r = bmc, HEADS * n
    lrows = m * hw
    x = rnd(b * m * c, hw, d, seed=160 + hw + d)
    for form in ("pair", "broadcast"):
        qt = rnd(*((b * c, r, d) if form == "pair" else (r, d)), seed=161 + hw + n) * (4.3 / math.sqrt(d))
        out, lse = run_lse(L, x, qt, b, m, c, hw, d, n)
        scratch = torch.empty(b * c * L.extract_pool_plan(m, hw, d, r)[2], device="cuda")
        plain = torch.empty(b * c, r, d, device="cuda")
        L.extract_pool(x.cuda(), qt.cuda(), b, m, c, hw, d, n, scratch, plain)
        assert torch.equal(out, plain)
        xp = pair_rows(x.double(), b, m, c)
        q64 = qt.double().expand(b * c, r, d) if form == "broadcast" else qt.double()
        s = q64 @ xp.transpose(1, 2)
        ref = torch.logsumexp(s, dim=-1)
        delta = (d + 1) * U * (q64.abs() @ xp.abs().transpose(1, 2)).max(dim=-1).values
        bound = SECOND * (delta + 6 * EPS_E + (lrows + 6) * U + EPS_E * math.log(lrows) + U * ref.abs())
        err = (lse.double().cpu() - ref).abs()
        print(f"[derived] extract_pool_lse {bmc} hw={hw} n={n} D={d} {form}: err {float(err.max()):.3e} bound {float(bound.min()):.3e}.."
              f"{float(bound.max()):.3e} worst ratio {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())


# ---- la_extract_pool_bwd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bmc,hw,n,d", POW2_SHAPES, ids=POW2_IDS)
def test_zero_queries_spread_the_integer_gradient_evenly(L, bmc, hw, n, d):
    """All scores are 0 and L = M hw is a power of two: lse = log L, every weight is 1 / L exactly, and with small integers in the stream
    and in dout every product and partial sum is an integer multiple of 1 / L^2 below 2^24 of them (checked on the inputs below).  Then
    dx_l = (sum_j dout_j) / L exactly for every row of the pair, and dqt_j = sum_l (t_jl - delta_j) x_l / L is the fp64 value within 1 ulp.
    A dropped, doubled or misplaced row, or a pair that reads another pair's slabs or queries, is a whole-integer error.  The queries go in
    the broadcast form; dqt is then the sum over the pairs."""
    (b, m, c), r = bmc, HEADS * n
    lrows = m * hw
    assert lrows & (lrows - 1) == 0
    x = ints(-1, 1, b * m * c, hw, d, seed=140 + hw + d)
    dout = torch.zeros(b * c, r, d)
    pick = torch.randint(0, d, (b * c, r, 4), generator=torch.Generator().manual_seed(141 + hw + n))
    dout.scatter_(2, pick, ints(-2, 2, b * c, r, 4, seed=142 + hw + n))
    qt = torch.zeros(r, d)
    out, lse = run_lse(L, x, qt, b, m, c, hw, d, n)
    xp = pair_rows(x.double(), b, m, c)
    assert torch.equal(out.cpu().double(), xp.mean(dim=1, keepdim=True).expand(b * c, r, d))          # integers / 2^k: exact
    assert within_1ulp(lse, torch.full((b * c, r), math.log(lrows), dtype=torch.float64))
    g = dout.double()
    t = g @ xp.transpose(1, 2)
    delta = (g * out.cpu().double()).sum(-1, keepdim=True)
    ds = (t - delta) / lrows
    assert float((ds.abs() @ xp.abs()).sum(dim=0).max()) * lrows * lrows < 2 ** 24                   # every partial sum is exact in fp32
    dx, dqt = run_bwd(L, x, qt, out, lse, dout, b, m, c, hw, d, n)
    want_dx = slab_rows((g.sum(dim=1, keepdim=True) / lrows).expand(b * c, lrows, d).contiguous(), b, m, c, hw)
    assert torch.equal(dx.cpu().double(), want_dx)
    assert within_1ulp(dqt, (ds @ xp).sum(dim=0))


def hot_rows(split, tile, hw, m):
    """Row indices worth a one-hot: the first and last row, the ends of slabs, of the forward's pieces and of the backward's tiles."""
    rows_total = m * hw
    last = rows_total - 1
    cand = [0, last, hw - 1, hw, (m - 1) * hw, split - 1, split, last // split * split, last // split * split - 1, tile - 1, tile,
            last // tile * tile, last // tile * tile - 1, 15, 16, rows_total // 2]
    return sorted({v for v in cand if 0 <= v < rows_total})


@pytest.mark.parametrize("bmc,hw,n,d", SHAPES, ids=IDS)
def test_one_hot_rows_take_the_whole_gradient(L, bmc, hw, n, d):
    """The construction of the forward's one-hot test: query j looks at channel j only, where the stream holds an ascending ramp l / 64 (the
    forward's running statistics move in every tile) plus 300 in the one hot row of (pair, query), at the first and last rows of slabs,
    pieces and tiles.  Every other row scores at least 250 below: its fp32 weight exp(s - lse) underflows to exactly 0, so every row that
    is hot for no query gets dx exactly 0; a hot row gets the sum of its queries' dout within the derived bound, and dqt stays within its
    bound of the closed form."""
    (b, m, c), r = bmc, HEADS * n
    rows_total = m * hw
    split = L.extract_pool_plan(m, hw, d, r)[0]
    tile = L.extract_pool_bwd_plan(m, hw, d, r)[0]
    assert r <= d
    x = rnd(b * m * c, hw, d, seed=150 + hw + d + n)
    xp = pair_rows(x, b, m, c).clone()
    xp[:, :, :r] = (torch.arange(rows_total).float() / 64)[None, :, None]
    cand = hot_rows(split, tile, hw, m)
    hot = torch.tensor([[cand[(z * r + j) % len(cand)] for j in range(r)] for z in range(b * c)])
    for z in range(b * c):
        for j in range(r):
            xp[z, hot[z, j], j] += 300.0
    x = slab_rows(xp, b, m, c, hw)
    qt = torch.zeros(b * c, r, d)
    qt[:, torch.arange(r), torch.arange(r)] = 1.0
    dout = rnd(b * c, r, d, seed=151 + hw + n)
    out, lse = run_lse(L, x, qt, b, m, c, hw, d, n)
    dx, dqt = run_bwd(L, x, qt, out, lse, dout, b, m, c, hw, d, n)
    ref_dx, ref_dqt, b_dx, b_dqt, _ = closed_form(x, qt, out, lse, dout, b, m, c)
    is_hot = torch.zeros(b * c, rows_total, dtype=torch.bool)
    is_hot.scatter_(1, hot, True)
    dxp = pair_rows(dx.cpu(), b, m, c)
    cold = dxp[~is_hot]
    assert bool((cold == 0).all()), f"{int((cold != 0).any(dim=-1).sum())} rows that are hot for no query have a gradient"
    want = torch.zeros(b * c, rows_total, d, dtype=torch.float64)
    want.scatter_add_(1, hot[..., None].expand(b * c, r, d), dout.double())
    err_hot = (dxp.double() - want).abs()[is_hot]
    bound_hot = (pair_rows(b_dx, b, m, c) + (pair_rows(ref_dx, b, m, c) - want).abs())[is_hot]     # closed form vs the plain sum: p < 1, ds != 0
    err_q = (dqt.double().cpu() - ref_dqt).abs()
    print(f"[derived] extract_pool_bwd one-hot {bmc} hw={hw} n={n} D={d}: hot dx err {float(err_hot.max()):.3e} worst ratio "
          f"{float((err_hot / bound_hot).max()):.3f}, dqt err {float(err_q.max()):.3e} worst ratio {float((err_q / b_dqt).max()):.3f}")
    assert bool((err_hot <= bound_hot).all()) and bool((err_q <= b_dqt).all())


@pytest.mark.parametrize("bmc,hw,n,d", SHAPES, ids=IDS)
def test_normal_data_both_forms_batch_invariant_and_repeatable(L, bmc, hw, n, d):
    """qt scaled as in the forward's normal-data test (the score spread is printed).  Both qt forms against the closed form in fp64 within the
    bounds of the module docstring; the broadcast dqt is the fp32 sum, in z order, of the per-pair form's rows for the same queries; every
    pair alone (B = C = 1) gives the same dx rows and the same dqt bits as inside the batch; a second run gives the same bits."""
    (b, m, c), r = bmc, HEADS * n
    x = rnd(b * m * c, hw, d, seed=170 + hw + d)
    dout = rnd(b * c, r, d, seed=172 + hw + n)
    q1 = rnd(r, d, seed=171 + hw + n) * (4.3 / math.sqrt(d))
    got = {}
    for form, qt in (("pair", rnd(b * c, r, d, seed=173 + hw + n) * (4.3 / math.sqrt(d))), ("broadcast", q1),
                     ("pair of the broadcast block", q1.expand(b * c, r, d).contiguous())):
        out, lse = run_lse(L, x, qt, b, m, c, hw, d, n)
        dx, dqt = run_bwd(L, x, qt, out, lse, dout, b, m, c, hw, d, n)
        ref_dx, ref_dqt, b_dx, b_dqt, p = closed_form(x, qt, out, lse, dout, b, m, c)
        if form == "broadcast":
            b_dqt = b_dqt.sum(dim=0) + SECOND * b * c * U * ref_dqt.abs().sum(dim=0)
            ref_dqt = ref_dqt.sum(dim=0)
        e_x, e_q = (dx.double().cpu() - ref_dx).abs(), (dqt.double().cpu() - ref_dqt).abs()
        s = torch.log(p)
        spread = s.max(-1).values - s.min(-1).values
        print(f"[derived] extract_pool_bwd {bmc} hw={hw} n={n} D={d} {form}: spread {float(spread.min()):.1f}..{float(spread.max()):.1f} "
              f"dx err {float(e_x.max()):.3e} bound {float(b_dx.max()):.3e} worst ratio {float((e_x / b_dx).max()):.3f}; "
              f"dqt err {float(e_q.max()):.3e} bound {float(b_dqt.max()):.3e} worst ratio {float((e_q / b_dqt).max()):.3f}")
        assert bool((e_x <= b_dx).all()) and bool((e_q <= b_dqt).all()), form
        got[form] = (dx, dqt, out, lse, qt)
        dx2, dqt2 = run_bwd(L, x, qt, out, lse, dout, b, m, c, hw, d, n)
        assert torch.equal(dx2, dx) and torch.equal(dqt2, dqt), f"{form}: a second run gives other bits"
    # the broadcast form reads the same queries as its expansion: the same dx bits, and dqt summed over the pairs in z order
    dx_b, dqt_b = got["broadcast"][:2]
    dx_p, dqt_p = got["pair of the broadcast block"][:2]
    assert torch.equal(dx_b, dx_p)
    acc = dqt_p[0].cpu().clone()
    for z in range(1, b * c):
        acc = acc + dqt_p[z].cpu()
    assert torch.equal(dqt_b.cpu(), acc)
    # every pair alone
    dx, dqt, out, lse, qt = got["pair"]
    xv, dxv = x.view(b, m, c, hw, d), dx.view(b, m, c, hw, d)
    for z in range(b * c):
        one_x, one_q = run_bwd(L, xv[z // c, :, z % c].contiguous(), qt[z:z + 1].contiguous(), out[z:z + 1].contiguous(), lse[z:z + 1].contiguous(),
                               dout[z:z + 1].contiguous(), 1, m, 1, hw, d, n)
        assert torch.equal(one_x.view(m, hw, d), dxv[z // c, :, z % c]), f"pair {z} alone: other dx rows than in the batch"
        assert torch.equal(one_q[0], dqt[z]), f"pair {z} alone: another dqt than in the batch"


def test_refused_arguments_leave_everything_untouched(L):
    b, m, c, hw = 1, 2, 2, 25
    for d, n in ((96, 4), (64, 17), (64, 0)):
        r = HEADS * max(n, 1)
        x = rnd(b * m * c, hw, d, seed=180).cuda()
        z = torch.zeros(0, device="cuda")
        qt = rnd(b * c, HEADS * n, d, seed=181).cuda() if n else z
        lse_in = rnd(b * c, HEADS * n, seed=182).cuda() if n else z
        obuf, out = guarded(b * c, HEADS * n, d) if n else guarded(1)
        lbuf, lse = guarded(b * c, HEADS * n) if n else guarded(1)
        xbuf, dx = guarded(b * m * c, hw, d)
        qbuf, dqt = guarded(b * c, HEADS * n, d) if n else guarded(1)
        out, lse, dqt = (out, lse, dqt) if n else (out[:0], lse[:0], dqt[:0])
        sbuf, scratch = guarded(b * c * 4 * 48 * (d + 2))
        with pytest.raises(RuntimeError, match="la_extract_pool_lse"):
            L.extract_pool_lse(x, qt, b, m, c, hw, d, n, scratch, out, lse)
        with pytest.raises(RuntimeError, match="la_extract_pool_bwd"):
            L.extract_pool_bwd(x, qt, qt, lse_in, qt, b, m, c, hw, d, n, scratch, dx, dqt)
        with pytest.raises(RuntimeError, match="la_extract_pool_bwd_plan"):
            L.extract_pool_bwd_plan(m, hw, d, HEADS * n)
        assert untouched(obuf) and untouched(lbuf) and untouched(xbuf) and untouched(qbuf) and untouched(sbuf), (d, n, r)
    for bad in ((2, 25, 64, 12), (0, 25, 64, 8), (2, 0, 64, 8)):
        with pytest.raises(RuntimeError, match="la_extract_pool_bwd_plan"):
            L.extract_pool_bwd_plan(*bad)
    x, qt, lse_in = rnd(4, 25, 64, seed=183).cuda(), rnd(4, 8, 64, seed=184).cuda(), rnd(4, 8, seed=185).cuda()
    obuf, out = guarded(4, 8, 64)
    lbuf, lse = guarded(4, 8)
    xbuf, dx = guarded(4, 25, 64)
    qbuf, dqt = guarded(4, 8, 64)
    big = torch.empty(1 << 16, device="cuda")
    with pytest.raises(ValueError, match="scratch"):
        L.extract_pool_lse(x, qt, 2, 1, 2, 25, 64, 1, torch.empty(16, device="cuda"), out, lse)
    with pytest.raises(ValueError, match="scratch"):
        L.extract_pool_bwd(x, qt, qt, lse_in, qt, 2, 1, 2, 25, 64, 1, torch.empty(16, device="cuda"), dx, dqt)
    with pytest.raises(ValueError, match="extract_pool_lse"):
        L.extract_pool_lse(x, qt[:3].contiguous(), 2, 1, 2, 25, 64, 1, big, out, lse)
    with pytest.raises(ValueError, match="extract_pool_bwd"):
        L.extract_pool_bwd(x, qt[:3].contiguous(), qt, lse_in, qt, 2, 1, 2, 25, 64, 1, big, dx, dqt)
    with pytest.raises(ValueError, match="extract_pool_bwd"):        # dqt in another layout than qt
        L.extract_pool_bwd(x, qt, qt, lse_in, qt, 2, 1, 2, 25, 64, 1, big, dx, dqt[0])
    with pytest.raises(ValueError, match="extract_pool_bwd"):
        L.extract_pool_bwd(x, qt, qt, lse_in[:3].contiguous(), qt, 2, 1, 2, 25, 64, 1, big, dx, dqt)
    assert untouched(obuf) and untouched(lbuf) and untouched(xbuf) and untouched(qbuf)


# ---- la_extract_fold_bwd, la_extract_unfold_bwd --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bc,n,d", [(3, 1, 64), (2, 4, 256), (5, 5, 128), (1, 16, 256)])
def test_fold_and_unfold_backward_against_float64(L, bc, n, d):
    """la_extract_fold_bwd: dq[z n + j, h hd + e] = W_k[h hd + e] . dqt[z, h n + j] / sqrt(hd) (D terms, written), dW_k[h hd + e] += sum_(z, j)
    q[z n + j, h hd + e] dqt[z, h n + j] / sqrt(hd) (BC n terms, added to the destination), db_k written as exactly 0.
    la_extract_unfold_bwd: dpooled[z, h n + j] = sum_e do[z n + j, h hd + e] W_v[h hd + e] (hd terms, written), dW_v and db_v the same sums
    over (z, j) of do x pooled and of do (added).  Bounds (terms + 2) U sum |terms|; integer inputs come back exactly, and a second call
    doubles the accumulated ones."""
    di, hd, r = d // 2, d // 2 // HEADS, HEADS * n
    scale = 1.0 / math.sqrt(hd)
    for kind in ("int", "normal"):
        mk = (lambda *s, seed: ints(-4, 4, *s, seed=seed)) if kind == "int" else rnd
        exact = kind == "int"
        # fold
        dqt, q, wk = mk(bc, r, d, seed=190 + d), mk(bc * n, di, seed=191 + d), mk(di, d, seed=192 + d)
        qb, dq = guarded(bc * n, di)
        wb, dwk = guarded_zero(di, d)
        bb, dbk = guarded(di)
        L.extract_fold_bwd(dqt.cuda(), q.cuda(), wk.cuda(), bc, n, d, dq, dwk, dbk)
        check_guards(qb, dq)
        check_guards(wb, dwk)
        check_guards(bb, dbk)
        assert bool((dbk == 0).all()), "the k_proj.bias gradient is exactly zero"
        g4, q4, w3 = dqt.double().view(bc, HEADS, n, d), q.double().view(bc, n, HEADS, hd), wk.double().view(HEADS, hd, d)
        ref_dq = torch.einsum("zhnf,hef->znhe", g4, w3).reshape(bc * n, di) * scale
        mag_dq = torch.einsum("zhnf,hef->znhe", g4.abs(), w3.abs()).reshape(bc * n, di) * scale
        ref_dw = torch.einsum("znhe,zhnf->hef", q4, g4).reshape(di, d) * scale
        mag_dw = torch.einsum("znhe,zhnf->hef", q4.abs(), g4.abs()).reshape(di, d) * scale
        e_dq, e_dw = (dq.double().cpu() - ref_dq).abs(), (dwk.double().cpu() - ref_dw).abs()
        if exact and hd in (4, 16):                                   # 1 / sqrt(hd) is a power of two
            assert torch.equal(dq.cpu(), ref_dq.float()) and torch.equal(dwk.cpu(), ref_dw.float())
            L.extract_fold_bwd(dqt.cuda(), q.cuda(), wk.cuda(), bc, n, d, dq, dwk, dbk)
            assert torch.equal(dq.cpu(), ref_dq.float()) and torch.equal(dwk.cpu(), (2 * ref_dw).float()) and bool((dbk == 0).all())
        else:
            print(f"[derived] extract_fold_bwd bc={bc} n={n} D={d} {kind}: dq err {float(e_dq.max()):.3e} bound {float(((d + 2) * U * mag_dq).max()):.3e}, "
                  f"dWk err {float(e_dw.max()):.3e} bound {float(((bc * n + 2) * U * mag_dw).max()):.3e}")
            assert bool((e_dq <= (d + 2) * U * mag_dq).all()) and bool((e_dw <= (bc * n + 2) * U * mag_dw).all())
        # unfold
        do, pooled, wv = mk(bc * n, di, seed=193 + d), mk(bc, r, d, seed=194 + d), mk(di, d, seed=195 + d)
        pb, dpooled = guarded(bc, r, d)
        wb, dwv = guarded_zero(di, d)
        bb, dbv = guarded_zero(di)
        L.extract_unfold_bwd(do.cuda(), pooled.cuda(), wv.cuda(), bc, n, d, dpooled, dwv, dbv)
        check_guards(pb, dpooled)
        check_guards(wb, dwv)
        check_guards(bb, dbv)
        o4, p4, v3 = do.double().view(bc, n, HEADS, hd), pooled.double().view(bc, HEADS, n, d), wv.double().view(HEADS, hd, d)
        ref_dp = torch.einsum("znhe,hef->zhnf", o4, v3).reshape(bc, r, d)
        mag_dp = torch.einsum("znhe,hef->zhnf", o4.abs(), v3.abs()).reshape(bc, r, d)
        ref_dw = torch.einsum("znhe,zhnf->hef", o4, p4).reshape(di, d)
        mag_dw = torch.einsum("znhe,zhnf->hef", o4.abs(), p4.abs()).reshape(di, d)
        ref_db, mag_db = do.double().sum(dim=0), do.double().abs().sum(dim=0)
        e_dp, e_dw, e_db = (dpooled.double().cpu() - ref_dp).abs(), (dwv.double().cpu() - ref_dw).abs(), (dbv.double().cpu() - ref_db).abs()
        if exact:
            assert torch.equal(dpooled.cpu(), ref_dp.float()) and torch.equal(dwv.cpu(), ref_dw.float()) and torch.equal(dbv.cpu(), ref_db.float())
            L.extract_unfold_bwd(do.cuda(), pooled.cuda(), wv.cuda(), bc, n, d, dpooled, dwv, dbv)
            assert torch.equal(dpooled.cpu(), ref_dp.float()) and torch.equal(dwv.cpu(), (2 * ref_dw).float()) and torch.equal(dbv.cpu(), (2 * ref_db).float())
        else:
            print(f"[derived] extract_unfold_bwd bc={bc} n={n} D={d}: dpooled err {float(e_dp.max()):.3e} bound {float(((hd + 2) * U * mag_dp).max()):.3e}, "
                  f"dWv err {float(e_dw.max()):.3e} bound {float(((bc * n + 2) * U * mag_dw).max()):.3e}, dbv err {float(e_db.max()):.3e}")
            assert bool((e_dp <= (hd + 2) * U * mag_dp).all()) and bool((e_dw <= (bc * n + 2) * U * mag_dw).all())
            assert bool((e_db <= (bc * n + 2) * U * mag_db).all())
    for bad_d, bad_n in ((96, 4), (64, 17), (64, 0)):
        buf, out = guarded(4096)
        z = torch.zeros(1 << 16, device="cuda")
        rr, dd = HEADS * bad_n, bad_d // 2
        with pytest.raises((RuntimeError, ValueError)):
            L.extract_fold_bwd(z[: bc * rr * bad_d], z[: bc * bad_n * dd], z[: dd * bad_d], bc, bad_n, bad_d, out[: bc * bad_n * dd] if bad_n else out[:0],
                               out[: dd * bad_d], out[:dd])
        with pytest.raises((RuntimeError, ValueError)):
            L.extract_unfold_bwd(z[: bc * bad_n * dd], z[: bc * rr * bad_d], z[: dd * bad_d], bc, bad_n, bad_d, out[: bc * rr * bad_d] if bad_n else out[:0],
                                 out[: dd * bad_d], out[:dd])
        assert untouched(buf)
