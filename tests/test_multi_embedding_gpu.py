"""GPU: the four kernels of the per-example family called directly - la_region_mean / la_region_mean_bwd (dec.hip, train.hip) and
la_classify_max / la_classify_max_bwd - against float64 torch on the CPU evaluated from the same fp32 inputs, with the conventions of
tests/test_decoder_ops_gpu.py: outputs sit between NaN (or 7) guards, assertions are bit-exact where the arithmetic allows and otherwise
a bound derived from the fp64 quantities; refused arguments leave NaN-filled outputs untouched.

Bounds.  U = 2^-24.  Any fp32 summation order of n terms (one more rounding allowed) errs by at most (n + 1) U sum|terms| (``sum_bound``).
  region mean        n = |bin| terms and one division: (n + 2) U mean|x| over the bin
  region mean bwd    at most 4 bins per pixel, a division each: 6 U sum_bins |dy| / |bin|
  classify max       a Cf-term dot product per example: (Cf + 1) U sum_f |p_f x_f| =: d(n); the maximum is 1-Lipschitz in the sup norm, so
                     the value is within max_n d(n) of the fp64 maximum, the fp64 score of the reported winner within twice that of the fp64
                     maximum, and the winner IS the fp64 argmax wherever the fp64 top-2 gap exceeds twice that
  classify max bwd   dfeat: C terms; dprotos: the prefill and up to Npix products, folded in any order (LDS and global atomics)
"""
import math

import pytest
import torch

from tests import multi_embedding_ref as R
from tests.helpers import GUARD, L, NAN, check_guards, guarded, untouched, within_1ulp

pytestmark = pytest.mark.gpu

NINF = float("-inf")
U = 2.0 ** -24


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def rint(*shape, seed=0, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


# =========================================================================================================================
# la_region_mean / la_region_mean_bwd
# =========================================================================================================================
B, M, C = 2, 2, 3        # p / C against p % C and the (m, i, j, c) output order both matter
REGION_SHAPES = [(16, 3), (5, 2), (30, 2), (4, 4)]      # overlapping uneven bins; overlapping; the Pascal grid; one pixel per bin


def region_bwd_ref(x64, dy64, g, k):
    x = x64.clone().requires_grad_(True)
    R.pool_examples(x, B, M, C, g, k).backward(dy64)
    return x.grad


@pytest.mark.parametrize("d", [64, 256])
@pytest.mark.parametrize("g,k", REGION_SHAPES)
def test_region_mean_and_backward(L, g, k, d):
    from labelanything_amd import autograd_ops as A
    p, hw, n = B * M * C, g * g, M * k * k
    nmax = max(hi - lo for lo, hi in R.bins(g, k)) ** 2
    for kind in ("int", "normal"):
        x = rint(p, hw, d, seed=900 + g) if kind == "int" else rnd(p, hw, d, seed=901 + g + d)
        xd = x.cuda()
        buf, out = guarded(B, n, C, d)
        L.region_mean(xd, B, M, C, g, k, d, out)
        check_guards(buf, out)
        ref = R.pool_examples(x.double(), B, M, C, g, k)
        if k == g:                                  # one pixel per bin: a permutation of the input, x / 1
            assert torch.equal(out.cpu(), ref.float())
        elif kind == "int":                         # exact sums: a dropped, doubled or misplaced pixel is a whole-integer error
            assert within_1ulp(out, ref)
        else:
            bound = (nmax + 2) * U * R.pool_examples(x.double().abs(), B, M, C, g, k)
            err = (out.double().cpu() - ref).abs()
            print(f"[derived] region_mean g={g} k={k} D={d}: err {float(err.max()):.3e} bound {float(bound.max()):.3e}")
            assert bool((err <= bound).all())
        # the result does not depend on the batch: the first image alone gives bit-identical rows
        b1, out1 = guarded(1, n, C, d)
        L.region_mean(xd[: M * C].contiguous(), 1, M, C, g, k, d, out1)
        check_guards(b1, out1)
        assert torch.equal(out1[0], out[0])
    # backward: every pixel gathers dy / |bin| of its (at most four) bins; written over NaN
    dy = rnd(B, n, C, d, seed=902 + g + d)
    bufx, dx = guarded(p * hw, d)
    L.region_mean_bwd(dy.cuda(), B, M, C, g, k, d, dx)
    check_guards(bufx, dx)
    x64 = x.double()
    ref = region_bwd_ref(x64, dy.double(), g, k)
    got = dx.view(p, hw, d).double().cpu()
    if k == g:
        assert torch.equal(got, ref)
    else:
        bound = 6 * U * region_bwd_ref(x64, dy.double().abs(), g, k)
        err = (got - ref).abs()
        print(f"[derived] region_mean_bwd g={g} k={k} D={d}: err {float(err.max()):.3e} bound {float(bound.max()):.3e}")
        assert bool((err <= bound).all())
    # the autograd node wraps the pair
    xa = xd.view(p * hw, d).clone().requires_grad_(True)
    ya = A.region_mean(xa, B, M, C, g, k)
    ya.backward(dy.cuda())
    assert torch.equal(ya.detach(), out) and torch.equal(xa.grad, dx)


@pytest.mark.parametrize("g,k,d", [(8, 2, 6), (8, 2, 1028), (4, 5, 64), (8, 0, 64)])
def test_region_mean_refusals(L, g, k, d):
    """D % 4 != 0, D > 1024, k > g, k < 1: LA_CHECK_ARG, outputs untouched."""
    p = B * M * C
    x = torch.zeros(p, g * g, d, device="cuda")
    kk = max(k, 1) ** 2
    buf, out = guarded(B, M * kk, C, d)
    if k == 0:
        out = out.view(-1)[:0]
    with pytest.raises((RuntimeError, ValueError)):
        L.region_mean(x, B, M, C, g, k, d, out)
    assert untouched(buf)
    bufx, dx = guarded(p * g * g, d)
    dy = torch.zeros(B, M * kk, C, d, device="cuda")
    if k == 0:
        dy = dy.view(-1)[:0]
    with pytest.raises((RuntimeError, ValueError)):
        L.region_mean_bwd(dy, B, M, C, g, k, d, dx)
    assert untouched(bufx)


# =========================================================================================================================
# la_classify_max / la_classify_max_bwd
# =========================================================================================================================
# (B, N, C, Npix, Cf): every feature width on one tile + a tail (300 = 256 + 44); 256 tokens (the LDS limit N C Cf = 8192) on a partial tile
CM_SHAPES = [(2, 5, 3, 300, 8), (2, 5, 3, 300, 16), (2, 5, 3, 300, 32), (2, 5, 3, 300, 64), (2, 64, 4, 70, 32)]
SKIP_CAP = 0.01          # the exact-winner check may skip at most this fraction of the entries (fp64 top-2 gap <= twice the bound)


def cm_inputs(b, n, c, npix, cf):
    seed = 950 + n * 7 + cf + npix
    feat, protos = rnd(b, npix, cf, seed=seed), rnd(b, n, c, cf, seed=seed + 1)
    flags = (torch.rand(b, n, c, generator=torch.Generator().manual_seed(seed + 2)) < 0.7).to(torch.uint8)
    flags[:, 0, :] = 1                      # every class has an example ...
    flags[0, :, c - 1] = 0                  # ... but one (b, c) has none
    flags[b - 1, :, 0] = 0
    flags[b - 1, n - 2, 0] = 1              # ... and one has a single valid example
    return feat, protos, flags


def cm_reference(feat, protos, flags):
    """fp64 per-example scores (-inf on invalid examples), their maximum / argmax, the per-example dot bound and the top-2 gap."""
    f64, p64 = feat.double(), protos.double()
    per = R.per_example_logits(p64, f64, flags)                                                        # [b, n, c, pix]
    dot_bound = (feat.shape[-1] + 1) * U * torch.einsum("bncf,bpf->bncp", p64.abs(), f64.abs())
    dot_bound = dot_bound.masked_fill((flags == 0).unsqueeze(-1), 0.0)
    seg, win = R.classify_max(p64, f64, flags)
    bound = dot_bound.max(dim=1).values                                                                # [b, c, pix]
    top = per.topk(2, dim=1).values
    gap = torch.where(torch.isfinite(top[:, 1]), top[:, 0] - top[:, 1], torch.full_like(top[:, 0], math.inf))   # a single valid example: no rival
    return per, seg, win, bound, gap


@pytest.mark.parametrize("b,n,c,npix,cf", CM_SHAPES)
def test_classify_max_and_backward(L, b, n, c, npix, cf):
    from labelanything_amd import autograd_ops as A
    feat, protos, flags = cm_inputs(b, n, c, npix, cf)
    per, seg64, win64, bound, gap = cm_reference(feat, protos, flags)
    none = flags.sum(dim=1) == 0                                                                       # [b, c]
    assert bool(none[0, c - 1]) and int(flags[b - 1, :, 0].sum()) == 1 and int(none.sum()) == 1
    fd, pd, fl = feat.cuda().view(b * npix, cf), protos.cuda(), flags.cuda()
    bs, seg = guarded(b, c, npix)
    bw, win = guarded(b, c, npix, dtype=torch.int32, fill=7)
    L.classify_max(fd, pd, fl, b, npix, n, c, cf, seg, win)
    torch.cuda.synchronize()
    assert bool(torch.isnan(torch.cat([bs[:GUARD], bs[GUARD + seg.numel():]])).all()) and not bool(torch.isnan(seg).any())
    check_guards(bw, win, fill=7, may_hold_fill=n > 7)
    got, gw = seg.cpu(), win.cpu().long()
    # no valid example: -inf and -1, exactly there
    assert bool((got[none] == NINF).all()) and bool((gw[none] == -1).all())
    assert bool(torch.isfinite(got[~none]).all()) and bool((gw[~none] >= 0).all()) and bool((gw < n).all())
    # values: within the dot bound of the fp64 maximum
    live = ~none.unsqueeze(-1).expand_as(got)
    err = (got.double() - seg64).abs()[live]
    print(f"[derived] classify_max N={n} C={c} Cf={cf} npix={npix}: err {float(err.max()):.3e} bound {float(bound[live].max()):.3e} "
          f"(min {float(bound[live].min()):.3e})")
    assert bool((err <= bound[live]).all())
    # winners: a valid example whose fp64 score is within twice the bound of the fp64 maximum, everywhere ...
    gwc = gw.clamp_min(0)
    flag_of_winner = torch.gather(flags.long().unsqueeze(-1).expand(b, n, c, npix), 1, gwc.unsqueeze(1)).squeeze(1)
    assert bool((flag_of_winner[live] == 1).all())
    score_of_winner = torch.gather(per, 1, gwc.unsqueeze(1)).squeeze(1)
    assert bool((score_of_winner[live] >= (seg64 - 2 * bound)[live]).all())
    # ... and THE fp64 argmax wherever the fp64 top-2 gap exceeds twice the bound; the entries that leaves out are capped
    clear = (gap > 2 * bound) & live
    skipped = 1.0 - float(clear.sum()) / float(live.sum())
    print(f"[winners] exact check skips {skipped:.4%} of the entries (cap {SKIP_CAP:.0%})")
    assert skipped <= SKIP_CAP
    assert torch.equal(gw[clear], win64[clear])
    # without the winners' plane the values are the same bits
    bs2, seg2 = guarded(b, c, npix)
    L.classify_max(fd, pd, fl, b, npix, n, c, cf, seg2, None)
    torch.cuda.synchronize()
    assert torch.equal(seg2, seg)

    # ---- backward, with the kernel's own winners (validated above) ----------------------------------------------------------
    dseg = rnd(b, c, npix, seed=970 + cf + n)
    dseg[none] = NAN                                      # planes without a winner must not be read into the result
    pre = rnd(b, n, c, cf, seed=971 + cf + n)
    bf, dfeat = guarded(b * npix, cf)
    bp, dprotos = guarded(b, n, c, cf)
    dprotos.copy_(pre)
    L.classify_max_bwd(dseg.cuda(), fd, pd, win, b, npix, n, c, cf, dfeat, dprotos)
    check_guards(bf, dfeat)
    check_guards(bp, dprotos)
    d64 = torch.where(gw >= 0, dseg.double(), torch.zeros((), dtype=torch.float64))                  # [b, c, pix]
    p_win = torch.gather(protos.double().permute(0, 2, 1, 3), 2, gwc.unsqueeze(-1).expand(b, c, npix, cf))   # protos[b, win, c, :] as [b, c, pix, f]
    terms = d64.unsqueeze(-1) * p_win
    ref_dfeat, bnd_dfeat = terms.sum(dim=1), (c + 1) * U * terms.abs().sum(dim=1)
    onehot = torch.zeros(b, n, c, npix, dtype=torch.float64).scatter_(1, gwc.unsqueeze(1), (gw >= 0).double().unsqueeze(1))
    ref_dp = pre.double() + torch.einsum("bncp,bcp,bpf->bncf", onehot, d64, feat.double())
    bnd_dp = (npix + 2) * U * (pre.double().abs() + torch.einsum("bncp,bcp,bpf->bncf", onehot, d64.abs(), feat.double().abs()))
    e1 = (dfeat.view(b, npix, cf).double().cpu() - ref_dfeat).abs()
    e2 = (dprotos.double().cpu() - ref_dp).abs()
    print(f"[derived] classify_max_bwd: dfeat err {float(e1.max()):.3e} bound {float(bnd_dfeat.max()):.3e}; "
          f"dprotos err {float(e2.max()):.3e} bound {float(bnd_dp.max()):.3e}")
    assert bool((e1 <= bnd_dfeat).all()) and bool((e2 <= bnd_dp).all())
    # examples that won nowhere (the invalid ones among them) keep the prefill exactly
    unused = onehot.sum(dim=3) == 0
    assert bool(unused.any()) and torch.equal(dprotos.cpu()[unused], pre[unused])
    # zero gradient: dfeat exactly zero, dprotos exactly the prefill
    bf0, dfeat0 = guarded(b * npix, cf)
    bp0, dprotos0 = guarded(b, n, c, cf)
    dprotos0.copy_(pre)
    L.classify_max_bwd(torch.zeros(b, c, npix, device="cuda"), fd, pd, win, b, npix, n, c, cf, dfeat0, dprotos0)
    check_guards(bf0, dfeat0)
    assert bool((dfeat0 == 0).all()) and torch.equal(dprotos0.cpu(), pre)

    # ---- the autograd node -------------------------------------------------------------------------------------------------
    fa, pa = fd.clone().requires_grad_(True), pd.clone().requires_grad_(True)
    out = A.classify_max(fa, pa, fl, b, npix, n, c)
    assert torch.equal(out.detach(), seg)
    out.backward(torch.nan_to_num(dseg, nan=0.0).cuda())
    assert bool(((fa.grad.view(b, npix, cf).double().cpu() - ref_dfeat).abs() <= bnd_dfeat).all())
    assert bool(((pa.grad.double().cpu() - (ref_dp - pre.double())).abs() <= bnd_dp).all())


@pytest.mark.parametrize("cf", [8, 32])
def test_classify_max_ties_go_to_the_lowest_example(L, cf):
    """Two examples with identical prototypes score identically (same operands, same order): the lower n is reported, and flagging the
    duplicate out changes nothing."""
    b, n, c, npix = 2, 5, 3, 300
    feat, protos, _ = cm_inputs(b, n, c, npix, cf)
    protos[:, 3] = protos[:, 1]
    protos[:, 4] = protos[:, 0]
    flags = torch.ones(b, n, c, dtype=torch.uint8)
    fd, pd = feat.cuda().view(b * npix, cf), protos.cuda()
    bs, seg = guarded(b, c, npix)
    bw, win = guarded(b, c, npix, dtype=torch.int32, fill=7)
    L.classify_max(fd, pd, flags.cuda(), b, npix, n, c, cf, seg, win)
    check_guards(bs, seg)
    check_guards(bw, win, fill=7)
    assert bool((win <= 2).all()) and bool((win >= 0).all())
    assert int((win == 0).sum()) > 0 and int((win == 1).sum()) > 0
    flags2 = flags.clone()
    flags2[:, 3:] = 0
    bs2, seg2 = guarded(b, c, npix)
    bw2, win2 = guarded(b, c, npix, dtype=torch.int32, fill=7)
    L.classify_max(fd, pd, flags2.cuda(), b, npix, n, c, cf, seg2, win2)
    torch.cuda.synchronize()
    assert torch.equal(seg2, seg) and torch.equal(win2, win)
    # the lower duplicate flagged out instead: its twin takes over with the same value
    flags3 = flags.clone()
    flags3[:, :2] = 0
    bs3, seg3 = guarded(b, c, npix)
    bw3, win3 = guarded(b, c, npix, dtype=torch.int32, fill=7)
    L.classify_max(fd, pd, flags3.cuda(), b, npix, n, c, cf, seg3, win3)
    torch.cuda.synchronize()
    assert torch.equal(seg3, seg)
    assert torch.equal(win3, torch.where(win == 0, torch.full_like(win, 4), torch.where(win == 1, torch.full_like(win, 3), win)))


@pytest.mark.parametrize("n,c,cf", [(5, 3, 12), (5, 33, 8), (65, 4, 32), (5, 3, 128)])
def test_classify_max_refusals(L, n, c, cf):
    """Feature widths outside {8, 16, 32, 64}, C > 32, N C Cf > 8192: LA_CHECK_ARG, outputs untouched - forward and backward."""
    b, npix = 1, 64
    feat, protos = torch.zeros(b * npix, cf, device="cuda"), torch.zeros(b, n, c, cf, device="cuda")
    flags = torch.ones(b, n, c, dtype=torch.uint8, device="cuda")
    bs, seg = guarded(b, c, npix)
    bw, win = guarded(b, c, npix, dtype=torch.int32, fill=7)
    with pytest.raises(RuntimeError, match="la_classify_max"):
        L.classify_max(feat, protos, flags, b, npix, n, c, cf, seg, win)
    assert untouched(bs) and untouched(bw, fill=7)
    bf, dfeat = guarded(b * npix, cf)
    bp, dprotos = guarded(b, n, c, cf)
    with pytest.raises(RuntimeError, match="la_classify_max_bwd"):
        L.classify_max_bwd(torch.zeros(b, c, npix, device="cuda"), feat, protos, torch.zeros(b, c, npix, dtype=torch.int32, device="cuda"),
                           b, npix, n, c, cf, dfeat, dprotos)
    assert untouched(bf) and untouched(bp)
