"""GPU: the four entry points of ``conv_classification`` called directly - la_proto_kernels / la_proto_kernels_bwd and la_classify_conv /
la_classify_conv_bwd (csrc/convcls.hip) - against float64 torch on the CPU (tests/convcls_ref.py and its autograd) evaluated from the same
fp32 inputs.  Conventions of tests/test_levels_gpu.py: outputs sit between NaN guards and are written over NaN; refused arguments leave
NaN-filled outputs untouched.

THE PATH THAT IS BOUNDED: exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) for the three products over channels / taps / pixels and fmaf for the
prototype kernels - fp32 multiply-add throughout, no plane-pair products, so no 3 * 2^-22 per-product term.

Two kinds of input.
  Small integers.  Every product and every partial sum - in ANY order - is an integer whose magnitude the test bounds on the CPU by
    evaluating the same formula on the absolute values; below 2^24 such numbers are exact in fp32, so every output must EQUAL the float64
    result.  An all-ones input counts the taps a pixel has: 9, 12, 15, 16, 20 or 25.
  Normal inputs.  U = 2^-24.  A sum of n terms in any order errs by at most (n + 1) U times the same formula on absolute values:
    n = 25 cf for the logits, 25 C for dfeat, H W for dK, 10 cf for the composed kernels (cf for the first layer inside 9 cf of the
    second).  The gradients of the kernel composition nest two sums and take the total: 18 cf for dprotos (9 cf for dk1, 9 cf over it),
    cf + 9 BC for dW2 (k1 inside), 9 cf + BC for dW1 (dk1 inside).  Printed as [derived] with the worst measured ratio to the bound.
"""
import pytest
import torch

from tests import convcls_ref as R
from tests.helpers import L, check_guards, guarded, guarded_zero, untouched

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 24

FWD_SHAPES = [(1, 1, 32, 2, 3),         # the map is smaller than the 5 x 5 support
              (1, 1, 32, 5, 5),         # every pixel is a border pixel
              (2, 3, 32, 13, 9),        # odd sizes; per-episode kernels with B > 1; a class pair and a single class
              (1, 2, 64, 33, 40),       # straddles tile edges
              (1, 3, 32, 120, 120),     # the recipe's map size
              (1, 11, 32, 24, 24),      # many classes: six workgroups along the class axis
              (1, 17, 32, 24, 24),
              (2, 3, 256, 64, 64)]      # the fixture shape; every channel chunk
BWD_SHAPES = FWD_SHAPES[:4] + [(2, 3, 256, 16, 16)]
PROTO_SHAPES = [(1, 32), (6, 32), (3, 64), (6, 256)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=gen(seed))


def rint(*shape, seed=0, lo=-2, hi=3):
    return torch.randint(lo, hi, shape, generator=gen(seed)).float()


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements with a positive bound; where the bound is zero (a tap that meets no pixel of a map smaller
    than the 5 x 5 support, for instance: every term is absent) the result must be exactly the reference's."""
    err = (got.double() - ref).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all()), "an element whose every term is absent is not exact"
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


# =========================================================================================================================
# la_classify_conv / la_classify_conv_bwd
# =========================================================================================================================
def conv_ref(feat, k, dseg=None):
    """float64: feat (B, H, W, cf) NHWC, k (B, C, 25, cf) -> seg (B, C, H, W) [, dfeat NHWC, dk] of tests/convcls_ref.correlate5."""
    f = feat.double().clone().requires_grad_(dseg is not None)
    kk = k.double().clone().requires_grad_(dseg is not None)
    seg = R.correlate5(f.permute(0, 3, 1, 2), R.from_tap_major(kk))
    if dseg is None:
        return seg
    seg.backward(dseg.double())
    return seg.detach(), f.grad, kk.grad


def run_conv(L, shape, feat, k):
    b, c, cf, h, w = shape
    bs, seg = guarded(b, c, h, w)
    L.classify_conv(feat.cuda().contiguous(), k.cuda().contiguous(), b, c, h, w, cf, seg)
    check_guards(bs, seg)
    return seg.cpu()


def run_conv_bwd(L, shape, dseg, feat, k):
    b, c, cf, h, w = shape
    bf, dfeat = guarded(b, h, w, cf)
    bk, dk = guarded(b, c, 25, cf)
    L.classify_conv_bwd(dseg.cuda().contiguous(), feat.cuda().contiguous(), k.cuda().contiguous(), b, c, h, w, cf, dfeat, dk)
    check_guards(bf, dfeat)
    check_guards(bk, dk)
    return dfeat.cpu(), dk.cpu()


def conv_inputs(shape, kind, seed):
    b, c, cf, h, w = shape
    if kind == "int":
        return rint(b, h, w, cf, seed=seed), rint(b, c, 25, cf, seed=seed + 1), rint(b, c, h, w, seed=seed + 2)
    return rnd(b, h, w, cf, seed=seed), rnd(b, c, 25, cf, seed=seed + 1, scale=0.3), rnd(b, c, h, w, seed=seed + 2)


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_classify_conv_integers_are_exact(L, shape):
    feat, k, _ = conv_inputs(shape, "int", seed=100 + sum(shape))
    worst = float(conv_ref(feat.abs(), k.abs()).max())
    print(f"{shape}: largest sum of magnitudes {worst:.0f} (limit {EXACT_LIMIT:.0f})")
    assert worst < EXACT_LIMIT
    got = run_conv(L, shape, feat, k)
    assert torch.equal(got.double(), conv_ref(feat, k))


@pytest.mark.parametrize("shape", FWD_SHAPES[:5])
def test_all_ones_count_the_taps_and_episodes_keep_their_own_kernels(L, shape):
    b, c, cf, h, w = shape
    b = 2                                          # episode 1 carries the NEGATED kernels of episode 0
    feat = torch.ones(b, h, w, cf)
    k = torch.ones(b, c, 25, cf)
    k[1] = -1.0
    got = run_conv(L, (b, c, cf, h, w), feat, k)
    ny = torch.tensor([min(y + 2, h - 1) - max(y - 2, 0) + 1 for y in range(h)], dtype=torch.float32)
    nx = torch.tensor([min(x + 2, w - 1) - max(x - 2, 0) + 1 for x in range(w)], dtype=torch.float32)
    count = ny[:, None] * nx[None, :]
    if h >= 5 and w >= 5:
        assert set(count.flatten().tolist()) <= {9.0, 12.0, 15.0, 16.0, 20.0, 25.0}
    assert torch.equal(got[0], (cf * count).expand(c, h, w)) and torch.equal(got[1], (-cf * count).expand(c, h, w))


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_classify_conv_random_is_within_the_fp32_bound(L, shape):
    b, c, cf, h, w = shape
    feat, k, _ = conv_inputs(shape, "normal", seed=200 + sum(shape))
    ref = conv_ref(feat, k)
    bound = (25 * cf + 1) * U * conv_ref(feat.abs(), k.abs())
    ratio = worst_ratio(run_conv(L, shape, feat, k), ref, bound)
    print(f"{shape}: [derived] gamma = (25 cf + 1) 2^-24 = {(25 * cf + 1) * U:.3e}; worst |err| / bound {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_classify_conv_bwd_integers_are_exact(L, shape):
    feat, k, dseg = conv_inputs(shape, "int", seed=300 + sum(shape))
    mags = conv_ref(feat.abs(), k.abs(), dseg.abs())
    worst = max(float(m.max()) for m in mags)
    print(f"{shape}: largest sum of magnitudes {worst:.0f} (limit {EXACT_LIMIT:.0f})")
    assert worst < EXACT_LIMIT
    _, dfeat, dk = conv_ref(feat, k, dseg)
    got_f, got_k = run_conv_bwd(L, shape, dseg, feat, k)
    assert torch.equal(got_f.double(), dfeat), "dfeat"
    assert torch.equal(got_k.double(), dk), "dK"


@pytest.mark.parametrize("shape", BWD_SHAPES)
def test_classify_conv_bwd_random_is_bounded_and_repeats_bit_for_bit(L, shape):
    b, c, cf, h, w = shape
    feat, k, dseg = conv_inputs(shape, "normal", seed=400 + sum(shape))
    _, dfeat, dk = conv_ref(feat, k, dseg)
    _, afeat, ak = conv_ref(feat.abs(), k.abs(), dseg.abs())
    got_f, got_k = run_conv_bwd(L, shape, dseg, feat, k)
    rf = worst_ratio(got_f, dfeat, (25 * c + 1) * U * afeat)
    rk = worst_ratio(got_k, dk, (h * w + 1) * U * ak)
    print(f"{shape}: [derived] dfeat n = 25 C = {25 * c}, worst |err| / bound {rf:.4f}; dK n = H W = {h * w}, worst |err| / bound {rk:.4f}")
    assert rf <= 1.0 and rk <= 1.0
    again_f, again_k = run_conv_bwd(L, shape, dseg, feat, k)
    assert torch.equal(again_f, got_f) and torch.equal(again_k, got_k)


def test_classify_conv_refuses_what_it_does_not_take(L):
    b, c, h, w = 1, 2, 6, 6
    for cf in (48, 16, 288):
        feat = torch.ones(b, h, w, cf, device="cuda")
        k = torch.ones(b, c, 25, cf, device="cuda")
        bs, seg = guarded(b, c, h, w)
        with pytest.raises(RuntimeError, match="la_classify_conv.*cf"):
            L.classify_conv(feat, k, b, c, h, w, cf, seg)
        bf, dfeat = guarded(b, h, w, cf)
        bk, dk = guarded(b, c, 25, cf)
        with pytest.raises(RuntimeError, match="la_classify_conv_bwd.*cf"):
            L.classify_conv_bwd(torch.ones(b, c, h, w, device="cuda"), feat, k, b, c, h, w, cf, dfeat, dk)
        assert untouched(bs) and untouched(bf) and untouched(bk)
    feat = torch.ones(b, h, w, 32, device="cuda")
    empty = torch.empty(0, device="cuda")
    with pytest.raises(RuntimeError, match="la_classify_conv"):
        L.classify_conv(feat, empty, b, 0, h, w, 32, empty)               # C = 0
    with pytest.raises(RuntimeError, match="la_classify_conv_bwd"):
        L.classify_conv_bwd(empty, feat, empty, b, 0, h, w, 32, torch.empty_like(feat), empty)
    with pytest.raises(ValueError, match="classify_conv"):
        L.classify_conv(feat, torch.ones(b, c, 25, 32, device="cuda"), b, c, h, w, 32, torch.empty(b, c, h, w + 1, device="cuda"))
    torch.cuda.synchronize()


# =========================================================================================================================
# la_proto_kernels / la_proto_kernels_bwd
# =========================================================================================================================
def proto_ref(e, w1, w2, dk=None):
    """float64: protos (BC, cf), w1, w2 (cf, cf, 3, 3) -> k1 (BC, cf, 3, 3), K (BC, 25, cf) [, dprotos, dw1, dw2]."""
    leaves = [t.double().clone().requires_grad_(dk is not None) for t in (e, w1, w2)]
    k1 = R.first_step(leaves[0], leaves[1])
    k = R.tap_major(R.compose_kernels(*leaves))
    if dk is None:
        return k1, k
    k.backward(dk.double())
    return (k1.detach(), k.detach(), *[t.grad for t in leaves])


def proto_inputs(shape, kind, seed):
    bc, cf = shape
    if kind == "int":
        return (rint(bc, cf, seed=seed, lo=-1, hi=2), rint(cf, cf, 3, 3, seed=seed + 1, lo=-1, hi=2), rint(cf, cf, 3, 3, seed=seed + 2, lo=-1, hi=2),
                rint(bc, 25, cf, seed=seed + 3, lo=-1, hi=2))
    s = (9 * cf) ** -0.5
    return rnd(bc, cf, seed=seed), rnd(cf, cf, 3, 3, seed=seed + 1, scale=s), rnd(cf, cf, 3, 3, seed=seed + 2, scale=s), rnd(bc, 25, cf, seed=seed + 3)


def run_proto(L, shape, e, w1, w2, dk):
    bc, cf = shape
    dev = [t.cuda().contiguous() for t in (e, w1, w2, dk)]
    b1, k1 = guarded(bc, cf, 3, 3)
    bk, k = guarded(bc, 25, cf)
    L.proto_kernels(dev[0], dev[1], dev[2], bc, cf, k1, k)
    check_guards(b1, k1)
    check_guards(bk, k)
    bd, dk1 = guarded(bc, cf, 3, 3)
    be, de = guarded(bc, cf)
    bw1, dw1 = guarded_zero(cf, cf, 3, 3)
    bw2, dw2 = guarded_zero(cf, cf, 3, 3)
    L.proto_kernels_bwd(dev[3], dev[0], k1, dev[1], dev[2], bc, cf, dk1, de, dw1, dw2)
    for buf, view in ((bd, dk1), (be, de), (bw1, dw1), (bw2, dw2)):
        check_guards(buf, view)
    first = [t.cpu() for t in (k1, k, de, dw1, dw2)]
    L.proto_kernels_bwd(dev[3], dev[0], k1, dev[1], dev[2], bc, cf, dk1, de, dw1, dw2)      # dw1, dw2 are ACCUMULATED, dprotos written
    torch.cuda.synchronize()
    return first, [t.cpu() for t in (de, dw1, dw2)]


PROTO_NAMES = ("k1", "K", "dprotos", "dW1", "dW2")


@pytest.mark.parametrize("shape", PROTO_SHAPES)
def test_proto_kernels_integers_are_exact(L, shape):
    e, w1, w2, dk = proto_inputs(shape, "int", seed=500 + sum(shape))
    mags = proto_ref(e.abs(), w1.abs(), w2.abs(), dk.abs())
    worst = max(float(m.max()) for m in mags)
    print(f"{shape}: largest sum of magnitudes {worst:.0f} (limit {EXACT_LIMIT:.0f})")
    assert 2 * worst < EXACT_LIMIT
    ref = proto_ref(e, w1, w2, dk)
    first, second = run_proto(L, shape, e, w1, w2, dk)
    for name, g, r in zip(PROTO_NAMES, first, ref):
        assert torch.equal(g.double(), r), name
    assert torch.equal(second[0].double(), ref[2]), "dprotos is written, not accumulated"
    assert torch.equal(second[1].double(), 2 * ref[3]) and torch.equal(second[2].double(), 2 * ref[4]), "dW1 / dW2 accumulate"


@pytest.mark.parametrize("shape", PROTO_SHAPES)
def test_proto_kernels_random_are_within_the_fp32_bound(L, shape):
    bc, cf = shape
    e, w1, w2, dk = proto_inputs(shape, "normal", seed=600 + sum(shape))
    ref = proto_ref(e, w1, w2, dk)
    mags = proto_ref(e.abs(), w1.abs(), w2.abs(), dk.abs())
    terms = dict(k1=cf, K=10 * cf, dprotos=18 * cf, dW1=9 * cf + bc, dW2=cf + 9 * bc)
    first, _ = run_proto(L, shape, e, w1, w2, dk)
    for name, g, r, m in zip(PROTO_NAMES, first, ref, mags):
        ratio = worst_ratio(g, r, (terms[name] + 1) * U * m)
        print(f"{shape} {name}: [derived] n = {terms[name]}, worst |err| / bound {ratio:.4f}")
        assert ratio <= 1.0, name


def test_proto_kernels_refuse_what_they_do_not_take(L):
    for cf in (48, 16):
        e = torch.ones(2, cf, device="cuda")
        wt = torch.ones(cf, cf, 3, 3, device="cuda")
        b1, k1 = guarded(2, cf, 3, 3)
        bk, k = guarded(2, 25, cf)
        with pytest.raises(RuntimeError, match="la_proto_kernels.*cf"):
            L.proto_kernels(e, wt, wt, 2, cf, k1, k)
        bd, dk1 = guarded(2, cf, 3, 3)
        be, de = guarded(2, cf)
        with pytest.raises(RuntimeError, match="la_proto_kernels_bwd.*cf"):
            L.proto_kernels_bwd(torch.ones(2, 25, cf, device="cuda"), e, torch.ones(2, cf, 3, 3, device="cuda"), wt, wt, 2, cf, dk1, de,
                                torch.zeros_like(wt), torch.zeros_like(wt))
        assert untouched(b1) and untouched(bk) and untouched(bd) and untouched(be)
    torch.cuda.synchronize()


# =========================================================================================================================
# the autograd nodes
# =========================================================================================================================
def test_autograd_nodes_accumulate_into_existing_gradients(L):
    """proto_kernels -> classify_conv through autograd_ops, backward called twice: every .grad holds twice the float64 gradient (integer
    inputs: exactly), with and without a gradient sink for the two weights."""
    from labelanything_amd import autograd_ops as A
    b, c, cf, h, w = 2, 3, 32, 9, 7
    e = rint(b * c, cf, seed=1, lo=-1, hi=2)
    w1, w2 = rint(cf, cf, 3, 3, seed=2, lo=-1, hi=2), rint(cf, cf, 3, 3, seed=3, lo=-1, hi=2)
    feat, dseg = rint(b * h * w, cf, seed=4, lo=-1, hi=2), rint(b, c, h, w, seed=5, lo=-1, hi=2)

    def grads64(ins, ds):
        lv = [t.double().clone().requires_grad_(True) for t in ins]
        k = R.compose_kernels(lv[0], lv[1], lv[2]).view(b, c, cf, 5, 5)
        seg = R.correlate5(lv[3].view(b, h, w, cf).permute(0, 3, 1, 2), k)
        (seg * ds.double()).sum().backward()
        return [t.grad for t in lv], seg.detach()

    ref, seg64 = grads64((e, w1, w2, feat), dseg)
    mags, segmag = grads64([t.abs() for t in (e, w1, w2, feat)], dseg.abs())
    assert 2 * max(float(segmag.max()), *[float(m.max()) for m in mags]) < EXACT_LIMIT        # every partial sum, twice over, is exact
    dev = [t.cuda().requires_grad_(True) for t in (e, w1, w2, feat)]
    for _ in range(2):
        seg = A.classify_conv(dev[3], A.proto_kernels(dev[0], dev[1], dev[2]), b, c, h, w)
        (seg * dseg.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(seg.detach().cpu().double(), seg64)
    for name, t, r in zip(("protos", "w1", "w2", "feat"), dev, ref):
        assert torch.equal(t.grad.cpu().double(), 2 * r), name
    # with a sink the two weight gradients are added in place and autograd gets none
    sink_w = [t.detach().clone().contiguous() for t in dev[1:3]]
    views = [torch.zeros_like(t) for t in sink_w]
    touched = []
    old = A.SINK
    A.SINK = A.GradSink(sink_w, views, touched.append)
    try:
        leaves = [dev[0].detach().clone().requires_grad_(True), sink_w[0].requires_grad_(True), sink_w[1].requires_grad_(True)]
        for _ in range(2):
            seg = A.classify_conv(dev[3].detach(), A.proto_kernels(*leaves), b, c, h, w)
            (seg * dseg.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        A.SINK = old
    assert leaves[1].grad is None and leaves[2].grad is None and sorted(set(touched)) == [0, 1]
    assert torch.equal(views[0].cpu().double(), 2 * ref[1]) and torch.equal(views[1].cpu().double(), 2 * ref[2])
    assert torch.equal(leaves[0].grad.cpu().double(), 2 * ref[0])
