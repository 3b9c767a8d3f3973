"""GPU: the four kernels of the two-level classification head called directly - la_classify_wide / la_classify_wide_bwd and
la_level_reduce / la_level_reduce_bwd (csrc/levels.hip) - against float64 torch on the CPU (tests/levels_ref.py and its autograd) evaluated
from the same fp32 inputs.  Conventions of tests/test_multi_embedding_gpu.py: outputs sit between NaN guards and are written over NaN;
refused arguments leave NaN-filled outputs untouched.

Two kinds of input.
  Small integers.  Every product and every partial sum - in ANY order - is then a multiple of 1/64 (the enlargement's weights are
    products of eighths) whose magnitude stays below 2^24 / 64: the test shows that on the CPU by evaluating the same formula on the
    absolute values.  Such numbers are exact in fp32, so forward, dcls0, dcls1, dw, dbias (and the wide classify with its gradients) must
    EQUAL the float64 result: a dropped, doubled, clamped-instead-of-zeroed or transposed tap is a whole-unit error.
  Normal inputs.  U = 2^-24.  A sum of n terms in any order, one more rounding per term for the product and one for a final operation, errs
    by at most (n + 2) U times the same formula on absolute values.  n = 18 + 4 for the head (18 taps; the 4 enlargement products feed a
    tap), D for the wide classify, C for dimg, Npix for dtok, 9 for dcls0, 9 + 64 for dcls1 (a 9-tap sum inside a sum over the 8 x 8 fine
    pixels that read a coarse pixel), the number of pixels of the whole batch (+ 4) for dw and dbias.  Printed as [derived].
"""
import pytest
import torch

from tests import levels_ref as R
from tests.helpers import L, NAN, check_guards, guarded, guarded_zero, untouched

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 24 / 64

SHAPES = [(2, 3, 5, 7),        # odd, not square, smaller than a tile, several planes
          (1, 2, 16, 16),      # the fixture's geometry: 2 x 2 tiles
          (1, 1, 30, 30),      # the Pascal grid: 4 x 4 tiles, the last ones partial
          (1, 1, 1, 1)]        # every source index clamps
WIDTHS = [64, 256, 512]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rnd(*shape, seed=0, scale=1.0):
    return scale * torch.randn(*shape, generator=gen(seed))


def rint(*shape, seed=0, lo=-4, hi=5):
    return torch.randint(lo, hi, shape, generator=gen(seed)).float()


# =========================================================================================================================
# la_level_reduce / la_level_reduce_bwd
# =========================================================================================================================
def head_inputs(shape, kind, seed):
    b, c, gh, gw = shape
    if kind == "int":
        return (rint(b, c, 4 * gh, 4 * gw, seed=seed), rint(b, c, gh, gw, seed=seed + 1), rint(1, 2, 3, 3, seed=seed + 2, lo=-3, hi=4),
                rint(1, seed=seed + 3), rint(b, c, 4 * gh, 4 * gw, seed=seed + 4, lo=-2, hi=3))
    return (rnd(b, c, 4 * gh, 4 * gw, seed=seed, scale=5.0), rnd(b, c, gh, gw, seed=seed + 1, scale=30.0),      # the scales of the model's levels
            rnd(1, 2, 3, 3, seed=seed + 2, scale=0.3), rnd(1, seed=seed + 3, scale=0.3), rnd(b, c, 4 * gh, 4 * gw, seed=seed + 4))


def head_ref(cls0, cls1, w, bias, dseg):
    """float64 forward and gradients of tests/levels_ref.level_reduce by autograd."""
    leaves = [t.double().clone().requires_grad_(True) for t in (cls0, cls1, w, bias)]
    seg = R.level_reduce(*leaves)
    seg.backward(dseg.double())
    return (seg.detach(), *[t.grad for t in leaves])


def run_head(L, shape, cls0, cls1, w, bias, dseg):
    b, c, gh, gw = shape
    dev = [t.cuda().contiguous() for t in (cls0, cls1, w, bias, dseg)]
    bs, seg = guarded(b, c, 4 * gh, 4 * gw)
    L.level_reduce(dev[0], dev[1], dev[2], dev[3], b, c, gh, gw, seg)
    check_guards(bs, seg)
    b0, d0 = guarded(b, c, 4 * gh, 4 * gw)
    b1, d1 = guarded(b, c, gh, gw)
    bw, dw = guarded_zero(18)
    bb, db = guarded_zero(1)
    L.level_reduce_bwd(dev[4], dev[0], dev[1], dev[2], b, c, gh, gw, d0, d1, dw, db)
    for buf, view in ((b0, d0), (b1, d1), (bw, dw), (bb, db)):
        check_guards(buf, view)
    return [t.cpu() for t in (seg, d0, d1, dw.view(1, 2, 3, 3), db)]


NAMES = ("seg", "dcls0", "dcls1", "dw", "dbias")


@pytest.mark.parametrize("shape", SHAPES)
def test_level_reduce_integers_are_exact(L, shape):
    cls0, cls1, w, bias, dseg = head_inputs(shape, "int", seed=1000 + sum(shape))
    # the CPU side of the argument: the formulas on absolute values bound every partial sum, in any order
    mags = head_ref(cls0.abs(), cls1.abs(), w.abs(), bias.abs(), dseg.abs())
    worst = max(float(m.max()) for m in mags)
    print(f"{shape}: largest sum of magnitudes {worst:.1f} (limit {EXACT_LIMIT:.0f})")
    assert worst < EXACT_LIMIT
    ref = head_ref(cls0, cls1, w, bias, dseg)
    for r in ref:
        assert torch.equal(r * 64, (r * 64).round())                       # multiples of 1/64
    got = run_head(L, shape, cls0, cls1, w, bias, dseg)
    for name, g, r in zip(NAMES, got, ref):
        assert torch.equal(g.double(), r.reshape(g.shape)), name


@pytest.mark.parametrize("shape", SHAPES)
def test_level_reduce_normal_inputs_within_the_derived_bound(L, shape):
    b, c, gh, gw = shape
    cls0, cls1, w, bias, dseg = head_inputs(shape, "normal", seed=2000 + sum(shape))
    ref = head_ref(cls0, cls1, w, bias, dseg)
    mags = head_ref(cls0.abs(), cls1.abs(), w.abs(), bias.abs(), dseg.abs())
    npix = b * c * 16 * gh * gw
    terms = {"seg": 18 + 4, "dcls0": 9, "dcls1": 9 + 64, "dw": npix + 4, "dbias": npix}
    got = run_head(L, shape, cls0, cls1, w, bias, dseg)
    for name, g, r, m in zip(NAMES, got, ref, mags):
        bound = (terms[name] + 2) * U * m.reshape(g.shape)
        err = (g.double() - r.reshape(g.shape)).abs()
        print(f"[derived] level_reduce {shape} {name}: err {float(err.max()):.3e} bound {float(bound.max()):.3e} "
              f"(n = {terms[name]}, scale {float(r.abs().max()):.3e})")
        assert bool((err <= bound).all()), name


def test_one_plane_alone_is_bit_identical_to_the_plane_in_a_batch(L):
    shape = (2, 3, 5, 7)
    b, c, gh, gw = shape
    cls0, cls1, w, bias, dseg = head_inputs(shape, "normal", seed=31)
    seg, d0, d1, _, _ = run_head(L, shape, cls0, cls1, w, bias, dseg)
    for bi, ci in ((0, 0), (1, 2), (0, 1)):
        one = [t[bi:bi + 1, ci:ci + 1].contiguous() for t in (cls0, cls1)] + [w, bias, dseg[bi:bi + 1, ci:ci + 1].contiguous()]
        s1, e0, e1, _, _ = run_head(L, (1, 1, gh, gw), *one)
        assert torch.equal(s1[0, 0], seg[bi, ci]) and torch.equal(e0[0, 0], d0[bi, ci]) and torch.equal(e1[0, 0], d1[bi, ci])
    # a neighbouring plane full of NaN changes nothing: halos never read another plane
    poisoned0, poisoned1 = cls0.clone(), cls1.clone()
    poisoned0[0, 0], poisoned1[0, 0], poisoned0[1, 0], poisoned1[1, 0] = NAN, NAN, NAN, NAN
    poisoned0[0, 2], poisoned1[0, 2] = NAN, NAN
    dev = [t.cuda() for t in (poisoned0, poisoned1, w, bias)]
    bs, out = guarded(b, c, 4 * gh, 4 * gw)
    L.level_reduce(*dev, b, c, gh, gw, out)
    torch.cuda.synchronize()
    assert torch.equal(out[0, 1].cpu(), seg[0, 1]) and torch.equal(out[1, 1].cpu(), seg[1, 1]) and torch.equal(out[1, 2].cpu(), seg[1, 2])


@pytest.mark.parametrize("shape", SHAPES)
def test_zero_weights_isolate_a_level(L, shape):
    """w[1] = 0: the result is conv3x3(cls0, w[0]) + bias - to the bit whatever cls1 holds (the kernel's level-1 taps are fmaf(0, u, acc)),
    EQUAL to the float64 convolution on integers, and within the 9-term bound of it otherwise.  w[0] = 0 isolates the coarse level."""
    import torch.nn.functional as F
    b, c, gh, gw = shape
    for kind in ("int", "normal"):
        cls0, cls1, w, bias, dseg = head_inputs(shape, kind, seed=3000 + sum(shape))
        w_fine = w.clone()
        w_fine[0, 1] = 0
        a = run_head(L, shape, cls0, cls1, w_fine, bias, dseg)
        other = run_head(L, shape, cls0, 7.0 * cls1.flip(-1) + 3.0, w_fine, bias, dseg)
        assert torch.equal(a[0], other[0]) and torch.equal(a[1], other[1])
        assert bool((a[2] == 0).all())                                            # no gradient reaches the coarse level
        conv = lambda x, k, bb: F.conv2d(x.double().reshape(b * c, 1, 4 * gh, 4 * gw), k.double().reshape(1, 1, 3, 3), bb, padding=1) \
            .reshape(b, c, 4 * gh, 4 * gw)
        want = conv(cls0, w[0, 0], bias.double())
        if kind == "int":
            assert torch.equal(a[0].double(), want)
        else:
            bound = (9 + 2) * U * conv(cls0.abs(), w[0, 0].abs(), bias.double().abs())
            assert bool(((a[0].double() - want).abs() <= bound).all())
        w_coarse = w.clone()
        w_coarse[0, 0] = 0
        z = run_head(L, shape, cls0, cls1, w_coarse, bias, dseg)
        other = run_head(L, shape, 5.0 * cls0.flip(-2) - 1.0, cls1, w_coarse, bias, dseg)
        assert torch.equal(z[0], other[0]) and torch.equal(z[2], other[2])
        assert bool((z[1] == 0).all())
        want = conv(R.enlarge4(cls1.double()), w[0, 1], bias.double())
        if kind == "int":
            assert torch.equal(z[0].double(), want)
        else:
            bound = (9 + 4 + 2) * U * conv(R.enlarge4(cls1.double().abs()), w[0, 1].abs(), bias.double().abs())
            assert bool(((z[0].double() - want).abs() <= bound).all())


def test_edge_rules_are_not_mixed(L):
    """A constant coarse plane enlarges to the same constant everywhere (source indices CLAMP), and the 3x3 sees zeros outside the fine
    plane (taps are ZEROED): with w[1] = ones the interior is 9 v, an edge 6 v, a corner 4 v - clamped taps would give 9 v everywhere, an
    enlargement that read zeros beyond the coarse plane less than 6 v / 4 v on the border."""
    b, c, gh, gw = 1, 1, 3, 5
    v = 3.0
    w = torch.zeros(1, 2, 3, 3)
    w[0, 1] = 1.0
    seg = run_head(L, (b, c, gh, gw), torch.zeros(b, c, 4 * gh, 4 * gw), torch.full((b, c, gh, gw), v), w, torch.zeros(1),
                   torch.ones(b, c, 4 * gh, 4 * gw))[0][0, 0]
    want = torch.full((4 * gh, 4 * gw), 9 * v)
    want[0, :], want[-1, :], want[:, 0], want[:, -1] = 6 * v, 6 * v, 6 * v, 6 * v
    want[0, 0], want[0, -1], want[-1, 0], want[-1, -1] = 4 * v, 4 * v, 4 * v, 4 * v
    assert torch.equal(seg, want)


def test_level_reduce_refuses_bad_arguments(L):
    buf, seg = guarded(1, 1, 8, 8)
    z = torch.zeros(64, device="cuda")
    with pytest.raises(ValueError, match="cls1"):
        L.level_reduce(z, z, z[:18], z[:1], 1, 1, 2, 2, seg)                     # cls1 must hold 4 values
    with pytest.raises(ValueError, match="w must hold 18"):
        L.level_reduce(z, z[:4], z[:9], z[:1], 1, 1, 2, 2, seg)
    with pytest.raises(RuntimeError, match="la_level_reduce"):
        L.level_reduce(z[:0], z[:0], z[:18], z[:1], 0, 1, 2, 2, seg[:0])
    assert untouched(buf)


# =========================================================================================================================
# la_classify_wide / la_classify_wide_bwd
# =========================================================================================================================
def wide_ref(tok, img, dseg):
    t, i = tok.double().clone().requires_grad_(True), img.double().clone().requires_grad_(True)
    seg = R.coarse_classify(t, i)
    seg.backward(dseg.double())
    return seg.detach(), i.grad, t.grad


def run_wide(L, b, npix, c, d, tok, img, dseg):
    dev = [t.cuda().contiguous() for t in (tok, img, dseg)]
    bs, seg = guarded(b, c, npix)
    L.classify_wide(dev[0], dev[1], b, npix, c, d, seg)
    check_guards(bs, seg)
    bi, dimg = guarded(b, npix, d)
    bt, dtok = guarded_zero(b, c, d)
    L.classify_wide_bwd(dev[2], dev[0], dev[1], b, npix, c, d, dimg, dtok)
    check_guards(bi, dimg)
    check_guards(bt, dtok)
    return seg.cpu(), dimg.cpu(), dtok.cpu()


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("shape", SHAPES + [(1, 11, 9, 9)])                  # 11 classes: two groups of 8
def test_classify_wide_and_backward(L, shape, d):
    b, c, gh, gw = shape
    npix = gh * gw
    for kind in ("int", "normal"):
        seed = 4000 + sum(shape) + d
        if kind == "int":
            tok, img, dseg = rint(b, c, d, seed=seed), rint(b, npix, d, seed=seed + 1), rint(b, c, npix, seed=seed + 2)
        else:
            tok, img, dseg = rnd(b, c, d, seed=seed, scale=2.0), rnd(b, npix, d, seed=seed + 1), rnd(b, c, npix, seed=seed + 2)
        ref = wide_ref(tok, img, dseg)
        mags = wide_ref(tok.abs(), img.abs(), dseg.abs())
        got = run_wide(L, b, npix, c, d, tok, img, dseg)
        if kind == "int":
            assert max(float(m.max()) for m in mags) < 2.0 ** 24                 # integers below 2^24: exact in any order
            for name, g, r in zip(("seg", "dimg", "dtok"), got, ref):
                assert torch.equal(g.double(), r), name
        else:
            for name, n, g, r, m in zip(("seg", "dimg", "dtok"), (d, c, npix), got, ref, mags):
                bound = (n + 2) * U * m
                err = (g.double() - r).abs()
                print(f"[derived] classify_wide {shape} D={d} {name}: err {float(err.max()):.3e} bound {float(bound.max()):.3e} (n = {n})")
                assert bool((err <= bound).all()), name
            # one image alone: bit-identical rows (dtok is folded by atomics: its order is not fixed, the others' is)
            last = b - 1
            s1, i1, _ = run_wide(L, 1, npix, c, d, tok[last:], img[last:], dseg[last:])
            assert torch.equal(s1[0], got[0][last]) and torch.equal(i1[0], got[1][last])


@pytest.mark.parametrize("d,c", [(96, 2), (1088, 2), (256, 33)])
def test_classify_wide_refuses(L, d, c):
    b, npix = 1, 4
    tok, img, dseg = torch.zeros(b, c, d, device="cuda"), torch.zeros(b, npix, d, device="cuda"), torch.zeros(b, c, npix, device="cuda")
    bs, seg = guarded(b, c, npix)
    with pytest.raises(RuntimeError, match=r"la_classify_wide: (width D=|C=33 classes)"):
        L.classify_wide(tok, img, b, npix, c, d, seg)
    bi, dimg = guarded(b, npix, d)
    bt, dtok = guarded(b, c, d)
    with pytest.raises(RuntimeError, match=r"la_classify_wide_bwd: (width D=|C=33 classes)"):
        L.classify_wide_bwd(dseg, tok, img, b, npix, c, d, dimg, dtok)
    assert untouched(bs) and untouched(bi) and untouched(bt)
    with pytest.raises(ValueError, match="seg must hold"):
        L.classify_wide(tok, img, b, npix, c, d, seg[:, :1])


# =========================================================================================================================
# the autograd nodes
# =========================================================================================================================
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 2, 16, 16)])
def test_autograd_nodes_return_what_the_kernel_pairs_return(L, shape):
    """Written outputs (seg, dcls0, dcls1, dimg) are compared bit for bit on both kinds of input; the ACCUMULATED ones (dw, dbias, dtok:
    atomics, no fixed order) bit for bit on integer inputs, where every order gives the same bits, and on normal inputs against float64
    within the derived bound of the kernel tests (the nodes run without a gradient sink here: dw / dbias go through their temporaries)."""
    from labelanything_amd import autograd_ops as A
    b, c, gh, gw = shape
    d, npix = 64, gh * gw
    for kind in ("int", "normal"):
        cls0, cls1, w, bias, dseg = head_inputs(shape, kind, seed=5000 + sum(shape))
        raw = run_head(L, shape, cls0, cls1, w, bias, dseg)
        leaves = [t.cuda().requires_grad_(True) for t in (cls0, cls1, w, bias)]
        seg = A.level_reduce(*leaves, b, c, gh, gw)
        seg.backward(dseg.cuda())
        torch.cuda.synchronize()
        got = [seg.detach().cpu()] + [t.grad.cpu() for t in leaves]
        for name, g, r in zip(NAMES, got, raw):
            if kind == "int" or name in ("seg", "dcls0", "dcls1"):
                assert torch.equal(g, r.reshape(g.shape)), (kind, name)
        if kind == "normal":
            ref = head_ref(cls0, cls1, w, bias, dseg)
            mags = head_ref(cls0.abs(), cls1.abs(), w.abs(), bias.abs(), dseg.abs())
            terms = b * c * 16 * gh * gw + 4
            for i in (3, 4):
                err, bound = (got[i].double() - ref[i].reshape(got[i].shape)).abs(), (terms + 2) * U * mags[i].reshape(got[i].shape)
                print(f"[derived] node {shape} {NAMES[i]}: err {float(err.max()):.3e} bound {float(bound.max()):.3e}")
                assert bool((err <= bound).all()), NAMES[i]
        if kind == "int":
            tok, img, ds = rint(b, c, d, seed=61), rint(b, npix, d, seed=62), rint(b, c, npix, seed=63)
        else:
            tok, img, ds = rnd(b, c, d, seed=61), rnd(b, npix, d, seed=62), rnd(b, c, npix, seed=63)
        raw = run_wide(L, b, npix, c, d, tok, img, ds)
        ti, ii = tok.reshape(b * c, d).cuda().requires_grad_(True), img.reshape(b * npix, d).cuda().requires_grad_(True)
        seg = A.classify_wide(ii, ti, b, npix, c)
        seg.backward(ds.cuda())
        torch.cuda.synchronize()
        assert torch.equal(seg.detach().cpu(), raw[0]) and torch.equal(ii.grad.cpu().view(b, npix, d), raw[1])
        if kind == "int":
            assert torch.equal(ti.grad.cpu().view(b, c, d), raw[2])
        else:
            ref, mags = wide_ref(tok, img, ds), wide_ref(tok.abs(), img.abs(), ds.abs())
            err, bound = (ti.grad.cpu().view(b, c, d).double() - ref[2]).abs(), (npix + 2) * U * mags[2]
            print(f"[derived] node {shape} dtok: err {float(err.max()):.3e} bound {float(bound.max()):.3e}")
            assert bool((err <= bound).all())
