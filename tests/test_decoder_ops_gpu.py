"""GPU: the prompt-encoder / mask-decoder side of the C ABI (dec.hip, post.hip and the decoder kernels of train.hip), every
entry point called directly against a plain fp64 torch reference on the CPU evaluated from the same fp32 inputs.

Three kinds of assertion, in this order of preference:
  1. bit-exact - data movement, single fp32 adds, 16-bit copies (= the rounding of the fp32 stream written by the same call), plane pairs
     (hi = rn(v), lo = rn(v - hi)) and reductions over small integers (exact in fp32, so a dropped / doubled row is a whole-integer error);
  2. a bound derived in the test from the fp64 quantities (forward error of an n-term fp32 sum, roundings of a sin / cos argument);
  3. measured against the reference: the reference's own op sequence is ALSO evaluated in fp32 torch on the CPU, its max-norm error
     against fp64 is e32, and the kernel must stay within 4 * e32 + 1e-6 of max|ref| (``check_measured``; never computed from the kernel's
     output).  The figures observed on the MI355X are in profiles/r08_notes.md.

Every output is a view into a larger allocation whose guard elements hold a sentinel (NaN, or 7 for integer outputs): after the call the
guards must be unchanged and the view must hold no sentinel, so a tail written past its row - or not written at all - shows.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import lam_oracle as O
from tests.helpers import L, NAN, check_guards, guarded, rel_err, rint, rnd, untouched, within_1ulp

pytestmark = pytest.mark.gpu

NINF = float("-inf")
U = 2.0 ** -24               # unit roundoff of fp32


def check_measured(name, got, ref64, ref32):
    """Assertion kind 3: bound = 4 * e32 + 1e-6 of max|ref|, e32 = the error of the same ops in fp32 torch on the CPU."""
    scale = float(ref64.abs().max().clamp_min(1e-30))
    e32 = float((ref32.double() - ref64).abs().max()) / scale
    err = float((got.detach().double().cpu() - ref64).abs().max()) / scale
    bound = 4.0 * e32 + 1e-6
    print(f"[measured] {name}: e32 {e32:.3e}  kernel {err:.3e}  bound {bound:.3e}")
    assert err <= bound, (name, err, bound)


def split_planes_ok(planes, v32, d):
    """planes [rows, 2 d] fp16 = [hi | lo] of the fp32 rows v32 [rows, d]."""
    hi = v32.half()
    lo = (v32 - hi.float()).half()
    return torch.equal(planes[:, :d], hi) and torch.equal(planes[:, d:], lo)


DTS = {"f16": ("LA_F16", torch.float16), "bf16": ("LA_BF16", torch.bfloat16), "f32": ("LA_F32", torch.float32), "f16x2": ("LA_F16X2", torch.float16)}


def sixteen_ok(out16, v32, dt, d):
    """out16 is the storage form ``dt`` of the fp32 rows v32: plain rounding, an fp32 copy, or the plane pair."""
    if dt == "f16x2":
        return split_planes_ok(out16, v32, d)
    return torch.equal(out16, v32.to(DTS[dt][1]))


# =========================================================================================================================
# positional encodings and sparse tokens
# =========================================================================================================================
PE_KEY = "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"


def pe_bound(arg64):
    """|sinf / cosf (fp32 argument) - sin / cos (fp64 argument)|: about 6 fp32 roundings of the argument (8 * 2^-24 * A, A the largest
    |argument|) plus 2 ulp of sinf / cosf and the rounding of the sum with the type row (2^-22)."""
    return 8.0 * U * float(arg64.abs().max()) + 2.0 ** -22


def pe_args(gm64, coords01):
    return 2.0 * math.pi * ((2.0 * coords01 - 1.0) @ gm64)


@pytest.mark.parametrize("g,d", [(1, 2), (15, 64), (16, 256), (30, 512)])
def test_dense_pe(L, g, d):
    """la_dense_pe against O.dense_pe in fp64 (pixel centres (i + 0.5) / g, channels [sin | cos], x fastest)."""
    gm = rnd(2, d // 2, seed=300 + g)
    buf, out = guarded(g * g, d)
    L.dense_pe(gm, g, d, out)
    check_guards(buf, out)
    gm64 = gm.double().cpu()
    ref = O.dense_pe({PE_KEY: gm64}, g)[0].permute(1, 2, 0).reshape(g * g, d)
    ctr = ((torch.arange(g, dtype=torch.float32) + 0.5) / g).double()
    yy, xx = torch.meshgrid(ctr, ctr, indexing="ij")
    bound = pe_bound(pe_args(gm64, torch.stack([xx, yy], dim=-1)))
    err = float((out.double().cpu() - ref).abs().max())
    print(f"[derived] dense_pe g={g} D={d}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("d", [64, 256])
def test_point_embed(L, d):
    """la_point_embed: one call with all six token kinds and both shift values; kinds 0 / 5 are the learned rows bit for bit whatever their
    xy, the others sin / cos of 2 pi ((2x - 1) g1 + (2y - 1) g2) plus the type row, with and without the half-pixel shift."""
    n, size = 37, 1024
    special = [(0.0, 0.0), (size - 1.0, size - 1.0), (0.0, size - 1.0), (511.5, 3.25), (1022.75, 0.125), (17.0, 640.0)]
    xy = torch.zeros(n, 2)
    kind = torch.zeros(n, dtype=torch.int32)
    shift = torch.zeros(n, dtype=torch.int32)
    for i in range(n):
        pair = i // 2                              # tokens 2j and 2j + 1: same xy and kind, shift 0 / 1
        kind[i] = (pair + pair // 6) % 6           # every kind meets several coordinates
        shift[i] = i % 2
        xy[i] = torch.tensor(special[pair % len(special)]) if pair < 12 else torch.rand(2, generator=torch.Generator().manual_seed(pair)) * (size - 1)
    wild = (kind == 0) | (kind == 5)
    xy[wild] = torch.tensor([1.0e30, -5.0e8])      # never read for these kinds
    assert set(kind.tolist()) == set(range(6)) and set(shift.tolist()) == {0, 1}
    gm = rnd(2, d // 2, seed=311)
    type_emb = rnd(4, d, seed=312)
    nap, nos = rnd(d, seed=313), rnd(d, seed=314)
    buf, out = guarded(n, d)
    L.point_embed(xy.cuda(), kind.cuda(), shift.cuda(), d, size, gm, type_emb, nap, nos, out)
    check_guards(buf, out)
    got = out.cpu()
    assert torch.equal(got[kind == 0], nap.cpu().expand(int((kind == 0).sum()), d))
    assert torch.equal(got[kind == 5], nos.cpu().expand(int((kind == 5).sum()), d))
    pts = ~wild
    gm64 = gm.double().cpu()
    coords = (xy[pts].double() + 0.5 * shift[pts].double().unsqueeze(1)) / size
    ref = O.pe_encode({PE_KEY: gm64}, coords) + type_emb.double().cpu()[(kind[pts] - 1).long()]
    bound = pe_bound(pe_args(gm64, coords))
    err = float((got[pts].double() - ref).abs().max())
    print(f"[derived] point_embed D={d}: err {err:.3e} bound {bound:.3e}")
    assert err <= bound
    # the half-pixel shift: the same xy with shift 0 and 1 differ (by far more than the bound), each matching its own reference above
    even = torch.arange(0, n - 1, 2)
    even = even[pts[even]]
    assert bool(((got[even] - got[even + 1]).abs().amax(dim=1) > 2 * bound).all())


# =========================================================================================================================
# dense prompt: la_mask_embed
# =========================================================================================================================
MD = "prompt_encoder.mask_downscaling"
#              Hm   g   D  P  C   mask kinds per slot                                   flags (0 = missing slot)
MASK_GEOMS = {
    "identity": (64, 16, 64, 6, 3, ("zero", "one", "half", "random", "single", "random"), (1, 1, 1, 0, 1, 1)),     # hw = 8 blocks of 32
    "reduce15": (64, 15, 64, 4, 2, ("random", "single", "one", "half"), (1, 1, 0, 1)),                             # hw = 225: a tail of 1
    "reduce30": (128, 30, 256, 2, 1, ("half", "random"), (0, 1)),                                                  # 32 -> 30: a tail of 4
    "enlarge": (32, 16, 64, 2, 2, ("random", "one"), (1, 0)),
    "wide512": (64, 7, 512, 3, 3, ("half", "random", "single"), (1, 0, 1)),                                        # D above one 256-thread pass
}
_mask_inputs = {}
_mask_refs = {}


def mask_inputs(name):
    """fp32 CPU inputs of a geometry (built once)."""
    if name in _mask_inputs:
        return _mask_inputs[name]
    hm, g, d, p, c, kinds, flags = MASK_GEOMS[name]
    gen = torch.Generator().manual_seed(400 + sorted(MASK_GEOMS).index(name))

    def r(*shape, scale=1.0):
        return torch.randn(*shape, generator=gen) * scale

    w = {MD + ".0.weight": r(4, 1, 2, 2, scale=0.7), MD + ".0.bias": r(4, scale=0.5),
         MD + ".1.weight": 1.0 + r(4, scale=0.1), MD + ".1.bias": r(4, scale=0.1),
         MD + ".3.weight": r(16, 4, 2, 2, scale=0.25), MD + ".3.bias": r(16, scale=0.5),
         MD + ".4.weight": 1.0 + r(16, scale=0.1), MD + ".4.bias": r(16, scale=0.1),
         MD + ".6.weight": r(d, 16, 1, 1, scale=0.25), MD + ".6.bias": r(d, scale=0.5),
         "not_a_mask": r(d), "no_mask": r(d)}
    masks = torch.zeros(p, hm, hm)
    for i, k in enumerate(kinds):
        if k == "one":
            masks[i] = 1.0
        elif k == "half":
            masks[i, :, : hm // 2] = 1.0
        elif k == "random":
            masks[i] = (torch.rand(hm, hm, generator=gen) < 0.5).float()
        elif k == "single":
            masks[i, hm - 1, hm - 1] = 1.0
    inp = {"w": w, "masks": masks, "flags": torch.tensor(flags, dtype=torch.int32), "support": r(p // c, g * g, d), "class_enc": r(c, d),
           "pe": r(g * g, d)}
    _mask_inputs[name] = inp
    return inp


def mask_embed_ref(name, has_masks, has_support, has_class, dtype):
    """The reference's own order (prompt_encoder.py:516-540, 787-814): mask_downscaling, not_a_mask for the missing slots, bilinear
    resample to the grid, + support of pair p // C, + class row p % C.  -> [P, hw, D]."""
    key = (name, has_masks, has_support, has_class, dtype)
    if key in _mask_refs:
        return _mask_refs[key]
    hm, g, d, p, c, _, _ = MASK_GEOMS[name]
    inp = mask_inputs(name)
    w = {k: v.to(dtype) for k, v in inp["w"].items()}
    if has_masks:
        dense = O.mask_downscale(w, inp["masks"].to(dtype).unsqueeze(1))
        missing = (inp["flags"] == 0).view(p, 1, 1, 1)
        dense = torch.where(missing, w["not_a_mask"].view(1, d, 1, 1).expand_as(dense), dense)
    else:
        dense = w["no_mask"].view(1, d, 1, 1).expand(p, d, g, g)
    if dense.shape[-1] != g:
        dense = F.interpolate(dense, size=(g, g), mode="bilinear", align_corners=False)
    out = dense.permute(0, 2, 3, 1).reshape(p, g * g, d)
    slot = torch.arange(p)
    if has_support:
        out = inp["support"].to(dtype)[slot // c] + out
    if has_class:
        out = out + inp["class_enc"].to(dtype)[slot % c].unsqueeze(1)
    _mask_refs[key] = out
    return out


def run_mask_embed(L, name, *, has_masks=True, has_support=True, has_class=True, with16=True, dt="f16"):
    hm, g, d, p, c, _, _ = MASK_GEOMS[name]
    hw = g * g
    inp = mask_inputs(name)
    w = inp["w"]
    wlist = [w[MD + ".0.weight"], w[MD + ".0.bias"], w[MD + ".1.weight"], w[MD + ".1.bias"], w[MD + ".3.weight"], w[MD + ".3.bias"],
             w[MD + ".4.weight"], w[MD + ".4.bias"], w[MD + ".6.weight"].flatten(1), w[MD + ".6.bias"], w["not_a_mask"], w["no_mask"]]
    wlist = [t.contiguous().cuda() for t in wlist]
    masks = inp["masks"].cuda() if has_masks else None
    flags = inp["flags"].cuda() if has_masks else None
    support = inp["support"].cuda() if has_support else None
    class_enc = inp["class_enc"].cuda() if has_class else None
    pe = inp["pe"].cuda()
    code, tdt = getattr(L, DTS[dt][0]), DTS[dt][1]
    cols16 = 2 * d if dt == "f16x2" else d
    b32, src32 = guarded(p * hw, d)
    b16, src16 = guarded(p * hw, cols16, dtype=tdt) if with16 else (None, None)
    bpe, srcpe16 = guarded(p * hw, cols16, dtype=tdt) if with16 else (None, None)
    L.mask_embed(masks, flags, p, c, hm if has_masks else 0, g, d, wlist, support, class_enc, pe, src32, src16, srcpe16, code)
    check_guards(b32, src32)
    label = f"mask_embed {name} masks={has_masks} support={has_support} class={has_class} dt={dt}"
    check_measured(label, src32.view(p, hw, d), mask_embed_ref(name, has_masks, has_support, has_class, torch.float64),
                   mask_embed_ref(name, has_masks, has_support, has_class, torch.float32))
    if with16:
        check_guards(b16, src16)
        check_guards(bpe, srcpe16)
        assert sixteen_ok(src16, src32, dt, d), "src16 is not the stored form of src32"
        assert sixteen_ok(srcpe16, (src32.view(p, hw, d) + pe).view(p * hw, d), dt, d), "srcpe16 is not the stored form of src32 + pe"
    # rows without a mask: the learned row (+ class) + support in the kernel's fp32 order, bit for bit
    base = wlist[10] if has_masks else wlist[11]
    rows = torch.nonzero(inp["flags"] == 0).flatten().tolist() if has_masks else list(range(p))
    assert rows
    for s in rows:
        v = base + class_enc[s % c] if has_class else base
        v = v.unsqueeze(0) + support[s // c] if has_support else v.unsqueeze(0).expand(hw, d)
        assert torch.equal(src32.view(p, hw, d)[s], v), f"slot {s} is not not_a_mask / no_mask + class + support"


@pytest.mark.parametrize("name", list(MASK_GEOMS))
def test_mask_embed_geometries(L, name):
    """la_mask_embed at every resample regime (identity, reduction with hw % 32 tails, non-integer ratio, enlargement, D above one
    256-thread pass): the kernel resamples BEFORE the 1x1 convolution, the reference after it - the commutation is what is checked."""
    run_mask_embed(L, name)


@pytest.mark.parametrize("variant", ["no_masks", "no_support", "no_class", "no_16", "f32", "bf16", "f16x2"])
@pytest.mark.parametrize("name", ["identity", "reduce15"])
def test_mask_embed_variants(L, name, variant):
    """la_mask_embed without masks (the no_mask row), without support, without class encoding, without the 16-bit operands and in every
    storage type of the 16-bit operands."""
    kw = {"no_masks": dict(has_masks=False), "no_support": dict(has_support=False), "no_class": dict(has_class=False), "no_16": dict(with16=False),
          "f32": dict(dt="f32"), "bf16": dict(dt="bf16"), "f16x2": dict(dt="f16x2")}[variant]
    run_mask_embed(L, name, **kw)


# =========================================================================================================================
# pooling, prototypes, classification
# =========================================================================================================================
COLMEAN_SHAPES = [(3, 4096, 256), (2, 225, 64), (5, 7, 4), (1, 901, 192), (2, 33, 1024)]


@pytest.mark.parametrize("p,hw,d", COLMEAN_SHAPES)
def test_colmean(L, p, hw, d):
    """la_colmean: integer data (sums exact in fp32: a dropped, doubled or misplaced row is a whole-integer error; 1 ulp for the division)
    and N(0, 1) data against the fp64 mean.  (5, 7, 4): fewer rows than the 16 chunks; (1, 901, 192): 48 float4 lanes, 5 row groups, 16
    idle threads; (2, 33, 1024): one row in flight."""
    for kind in ("int", "normal"):
        x = rint(p, hw, d, seed=500 + hw) if kind == "int" else rnd(p, hw, d, seed=501 + hw)
        buf, out = guarded(p, d)
        sbuf, scratch = guarded(p, L.COLMEAN_SPLIT, d)
        L.colmean(x.view(p * hw, d), p, hw, d, out, scratch)
        check_guards(buf, out)
        check_guards(sbuf, scratch)
        x64 = x.double().cpu()
        if kind == "int":
            assert within_1ulp(out, x64.sum(dim=1) / hw)
        else:
            check_measured(f"colmean ({p}, {hw}, {d})", out, x64.mean(dim=1), x.cpu().mean(dim=1))


def class_mean_ref(emb, fe):
    """prompt_encoder.py:738-745 as O.prompt_encoder states it: masked mean over the M supports, divisor clamped to >= 1."""
    fe_f = fe.to(emb.dtype).unsqueeze(-1)
    denom = fe_f.sum(dim=1)
    denom = torch.where(denom == 0, torch.ones_like(denom), denom)
    return (emb * fe_f).sum(dim=1) / denom


@pytest.mark.parametrize("b,m,c,d,flags", [
    (2, 3, 4, 64, [[[0, 1, 1, 0], [0, 1, 0, 1], [0, 1, 0, 0]], [[1, 1, 0, 1], [1, 0, 0, 1], [1, 0, 0, 0]]]),   # class 0 of item 0 / class 2 of item 1: no support
    (1, 1, 1, 256, [[[1]]]),
    (1, 1, 1, 256, [[[0]]]),
])
def test_class_mean(L, b, m, c, d, flags):
    """la_class_mean: classes with every support flagged, some, and none (divisor 1, result exactly 0)."""
    fe = torch.tensor(flags, dtype=torch.uint8)
    assert tuple(fe.shape) == (b, m, c)
    emb = rnd(b, m, c, d, seed=510 + d)
    buf, out = guarded(b, c, d)
    L.class_mean(emb, fe.cuda(), b, m, c, d, out)
    check_guards(buf, out)
    none = fe.sum(dim=1) == 0
    assert bool((out.cpu()[none] == 0).all())
    check_measured(f"class_mean ({b}, {m}, {c}, {d})", out, class_mean_ref(emb.double().cpu(), fe), class_mean_ref(emb.cpu(), fe))
    # integer data: exact sums, 1 ulp for the division
    embi = rint(b, m, c, d, seed=511 + d)
    buf, out = guarded(b, c, d)
    L.class_mean(embi, fe.cuda(), b, m, c, d, out)
    check_guards(buf, out)
    assert within_1ulp(out, class_mean_ref(embi.double().cpu(), fe))


def classify_ref(feat, protos, dseg):
    """seg[b, c, pix] = protos[b, c] . feat[b, pix] (mask_decoder.py:299-314) with its autograd gradients."""
    feat = feat.clone().requires_grad_(True)
    protos = protos.clone().requires_grad_(True)
    seg = torch.einsum("bcf,bpf->bcp", protos, feat)
    seg.backward(dseg)
    return seg.detach(), feat.grad, protos.grad


@pytest.mark.parametrize("c", [1, 5, 32])
@pytest.mark.parametrize("cf", [8, 16, 32, 64])
def test_classify_and_backward(L, cf, c):
    """la_classify / la_classify_bwd called directly (dfeat written over NaN, dprotos accumulated onto a known tensor) and through
    autograd_ops.classify, against fp64 autograd: one pixel, either side of the 256-pixel block, several blocks with a tail."""
    from labelanything_amd import autograd_ops as A
    for b in (1, 3):
        for npix in (1, 255, 256, 257, 1024 + 3):
            seed = 520 + cf + c + npix + b
            feat, protos = rnd(b * npix, cf, seed=seed), rnd(b, c, cf, seed=seed + 1)
            dseg, pre = rnd(b, c, npix, seed=seed + 2), rnd(b, c, cf, seed=seed + 3)
            cpu = [t.cpu() for t in (feat.view(b, npix, cf), protos, dseg)]
            r64 = classify_ref(*[t.double() for t in cpu])
            r32 = classify_ref(*cpu)
            tag = f"Cf={cf} C={c} B={b} npix={npix}"
            bs, seg = guarded(b, c, npix)
            L.classify(feat, protos, b, npix, c, cf, seg)
            check_guards(bs, seg)
            check_measured(f"classify {tag}", seg, r64[0], r32[0])
            bf, dfeat = guarded(b * npix, cf)
            bp, dprotos = guarded(b, c, cf)
            dprotos.copy_(pre)
            L.classify_bwd(dseg, feat, protos, b, npix, c, cf, dfeat, dprotos)
            check_guards(bf, dfeat)
            check_guards(bp, dprotos)
            check_measured(f"classify_bwd dfeat {tag}", dfeat.view(b, npix, cf), r64[1], r32[1])
            check_measured(f"classify_bwd dprotos {tag}", dprotos, pre.double().cpu() + r64[2], pre.cpu() + r32[2])
            fa, pa = feat.clone().requires_grad_(True), protos.clone().requires_grad_(True)
            out = A.classify(fa, pa, b, npix, c)
            out.backward(dseg)
            assert torch.equal(out.detach(), seg)
            check_measured(f"autograd classify dfeat {tag}", fa.grad.view(b, npix, cf), r64[1], r32[1])
            check_measured(f"autograd classify dprotos {tag}", pa.grad, r64[2], r32[2])


@pytest.mark.parametrize("groups,rep,d", [(3, 7, 8), (2, 225, 64), (1, 1, 4)])
def test_row_broadcast(L, groups, rep, d):
    """la_row_broadcast: scale 1 is a copy of every group's row to its rep rows; scale 1 / rep is one fp32 multiply."""
    src = rnd(groups, d, seed=530 + rep)
    for scale in (1.0, 1.0 / rep):
        buf, out = guarded(groups * rep, d)
        L.row_broadcast(src, groups, rep, d, scale, out)
        check_guards(buf, out)
        ref = src.repeat_interleave(rep, dim=0)
        if scale != 1.0:
            ref = ref * torch.tensor(scale, dtype=torch.float32, device="cuda")
        assert torch.equal(out, ref)


def sum_bound(terms64, dim, n):
    """Forward error of ANY fp32 summation order of n terms (plus one more rounding): (n + 1) * 2^-24 * sum|terms|."""
    return (n + 1) * U * terms64.abs().sum(dim=dim)


@pytest.mark.parametrize("groups,rep,d", [(3, 7, 8), (2, 225, 64)])
def test_autograd_mean_rows(L, groups, rep, d):
    """autograd_ops.mean_rows (la_colmean forward, la_row_broadcast backward) against fp64 autograd."""
    from labelanything_amd import autograd_ops as A
    x = rnd(groups * rep, d, seed=540 + rep).requires_grad_(True)
    dy = rnd(groups, d, seed=541 + rep)
    y = A.mean_rows(x, groups, rep)
    y.backward(dy)
    torch.cuda.synchronize()
    x64 = x.detach().double().cpu().view(groups, rep, d).requires_grad_(True)
    y64 = x64.mean(dim=1)
    y64.backward(dy.double().cpu())
    assert bool(((y.detach().double().cpu() - y64.detach()).abs() <= sum_bound(x64.detach(), 1, rep) / rep).all())
    # dx = dy / rep: one multiply by the fp32 value of 1 / rep (two roundings: within 3 * 2^-24 of the fp64 quotient)
    gx = x.grad.double().cpu().view(groups, rep, d)
    assert bool(((gx - x64.grad).abs() <= 3 * U * x64.grad.abs()).all())


@pytest.mark.parametrize("rows,ymod,d", [(12, 12, 6), (12, 4, 6), (450, 225, 64)])
def test_autograd_add_rows(L, rows, ymod, d):
    """autograd_ops.add_rows in both forms (ymod == rows: plain add; ymod | rows: y repeated) against fp64 autograd."""
    from labelanything_amd import autograd_ops as A
    x = rnd(rows, d, seed=550 + rows).requires_grad_(True)
    y = rnd(ymod, d, seed=551 + rows).requires_grad_(True)
    dz = rnd(rows, d, seed=552 + rows)
    z = A.add_rows(x, y)
    z.backward(dz)
    torch.cuda.synchronize()
    x64, y64 = x.detach().double().cpu().requires_grad_(True), y.detach().double().cpu().requires_grad_(True)
    z64 = x64 + y64.repeat(rows // ymod, 1)
    z64.backward(dz.double().cpu())
    assert torch.equal(z.detach(), x.detach() + y.detach().repeat(rows // ymod, 1))    # a single fp32 add
    assert float((z.detach().double().cpu() - z64.detach()).abs().max()) <= U * float(z64.detach().abs().max())
    assert torch.equal(x.grad.cpu(), dz.cpu())
    terms = dz.double().cpu().view(rows // ymod, ymod, d)
    assert bool(((y.grad.double().cpu() - y64.grad).abs() <= sum_bound(terms, 0, rows // ymod)).all())


# =========================================================================================================================
# layout and casts
# =========================================================================================================================
@pytest.mark.parametrize("n,c,hw", [(2, 33, 65), (1, 1, 1), (3, 256, 225), (1, 768, 31)])
def test_layout_transposes(L, n, c, hw):
    """la_nchw_to_nhwc (fp32 and / or 16-bit output) and la_nhwc_to_nchw against permute, bit for bit, and their round trip.
    (1, 768, 31): the weight-transpose use of the encoder's training path."""
    x = rnd(n, c, hw, seed=600 + hw)
    ref = x.permute(0, 2, 1).contiguous()
    for dt in ("f16", "bf16", "f32"):
        code, tdt = getattr(L, DTS[dt][0]), DTS[dt][1]
        for want32, want16 in ((True, True), (True, False), (False, True)):
            b32, o32 = guarded(n, hw, c) if want32 else (None, None)
            b16, o16 = guarded(n, hw, c, dtype=tdt) if want16 else (None, None)
            L.nchw_to_nhwc(x, n, c, hw, out32=o32, out16=o16, dt=code)
            if want32:
                check_guards(b32, o32)
                assert torch.equal(o32, ref)
            if want16:
                check_guards(b16, o16)
                assert torch.equal(o16, ref.to(tdt))
    bb, back = guarded(n, c, hw)
    L.nhwc_to_nchw(ref, n, c, hw, back)
    check_guards(bb, back)
    assert torch.equal(back, x)


def run_add_cast(L, rows, d, dt, ymode):
    code, tdt = getattr(L, DTS[dt][0]), DTS[dt][1]
    x = rnd(rows, d, seed=610 + d)
    if ymode == "none":
        y, ymod, ref = None, 0, x
    elif ymode == "rows":
        y, ymod = rnd(rows, d, seed=611), 0
        ref = x + y
    else:
        ymod = ymode
        y = rnd(ymod, d, seed=612)
        ref = x + y.repeat(rows // ymod, 1)
    for want32, want16 in ((True, True), (True, False), (False, True)):
        b32, o32 = guarded(rows, d) if want32 else (None, None)
        b16, o16 = guarded(rows, 2 * d if dt == "f16x2" else d, dtype=tdt) if want16 else (None, None)
        L.add_cast(x, y, ymod, out32=o32, out16=o16, dt=code)
        if want32:
            check_guards(b32, o32)
            assert torch.equal(o32, ref)
        if want16:
            check_guards(b16, o16)
            assert sixteen_ok(o16, ref, dt, d)


@pytest.mark.parametrize("ymode", ["none", "rows", 1, 7])
@pytest.mark.parametrize("dt", list(DTS))
def test_add_cast(L, dt, ymode):
    """la_add_cast at rows x D = (7, 6): y absent, one y row per x row (ymod 0), y repeated with a period that divides the rows; a single
    fp32 add, the 16-bit / plane-pair copy is the stored form of the fp32 result."""
    run_add_cast(L, 7, 6, dt, ymode)


def test_add_cast_past_two_sweeps(L):
    """la_add_cast just past two grid-stride sweeps of its 16384-block grid (the real workload always loops): rows = 32771, D = 256."""
    rows, d = 32771, 256
    assert 2 * 16384 * 256 < rows * d < 2 * 16384 * 256 + 1024
    x, y = rnd(rows, d, seed=620), rnd(1, d, seed=621)
    b32, o32 = guarded(rows, d)
    b16, o16 = guarded(rows, d, dtype=torch.float16)
    L.add_cast(x, y, 1, out32=o32, out16=o16, dt=L.LA_F16)
    check_guards(b32, o32)
    check_guards(b16, o16)
    ref = x + y
    assert torch.equal(o32, ref) and torch.equal(o16, ref.half())


N_FLAT = 8 * 1000 + 3


def test_cast(L):
    """la_cast: fp32 -> f16 / bf16 (with and without a scale), 16-bit -> fp32, fp32 -> fp32 in place with a scale; n = 8003 (a tail of 3
    after the groups of four)."""
    x = rnd(N_FLAT, seed=630, scale=3.0)
    s32 = torch.tensor(0.3, dtype=torch.float32, device="cuda")
    for tdt in (torch.float16, torch.bfloat16):
        for scale in (1.0, 0.3):
            buf, out = guarded(N_FLAT, dtype=tdt)
            L.cast(x, out, scale)
            check_guards(buf, out)
            assert torch.equal(out, (x if scale == 1.0 else x * s32).to(tdt))
        h = x.to(tdt)
        buf, out = guarded(N_FLAT)
        L.cast(h, out)
        check_guards(buf, out)
        assert torch.equal(out, h.float())
    buf, inplace = guarded(N_FLAT)
    inplace.copy_(x)
    L.cast(inplace, inplace, 0.3)
    check_guards(buf, inplace)
    assert torch.equal(inplace, x * s32)


def test_axpy(L):
    """la_axpy: y += a x as one fused multiply-add per element (1 ulp of the fp64 value)."""
    a = 0.37
    x = rnd(N_FLAT, seed=640)
    y0 = rnd(N_FLAT, seed=641)
    buf, y = guarded(N_FLAT)
    y.copy_(y0)
    L.axpy(x, y, a)
    check_guards(buf, y)
    a32 = float(torch.tensor(a, dtype=torch.float32))
    assert within_1ulp(y, a32 * x.double().cpu() + y0.double().cpu())


def act_inputs():
    tiny = 2.0 ** -140                                      # subnormal in fp32
    edge = torch.tensor([0.0, -0.0, 10.0, -10.0, tiny, -tiny, 2.0 ** -149, 1.0, -1.0, 0.5, -0.5, 3.0, -3.0, 6.0, -6.0])
    g = torch.Generator().manual_seed(650)
    return torch.cat([edge, torch.randn(1000 - edge.numel(), generator=g) * 3.0])


def gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def test_activations(L):
    """la_act_fwd / la_act_bwd: GELU against the fp64 erf form and its derivative, ReLU exactly (derivative 0 at +-0), on inputs that
    include 0, -0.0, +-10 and subnormals."""
    xc = act_inputs()
    n = xc.numel()
    x = xc.cuda()
    dy = rnd(n, seed=651)
    x64, dy64 = xc.double(), dy.double().cpu()
    buf, y = guarded(n)
    L.act_fwd(x, y, L.ACT_GELU)
    check_guards(buf, y)
    check_measured("act_fwd gelu", y, O.gelu(x64), O.gelu(xc))
    buf, dx = guarded(n)
    L.act_bwd(x, dy, dx, L.ACT_GELU)
    check_guards(buf, dx)
    x32g = xc.clone().requires_grad_(True)
    O.gelu(x32g).backward(dy.cpu())
    check_measured("act_bwd gelu", dx, dy64 * gelu_grad64(x64), x32g.grad)
    buf, y = guarded(n)
    L.act_fwd(x, y, L.ACT_RELU)
    check_guards(buf, y)
    assert torch.equal(y, torch.relu(x))
    buf, dx = guarded(n)
    L.act_bwd(x, dy, dx, L.ACT_RELU)
    check_guards(buf, dx)
    assert torch.equal(dx, dy * (x > 0).float())
    assert bool((dx[:2] == 0).all()) and bool((xc[:2] == 0).all())                   # x = 0 and x = -0.0: derivative 0


# =========================================================================================================================
# la_attn_small: output forms
# =========================================================================================================================
@pytest.mark.parametrize("b,nq,nk,heads,hd", [(2, 5, 96, 8, 16), (2, 5, 97, 8, 16), (1, 300, 7, 4, 64), (3, 1, 130, 2, 4)])
def test_attn_small_output_forms(L, b, nq, nk, heads, hd):
    """la_attn_small with q / k / v as column slices of one fused buffer (ld != heads * hd), either side of the Nk = 96 dispatch: the
    fp32 output against fp64 softmax attention; the f16 / bf16 output of the SAME call is the rounding of the fp32 output, the LA_F32
    form a copy, the LA_F16X2 form its hi / lo planes."""
    e = heads * hd
    rows = b * max(nq, nk)
    fused = rnd(rows, 3 * e + 4, seed=700 + nk)
    q, k, v = fused[: b * nq, :e], fused[: b * nk, e:2 * e], fused[: b * nk, 2 * e:3 * e]
    assert q.stride(0) == 3 * e + 4 and not q.is_contiguous()

    def heads_of(t, n):
        return t.double().cpu().reshape(b, n, heads, hd).permute(0, 2, 1, 3)

    s = heads_of(q, nq) @ heads_of(k, nk).transpose(-1, -2) / math.sqrt(hd)
    ref = (torch.softmax(s, dim=-1) @ heads_of(v, nk)).permute(0, 2, 1, 3).reshape(b * nq, e)
    o32_of = {}
    for dt in ("f16", "bf16", "f32"):
        b32, o32 = guarded(b * nq, e)
        b16, o16 = guarded(b * nq, e, dtype=DTS[dt][1])
        L.attn_small(q, k, v, b, nq, nk, heads, hd, out16=o16, out32=o32, dt=getattr(L, DTS[dt][0]))
        check_guards(b32, o32)
        check_guards(b16, o16)
        err = rel_err(o32, ref)
        print(f"[fixed] attn_small ({b}, {nq}, {nk}, {heads}, {hd}) {dt}: {err:.3e} (2e-6)")
        assert err < 2e-6
        assert torch.equal(o16, o32.to(DTS[dt][1]))
        o32_of[dt] = o32.clone()
    bx, ox = guarded(b * nq, 2 * e, dtype=torch.float16)
    L.attn_small(q, k, v, b, nq, nk, heads, hd, out16=ox, dt=L.LA_F16X2)
    check_guards(bx, ox)
    assert split_planes_ok(ox, o32_of["f16"], e)                # the plane-pair form runs the f16 kernel with a runtime flag
    bo, only32 = guarded(b * nq, e)
    L.attn_small(q, k, v, b, nq, nk, heads, hd, out32=only32, dt=L.LA_F32)
    check_guards(bo, only32)
    assert torch.equal(only32, o32_of["f32"])


# =========================================================================================================================
# post-processing: la_post_final
# =========================================================================================================================
POST_DIMS = {32: [(50, 40), (20, 30)], 64: [(100, 80), (40, 60)]}     # item 0 is enlarged, item 1 reduced and smaller than (Hmax, Wmax) in both axes


def post_sizes(s, custom):
    sizes = []
    for oh, ow in POST_DIMS[s]:
        ph, pw = O.preprocess_shape(oh, ow, s) if custom else (s, s)
        sizes.append([oh, ow, ph, pw])
    hmax, wmax = max(h for h, _ in POST_DIMS[s]), max(w for _, w in POST_DIMS[s])
    return torch.tensor(sizes, dtype=torch.int32), hmax, wmax


def post_flags(c):
    """Item 0: class 0 switched off; item 1: the last class (for C = 1: every class of item 0, none of item 1)."""
    f = torch.ones(2, c, dtype=torch.bool)
    f[0, 0] = False
    if c > 1:
        f[1, c - 1] = False
    return f


def run_post_final(L, big, s, c, sizes, hmax, wmax, flags, want_logits=True, want_argmax=True):
    b = 2
    bl, logits = guarded(b, c, hmax, wmax) if want_logits else (None, None)
    ba, am = guarded(b, hmax, wmax, dtype=torch.int64, fill=7) if want_argmax else (None, None)
    L.post_final(big.view(b * c, s, s), b, c, s, sizes.cuda(), None if flags is None else flags.to(torch.uint8).cuda(), hmax, wmax, logits, am)
    if want_logits:
        check_guards(bl, logits)
    if want_argmax:
        check_guards(ba, am, fill=7)
    return (logits.cpu() if want_logits else None), (am.cpu() if want_argmax else None)


@pytest.mark.parametrize("custom", [True, False])
@pytest.mark.parametrize("c", [1, 3, 5])
@pytest.mark.parametrize("s", [32, 64])
def test_post_final(L, s, c, custom):
    """la_post_final against O.postprocess (fp32 F.interpolate on the CPU, whose index rule the kernel states it follows exactly): sizes
    that differ within the batch, the crop of custom_preprocess (ph, pw < S) and ph = pw = S, flag_gts absent and with a class switched
    off (class 0 included).  Argmax must agree wherever the reference's top-2 margin exceeds the logit bound."""
    big = rnd(2, c, s, s, seed=800 + s + c)
    sizes, hmax, wmax = post_sizes(s, custom)
    assert (sizes[0, 0] > sizes[0, 2]) and (sizes[1, 0] < sizes[1, 2]) and bool(custom == bool((sizes[:, 2:] < s).any()))
    geo = O.LamGeometry(image_size=s, custom_preprocess=custom)
    dims = torch.tensor(POST_DIMS[s]).view(2, 1, 2)
    bound = 4.0 * 2.0 ** -23 * float(big.abs().max())           # five roundings of a convex combination on either side
    for flags in (None, post_flags(c)):
        logits, am = run_post_final(L, big, s, c, sizes, hmax, wmax, flags)
        ref = O.postprocess(geo, big.cpu().clone(), dims, flags)
        fin = torch.isfinite(ref)
        err = rel_err(logits, ref) * float(ref[fin].abs().max()) if fin.any() else rel_err(logits, ref)
        top2 = ref.topk(2, dim=1).values if c > 1 else None
        dead = (ref == NINF).all(dim=1)                          # every class -inf: torch.argmax and the kernel both say 0
        clear = ((top2[:, 0] - top2[:, 1]) > bound) | dead if c > 1 else torch.ones_like(dead)
        excluded = int((~clear).sum())
        print(f"[derived] post_final S={s} C={c} custom={custom} flags={flags is not None}: err {err:.3e} bound {bound:.3e}, "
              f"{excluded} of {clear.numel()} pixels inside the margin")
        assert err <= bound
        assert excluded <= 0.001 * clear.numel()
        assert torch.equal(am[clear], ref.argmax(dim=1)[clear])


def test_post_final_ties_and_output_selection(L):
    """la_post_final's exact cases: two classes with the identical plane -> the lower index; padding pixels -> class 0, also with class 0
    switched off (everything -inf: index 0); logits only, argmax only and both give the same values."""
    s, c = 32, 3
    big = rnd(2, c, s, s, seed=810)
    big[:, 1] = big[:, 0]
    sizes, hmax, wmax = post_sizes(s, True)
    pad = torch.ones(2, hmax, wmax, dtype=torch.bool)
    for i, (oh, ow) in enumerate(POST_DIMS[s]):
        pad[i, :oh, :ow] = False
    assert pad[1].any() and not pad[0].any()
    for flags in (None, post_flags(c)):
        logits, am = run_post_final(L, big, s, c, sizes, hmax, wmax, flags)
        only_logits, _ = run_post_final(L, big, s, c, sizes, hmax, wmax, flags, want_argmax=False)
        _, only_am = run_post_final(L, big, s, c, sizes, hmax, wmax, flags, want_logits=False)
        assert torch.equal(only_am, am)
        assert torch.equal(torch.isneginf(only_logits), torch.isneginf(logits))
        assert torch.equal(only_logits[torch.isfinite(logits)], logits[torch.isfinite(logits)])
        assert bool((am[pad] == 0).all())
        if flags is None:
            assert torch.equal(logits[:, 0][~pad], logits[:, 1][~pad]) and not bool((am == 1).any())
            assert bool((logits[:, 0][pad] == 0).all()) and bool((logits[:, 1:][pad.unsqueeze(1).expand(2, c - 1, hmax, wmax)] == NINF).all())
            assert torch.equal(am, logits.argmax(dim=1))                 # first maximal index, as torch.argmax
        else:
            assert bool((logits[0, 0] == NINF).all()) and bool((logits[1, c - 1] == NINF).all())
            inside0 = ~pad[0]
            assert not bool((am[0][inside0] == 0).any())                 # class 0 is off where there are finite logits ...
            assert bool((am[1][~pad[1]] != c - 1).all())
    # ... and padding with class 0 switched off is all -inf: index 0
    off = torch.ones(2, c, dtype=torch.bool)
    off[1, 0] = False
    logits, am = run_post_final(L, big, s, c, sizes, hmax, wmax, off)
    assert bool((logits[1][:, pad[1]] == NINF).all()) and bool((am[1][pad[1]] == 0).all())


# =========================================================================================================================
# rejected arguments: the argument check returns before any launch
# =========================================================================================================================
def test_rejected_arguments(L):
    """Every refused shape raises through _lib._check and leaves the NaN-filled output untouched (nothing is launched)."""
    def nan(*shape, dtype=torch.float32):
        return torch.full(shape, NAN, dtype=dtype, device="cuda")

    z = rnd(64, 64, seed=900)
    seg = nan(1, 2, 4)
    with pytest.raises(RuntimeError, match="la_classify"):
        L.classify(z[:4, :12].contiguous(), z[:2, :12].contiguous(), 1, 4, 2, 12, seg)
    assert untouched(seg)
    dfeat, dprotos = nan(4, 8), nan(33, 8)
    with pytest.raises(RuntimeError, match="la_classify_bwd"):
        L.classify_bwd(z[:33, :4].contiguous(), z[:4, :8].contiguous(), z[:33, :8].contiguous(), 1, 4, 33, 8, dfeat, dprotos)
    assert untouched(dfeat) and untouched(dprotos)
    for d in (6, 1028):
        x = rnd(2 * 3, d, seed=901)
        out, scratch = nan(2, d), nan(2, L.COLMEAN_SPLIT, d)
        with pytest.raises(RuntimeError, match="la_colmean"):
            L.colmean(x, 2, 3, d, out, scratch)
        assert untouched(out) and untouched(scratch)
    out = nan(2 * 3, 6)
    with pytest.raises(RuntimeError, match="la_row_broadcast"):
        L.row_broadcast(z[:2, :6].contiguous(), 2, 3, 6, 1.0, out)
    assert untouched(out)
    out = nan(4, 24)
    qkv = rnd(4, 72, seed=902)
    with pytest.raises(RuntimeError, match="la_attn_small"):
        L.attn_small(qkv[:, :24], qkv[:, 24:48], qkv[:, 48:], 1, 4, 4, 2, 12, out32=out, dt=L.LA_F32)
    assert untouched(out)
    out = nan(4, 4)
    q6, kv = rnd(4, 6, seed=903), rnd(4, 8, seed=904)
    with pytest.raises(RuntimeError, match="la_attn_small"):
        L.attn_small(q6[:, :4], kv[:, :4], kv[:, 4:], 1, 4, 4, 1, 4, out32=out, dt=L.LA_F32)
    assert untouched(out)
    g, d, p = 4, 8, 1
    wl = [rnd(n, seed=905) for n in (16, 4, 4, 4, 256, 16, 16, 16, d * 16, d, d, d)]
    src32, src16 = nan(p * g * g, d), nan(p * g * g, d, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="la_mask_embed"):
        L.mask_embed(torch.zeros(p, 30, 30, device="cuda"), torch.ones(p, dtype=torch.int32, device="cuda"), p, 1, 30, g, d, wl, None, None,
                     rnd(g * g, d, seed=906), src32, src16, None, L.LA_F16)
    assert untouched(src32) and untouched(src16)
