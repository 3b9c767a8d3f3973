"""GPU: the non-attention kernels of the training step - la_layernorm_bwd(_res), la_transpose16, la_gemm_tn16, la_gemm_tn(_db),
la_colsum_acc, la_gelu_bwd16, la_adamw_step - on every branch of their host dispatch, against tests/train_ref.py: float64 with a
derived element-wise allowance where the kernel rounds, the exact integer result (torch.equal) where it only multiplies and adds.

Every written output lies between NaN guards, every accumulated output (dw, db, dgamma, dbeta, colsum) is pre-loaded, and every case
prints its max err / allowance under -s.  The case lists are module constants: tests/test_train_ref_cpu.py runs an fp32 model of each
kernel (clean and with planted faults) on the same shapes and data.

case -> kernel instance (by the dispatch code of csrc/train.hip):
  LN_GENERIC   (37 | 8195) x 72 -> layernorm_bwd_kernel<2>; 13 x 160, 8195 x 192, 9 x 256 unaligned -> <4>; 5125 x 384 -> <8>;
               3075 x 520 -> <16>; 1029 x 1100, 5 x 2048 -> <32>; 65535 x 8 -> <1>
  LN_VEC       E = 256, 512, 768, 1024, 1280 -> layernorm_bwd_vec_kernel<1..5>
  LN_NARROW    E = 3, 4 -> layernorm_bwd_narrow_kernel<4>; 5, 8, 16 -> <16>; 17, 32 -> <32>
  GEMM_TN      the family column of the list; TRANSPOSE kinds -> the four transpose16_kernel instances;
  GELU_BWD     "v8" -> gelu_bwd16_v8_kernel, "tail" / "unaligned" -> gelu_bwd16_kernel
"""
import pytest
import torch

from tests import train_ref as R
from tests.helpers import L, NAN, check_guards, guarded, untouched       # noqa: F401  (L: the module's fixture)

pytestmark = pytest.mark.gpu

# (rows, E[, "unaligned"]).  Rows past 4 x the workgroup cap (256 x {8, 5, 3, 1}; vector kernel x {8, 5, 3, 3, 2}) run a ragged second
# round of the grid-stride loop
LN_GENERIC = [(37, 72), (8195, 72), (13, 160), (8195, 192), (5125, 384), (3075, 520), (1029, 1100), (5, 2048), (9, 256, "unaligned"), (65535, 8)]
LN_VEC = [(7, 256), (8195, 256), (5125, 512), (3075, 768), (3075, 1024), (2051, 1280)]
LN_NARROW = [(65536, 8), (65536, 3), (262147, 4), (262147, 5), (262147, 16), (262147, 17), (262147, 32)]       # 262147 > 1024 x 256 rows
F16, BF16 = torch.float16, torch.bfloat16

TRANSPOSE_KINDS = [(torch.float32, F16), (torch.float32, BF16), (F16, F16), (BF16, BF16)]
TRANSPOSE_SHAPES = [(1, 1, 64), (63, 7, 64), (64, 64, 64), (65, 66, 128), (130, 129, 320), (577, 200, 640)]        # (R, C, Rp)

TN16_ROWS = [1, 2, 7, 63, 64, 65] + [256 + r for r in range(1, 64)]

GEMM_TN = [(255, 36, 68, "register-fed"), (256, 36, 68, "DMA 32x32 small-M"), (257, 33, 68, "register-fed (N % 4)"), (4095, 4, 4, "DMA 32x32 small-M"),
           (4096, 4, 4, "tiny<4,4>"), (4096, 5, 8, "tiny<8,8>"), (4096, 9, 8, "register-fed (N % 4)"), (4097, 28, 12, "DMA<1,1,1,1>"),
           (4097, 260, 12, "DMA<4,1,2,1>"), (4097, 12, 260, "DMA<1,4,1,2>"), (4099, 132, 260, "DMA<2,2,2,2>"), (8200, 36, 36, "DMA<2,2,2,2>"),
           (4099, 33, 65, "register-fed (unaligned)")]
COLSUM = [(1, 1), (6, 256), (63, 3), (64, 300), (1000, 300), (8200, 5), (150, 2048), (4097, 257)]
GELU_BWD = [(8000, "v8"), (8003, "tail"), (8000, "unaligned")]
ADAMW_N = [4096 * 256 + 259, 1]


def _id(c):
    return "x".join(str(v) for v in c) if isinstance(c, tuple) else str(c)


def preloaded(values):
    """(buffer, view): an accumulated destination pre-loaded with ``values`` between NaN guards."""
    buf, view = guarded(*values.shape, dtype=values.dtype)
    view.copy_(values)
    return buf, view


def judge(label, got, ref, allowance):
    ratio, first = R.check(got, ref, allowance)
    print(f"  {label}: max err / allowance {ratio:.3g}")
    assert first is None, f"{label}: element {first} is {ratio:.3g} x its allowance away from the float64 value (or not finite)"
    return ratio


# ---- LayerNorm backward -------------------------------------------------------------------------------------------------------------
def run_layernorm(L, rows, e, forms, unaligned=False):
    """forms: "plain", "gelu", "res" (add distinct from dx), "inplace" (add is dx) - the last two with out16 in fp16 and bf16."""
    d = R.ln_data(rows, e, device="cuda")
    x, dy, gamma, beta, eps = d["x"], d["dy"], d["gamma"], d["beta"], d["eps"]
    if unaligned:
        x = R.flat_offset(x, 1)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    worst = 0.0
    plain_dx = None
    for form in forms:
        gelu = form == "gelu"
        for dt in ((F16, BF16) if form in ("res", "inplace") else (None,)):
            add = d["add"] if dt is not None else None
            ref, al = R.layernorm_bwd_case64(x, dy, gamma, beta, eps, gelu, add, dt, d["dgamma0"], d["dbeta0"])
            gbuf, dgamma = preloaded(d["dgamma0"])
            bbuf, dbeta = preloaded(d["dbeta0"])
            xbuf, dx = guarded(rows, e)
            got = dict(dx=dx, dgamma=dgamma, dbeta=dbeta)
            if dt is None:
                L.layernorm_bwd(x, dy, gamma, beta, eps, gelu, dx, dgamma, dbeta)
                if form == "plain":
                    plain_dx = dx
            else:
                obuf, out16 = guarded(rows, e, dtype=dt)
                if form == "inplace":
                    dx.copy_(add)
                    add = dx
                L.layernorm_bwd_res(x, dy, gamma, beta, eps, add, dx, out16, dgamma, dbeta)
                check_guards(obuf, out16)
                got["out16"] = out16
            for buf, view in ((gbuf, dgamma), (bbuf, dbeta), (xbuf, dx)):
                check_guards(buf, view)
            tag = f"{rows} x {e} {form}" + (f" {str(dt)[6:]}" if dt is not None else "")
            for name in got:
                worst = max(worst, judge(f"{tag} {name}", got[name], ref[name], al[name]))
            if form == "inplace" and plain_dx is not None and e % 256 == 0 and e <= 1280 and not unaligned:
                # the vector kernel: bit for bit la_layernorm_bwd followed by an fp32 add and a cast
                assert torch.equal(dx, plain_dx + d["add"]) and torch.equal(out16, (plain_dx + d["add"]).to(dt)), tag
    return worst


@pytest.mark.parametrize("case", LN_GENERIC, ids=_id)
def test_layernorm_backward_generic_kernel_every_instance_and_round(L, case):
    """la_layernorm_bwd / la_layernorm_bwd_res on layernorm_bwd_kernel<1, 2, 4, 8, 16, 32>: plain, with GELU, with a distinct skip
    gradient and in place (16-bit copy in fp16 and bf16), dx / out16 / dgamma / dbeta element-wise against float64."""
    run_layernorm(L, case[0], case[1], ("plain", "gelu", "res", "inplace"), unaligned=len(case) > 2)


@pytest.mark.parametrize("case", LN_VEC, ids=_id)
def test_layernorm_backward_vector_kernel_every_width_and_second_round(L, case):
    """layernorm_bwd_vec_kernel<1..5> in the same four forms; the in-place form equals la_layernorm_bwd + fp32 add + cast bit for bit,
    on the second grid-stride round as well."""
    run_layernorm(L, case[0], case[1], ("plain", "gelu", "res", "inplace"))


@pytest.mark.parametrize("case", LN_NARROW, ids=_id)
def test_layernorm_backward_narrow_kernel_odd_widths_and_past_the_grid_cap(L, case):
    """layernorm_bwd_narrow_kernel<4, 16, 32> (one thread per row, from 65536 rows on): widths between the template sizes, rows past
    the 1024 x 256 cap; plain and with GELU."""
    run_layernorm(L, case[0], case[1], ("plain", "gelu"))


@pytest.mark.parametrize("case", LN_GENERIC + LN_VEC + LN_NARROW, ids=_id)
def test_layernorm_backward_dbeta_is_the_exact_row_sum_of_integer_dy(L, case):
    """Without GELU dbeta += sum_r dy: on integer dy (and an integer pre-load) it is exact in any order.  The allowance of a column sum
    grows with rows x sum |term| and is wide at 10^5 rows; a row, a wave or a round lost from the sum cannot hide here."""
    rows, e = case[:2]
    d = R.ln_data(rows, e, device="cuda")
    dy = R.ints(rows, e, seed=rows + e, reduce=rows, factor=1)
    db0 = R.ints(e, seed=e, reduce=rows, factor=1)
    x = R.flat_offset(d["x"], 1) if len(case) > 2 else d["x"]
    bbuf, dbeta = preloaded(db0)
    gbuf, dgamma = preloaded(d["dgamma0"])
    xbuf, dx = guarded(rows, e)
    L.layernorm_bwd(x, dy, d["gamma"], d["beta"], d["eps"], False, dx, dgamma, dbeta)
    for buf, view in ((bbuf, dbeta), (gbuf, dgamma), (xbuf, dx)):
        check_guards(buf, view)
    assert torch.equal(dbeta, R.colsum_exact(dy, db0))


def test_layernorm_backward_refusals_write_nothing(L):
    """la_layernorm_bwd_res refuses a skip gradient / 16-bit copy on the narrow form, la_layernorm_bwd E = 2049: the kernel's own
    message, and dx, out16, dgamma, dbeta untouched."""
    narrow = "la_layernorm_bwd_res: the narrow (E <= 32) form has no skip / 16-bit output"
    for rows, e, with_add, with_16, msg in ((65536, 32, True, False, narrow), (65536, 32, False, True, narrow), (65536, 32, True, True, narrow),
                                            (3, 2049, False, False, "la_layernorm_bwd: E=2049 out of range (1..2048)")):
        d = R.ln_data(rows, e, device="cuda", seed=1)
        xbuf, dx = guarded(rows, e)
        obuf, out16 = guarded(rows, e, dtype=F16)
        gbuf, dgamma = preloaded(d["dgamma0"])
        bbuf, dbeta = preloaded(d["dbeta0"])
        with pytest.raises(RuntimeError) as err:
            if with_add or with_16:
                L.layernorm_bwd_res(d["x"], d["dy"], d["gamma"], d["beta"], d["eps"], d["add"] if with_add else None, dx, out16 if with_16 else None,
                                    dgamma, dbeta)
            else:
                L.layernorm_bwd(d["x"], d["dy"], d["gamma"], d["beta"], d["eps"], False, dx, dgamma, dbeta)
        assert msg in str(err.value)
        assert untouched(xbuf) and untouched(obuf)
        check_guards(gbuf, dgamma), check_guards(bbuf, dbeta)
        assert torch.equal(dgamma, d["dgamma0"]) and torch.equal(dbeta, d["dbeta0"])


# ---- la_transpose16 ------------------------------------------------------------------------------------------------------------------
def run_transpose(L, sdt, ddt, r, c, rp, off=None):
    """off None: compact source; else the column slice starting ``off`` elements into a NaN parent 16 columns wider."""
    src = R.ints(r, c, seed=r * 7 + c, reduce=r, dtype=sdt)
    if off is not None:
        src = R.as_slice(src, off, 16)
    cs0 = R.ints(c, seed=c + 3, reduce=r)
    want, want_cs = R.transpose16_exact(src, ddt, rp, cs0)
    dbuf, dst = guarded(c, rp, dtype=ddt)
    cbuf, cs = preloaded(cs0)
    L.transpose16(src, dst, colsum=cs)
    check_guards(dbuf, dst), check_guards(cbuf, cs)
    assert torch.equal(dst[:, :r], want[:, :r]), "transposed values"
    assert torch.equal(dst.view(torch.int16)[:, r:], torch.zeros_like(dst.view(torch.int16)[:, r:])), "rows R .. Rp must hold +0"
    assert torch.equal(cs, want_cs), "column sums onto the pre-loaded values"
    dbuf2, dst2 = guarded(c, rp, dtype=ddt)
    L.transpose16(src, dst2)                                   # without column sums
    check_guards(dbuf2, dst2)
    assert torch.equal(dst2.view(torch.int16), dst.view(torch.int16))


@pytest.mark.parametrize("shape", TRANSPOSE_SHAPES, ids=_id)
@pytest.mark.parametrize("kind", TRANSPOSE_KINDS, ids=lambda k: f"{str(k[0])[6:]}-{str(k[1])[6:]}")
def test_transpose16_is_exact_on_ragged_tiles_zero_tiles_and_slices(L, kind, shape):
    """la_transpose16, all four transpose16_kernel instances, bit for bit on integers: destination, the zero rows R .. Rp (whole extra
    zero tiles at Rp = 320, a second workgroup per column tile at 10 row tiles), pre-loaded column sums; compact, as a 16-byte aligned
    column slice of a NaN parent, and as a slice 4 elements in (8 bytes off for a 16-bit source: the element-wise loads)."""
    for off in (None, 8, 4):
        run_transpose(L, kind[0], kind[1], *shape, off=off)


def test_transpose16_refuses_unsupported_conversions(L):
    src = R.ints(64, 64, seed=1, reduce=64, dtype=F16)
    dbuf, dst = guarded(64, 64, dtype=BF16)
    with pytest.raises(RuntimeError, match="la_transpose16: unsupported conversion"):
        L.transpose16(src, dst)
    dbuf2, dst2 = guarded(64, 64, dtype=F16)
    with pytest.raises(RuntimeError, match="la_transpose16: unsupported conversion"):
        L.transpose16(src.to(BF16), dst2)
    assert untouched(dbuf) and untouched(dbuf2)


# ---- la_gemm_tn16 --------------------------------------------------------------------------------------------------------------------
def tn16_operands(r, n, k, dt):
    """dy, x as column slices of NaN parents (dy 64 columns in, x at the front of a parent 8 wider), db and dw pre-loads."""
    dy = R.as_slice(R.ints(r, n, seed=r + n, reduce=r, dtype=dt), 64, 64)
    x = R.as_slice(R.ints(r, k, seed=r + 5 * k, reduce=r, dtype=dt), 0, 8)
    return dy, x, R.ints(n, seed=n + 1, reduce=r)


@pytest.mark.parametrize("dt", [F16, BF16], ids=["float16", "bfloat16"])
def test_gemm_tn16_tail_mask_at_every_residue_of_the_row_count(L, dt):
    """la_gemm_tn16 at N = K = 256, exact on integers: R = 1, 2, 7, 63, 64, 65 and 256 + r for every r in 1 .. 63 - each value the
    mask of the last 64-row step takes, in both lane halves and all four k-slices; dw and db pre-loaded and guarded."""
    for r in TN16_ROWS:
        dy, x, db0 = tn16_operands(r, 256, 256, dt)
        dw0 = R.ints(256, 256, seed=r, reduce=r)
        want, want_db = R.gemm_tn16_exact(dy, x, dw0, db0)
        wbuf, dw = preloaded(dw0)
        bbuf, db = preloaded(db0)
        L.gemm_tn16(dy, x, dw, db=db)
        check_guards(wbuf, dw), check_guards(bbuf, db)
        assert torch.equal(dw, want), f"R = {r}: dw differs in {int((dw != want).sum())} elements"
        assert torch.equal(db, want_db), f"R = {r}: db"


@pytest.mark.parametrize("dt", [F16, BF16], ids=["float16", "bfloat16"])
@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_gemm_tn16_three_chunks_and_grouped_rows(L, dt, grouped):
    """R = 577, N = 512, K = 256: three row chunks, the last of 65 rows; with gsize = 256, gstride = 261 the 5 rows between the two
    weight blocks stay bit-identical."""
    r, n, k = 577, 512, 256
    dy, x, db0 = tn16_operands(r, n, k, dt)
    gsize, gstride = (256, 261) if grouped else (0, 0)
    buf0 = R.ints(gstride + 256 if grouped else n, k, seed=9, reduce=r)
    want, want_db = R.gemm_tn16_exact(dy, x, buf0, db0, gsize, gstride)
    wbuf, dw = preloaded(buf0)
    bbuf, db = preloaded(db0)
    if grouped:
        L.gemm_tn16(dy, x, dw[:gsize], db=db, gsize=gsize, gstride=gstride)
        assert torch.equal(dw[gsize:gstride], buf0[gsize:gstride]), "the rows between the blocks"
    else:
        L.gemm_tn16(dy, x, dw, db=db)
    check_guards(wbuf, dw), check_guards(bbuf, db)
    assert torch.equal(dw, want) and torch.equal(db, want_db)


def test_gemm_tn16_refusals_write_nothing(L):
    dy, x, db0 = tn16_operands(70, 256, 256, F16)
    dw0 = R.ints(256, 256, seed=2, reduce=70)
    wbuf, dw = preloaded(dw0)
    narrow = R.ints(70, 128, seed=3, reduce=70, dtype=F16)
    odd = R.as_slice(R.ints(70, 256, seed=4, reduce=70, dtype=F16), 0, 4)           # ldy = 260: not a multiple of 8
    for msg, call in (("la_gemm_tn16: N and K must be multiples of 256", lambda: L.gemm_tn16(narrow, x, dw[:128])),
                      ("la_gemm_tn16: row strides", lambda: L.gemm_tn16(odd, x, dw)),
                      ("la_gemm_tn16: bad row grouping", lambda: L.gemm_tn16(dy, x, dw[:128], gsize=128, gstride=127))):
        with pytest.raises(RuntimeError) as err:
            call()
        assert msg in str(err.value)
    check_guards(wbuf, dw)
    assert torch.equal(dw, dw0)


# ---- la_gemm_tn / la_gemm_tn_db ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GEMM_TN, ids=_id)
def test_gemm_tn_is_exact_on_both_sides_of_every_dispatch_switch(L, case):
    """la_gemm_tn(_db), exact on integers in every family (register-fed, tiny <4,4> / <8,8>, the five LDS-DMA shapes): with and without db,
    compact and as column slices 4 columns into NaN parents; db pre-loaded and untouched when not passed."""
    m, n, k, _ = case
    for sliced in (False, True):
        dy, x = R.ints(m, n, seed=m + n, reduce=m), R.ints(m, k, seed=m + 3 * k, reduce=m)
        if sliced:
            dy, x = R.as_slice(dy, 4, 8), R.as_slice(x, 4, 8)
        dw0, db0 = R.ints(n, k, seed=n * k, reduce=m), R.ints(n, seed=n, reduce=m)
        want, want_db = R.gemm_tn_exact(dy, x, dw0, db0)
        for with_db in (False, True):
            wbuf, dw = preloaded(dw0)
            bbuf, db = preloaded(db0)
            L.gemm_tn(dy, x, dw, db if with_db else None)
            check_guards(wbuf, dw), check_guards(bbuf, db)
            assert torch.equal(dw, want), f"sliced {sliced} db {with_db}: dw differs in {int((dw != want).sum())} elements"
            assert torch.equal(db, want_db if with_db else db0), f"sliced {sliced} db {with_db}: db"


# ---- la_colsum_acc -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", COLSUM, ids=_id)
def test_colsum_acc_is_exact_compact_and_on_a_slice(L, case):
    m, n = case
    for sliced in (False, True):
        dy = R.ints(m, n, seed=m * 3 + n, reduce=m)
        if sliced:
            dy = R.as_slice(dy, 3, 5)
        out0 = R.ints(n, seed=n + 11, reduce=m)
        obuf, out = preloaded(out0)
        L.colsum_acc(dy, out)
        check_guards(obuf, out)
        assert torch.equal(out, R.colsum_exact(dy, out0)), f"sliced {sliced}"


# ---- la_gelu_bwd16 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F16, BF16], ids=["float16", "bfloat16"])
@pytest.mark.parametrize("case", GELU_BWD, ids=_id)
def test_gelu_bwd16_both_kernels_with_either_or_both_outputs(L, case, dt):
    """la_gelu_bwd16 on gelu_bwd16_v8_kernel (n % 8 == 0, aligned) and gelu_bwd16_kernel (a tail of 3, or dh 4 bytes off): both outputs,
    d32 only, d16 only; d16 == the cast of d32 bit for bit; an output that is not passed is not written."""
    n, kind = case
    pre, dh = R.gelu_data(n, dt, device="cuda")
    if kind == "unaligned":
        dh = R.flat_offset(dh, 1)
        assert dh.data_ptr() % 16 == 4
    ref = R.gelu_bwd64(pre, dh)
    al32, al16 = R.gelu_bwd_bound64(pre, dh), R.gelu_bwd_bound64(pre, dh, dt)
    for want32, want16 in ((True, True), (True, False), (False, True)):
        buf32, d32 = guarded(n)
        buf16, d16 = guarded(n, dtype=dt)
        L.gelu_bwd16(pre, dh, d32 if want32 else None, d16 if want16 else None)
        tag = f"n = {n} {kind} {str(dt)[6:]} d32 {want32} d16 {want16}"
        if want32:
            check_guards(buf32, d32)
            judge(tag + " d32", d32, ref, al32)
        else:
            assert untouched(buf32), "d32 was not passed"
        if want16:
            check_guards(buf16, d16)
            judge(tag + " d16", d16, ref, al16)
        else:
            assert untouched(buf16), "d16 was not passed"
        if want32 and want16:
            assert torch.equal(d16, d32.to(dt))


# ---- la_adamw_step -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_step_parameters_and_both_moments_past_the_grid_cap(L, n):
    """la_adamw_step against adamw64 on n = 4096 x 256 + 259 (past the grid cap) and n = 1: lr = 1e-3, weight decay 0.01, grad_scale 0.25,
    steps numbered 1, 2 and 1000 from the states the kernel itself left; p, exp_avg and exp_avg_sq each element-wise."""
    p0, m0, v0, grads = R.adamw_data(n, device="cuda")
    h = R.ADAMW_HYPER
    bufs = [preloaded(t) for t in (p0, m0, v0)]
    p, m, v = (view for _, view in bufs)
    for step, g in zip(R.ADAMW_STEPS, grads):
        args = (p.clone(), g, m.clone(), v.clone(), h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], step, h["grad_scale"])
        ref, al = R.adamw64(*args), R.adamw_bound64(*args)
        L.adamw_step(p, g, m, v, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], step, h["grad_scale"])
        for (buf, view), name, r, a in zip(bufs, ("p", "exp_avg", "exp_avg_sq"), ref, al):
            check_guards(buf, view)
            judge(f"n = {n} step {step} {name}", view, r, a)
