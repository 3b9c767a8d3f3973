"""GPU: the direct LayerNorm kernels of csrc/norm.hip - la_layernorm, la_layernorm_g, la_norm_stats - on every instance launch_ln can
reach and on the ill-conditioned rows of tests/norm_profiles.py, element-wise against fp64 on the CPU.  Outputs lie between NaN guards
(tests/helpers.guarded): the predicated tail must not write past E and nothing may stay unwritten.

E -> layernorm_kernel<T, LPR, NVT, EXACT, CS> (norm_profiles.ln_instance is launch_ln; T = the 16-bit output type, every case runs fp32,
fp16 and bf16; CS = true in test_column_sums):

    E       4      8      12     16     20     32     36      64      68      128     132     256
    LPR     1      2      4      4      8      8      16      16      32      32      64      64
    NVT     1      1      1      1      1      1      1       1       1       1       1       1
    EXACT   yes    yes    no     yes    no     yes    no      yes     no      yes     no      yes

    E       260    512    516    768    772    1024   1028    1280    1284    2044    2048
    LPR     64     64     64     64     64     64     64      64      64      64      64
    NVT     2      2      3      3      4      4      5       5       8       8       8       (8 = LN_MAXV: E > 1280)
    EXACT   no     yes    no     yes    no     yes    no      yes     no      no      yes

Unreachable: EXACT = false at LPR 1 and 2 (only E = 4 and E = 8 get there), NVT 6 and 7 (E > 1280 takes LN_MAXV), NVT > 1 below LPR 64.

Bounds (norm_profiles.allow_out32 / allow_out16), per element, from the fp64 reference of the fp32 row actually normalised:
fp32 output |got - ref| <= 2 max(C_mean, C_two) u |gamma_i| (|z_i| + sqrt rho + 1) + 2 ulp32(ref), the constants from the fp32 restatement
of tests/test_norm_profiles_cpu.py and the factor 2 for the other summation tree (wave shuffles / DPP) and 1 / sqrtf; 16-bit outputs add
half an ulp of the type and one ulp32; GELU multiplies the first term by 1.13.  Measured figures: profiles/norm_conditioning.md.

Found by test_second_input_must_share_the_row_stride: la_layernorm indexes x2 with x's row stride, and _lib.layernorm passed a
contiguous x2 beside a column slice x (wrong rows read, silently).  The wrapper now refuses the mismatch."""
import functools

import pytest
import torch

from tests import norm_profiles as NP
from tests.helpers import GUARD, L, check_guards, guarded       # noqa: F401  (L: the module's fixture)

pytestmark = pytest.mark.gpu

ROWS = 299                      # 42 or 43 rows of every profile; no multiple of 256 / LPR for any LPR
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
E_OPTIONS = (36, 132, 768)      # LPR 16 predicated, LPR 64 predicated, NVT 3 exact
U = NP.U


def eps32(eps):
    return float(torch.tensor(eps, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def weights(e):
    g = torch.Generator().manual_seed(100 + e)
    return 1.0 + 0.1 * torch.randn(e, generator=g), 0.1 * torch.randn(e, generator=g)


@functools.lru_cache(maxsize=None)
def rows_of(kind, rows, e):
    return NP.build(kind, rows, e)


@functools.lru_cache(maxsize=None)
def reference(kind, rows, e, eps, gelu=False):
    gamma, beta = weights(e)
    return NP.layernorm64(rows_of(kind, rows, e), gamma, beta, eps32(eps), gelu=gelu)


def column_slice(x_cpu, fill=1.0e30):
    """x as a column slice of a wider buffer (ldx = E + 8, 16-byte aligned), loud values around it"""
    rows, e = x_cpu.shape
    wide = torch.full((rows, e + 8), fill, device="cuda")
    wide[:, 4:4 + e] = x_cpu.cuda()
    return wide[:, 4:4 + e]


def judge(tag, got, ref64, allow):
    ratio, first = NP.worst(got, ref64, allow)
    print(f"  [ln] {tag}: max err / allowance {ratio:.3g}")
    assert first is None, f"{tag}: element {first} is {ratio:.3g} x its allowance away from the fp64 value (or not finite)"
    return ratio


def judge_outputs(tag, ref, gamma, dtype, o32=None, o16=None, o16pe=None, gelu=False, dest=None):
    a32 = NP.allow_out32(ref, gamma, gelu)
    if o32 is not None:
        judge(tag + " out32", o32, ref["out"], a32)
    if o16 is not None:
        got = o16 if dest is None else o16[dest.cuda()]
        judge(tag + " out16", got, ref["out"], NP.allow_out16(ref["out"], a32, dtype))
        if o32 is not None and dest is None:
            assert torch.equal(o16, o32.to(dtype)), f"{tag}: the 16-bit output is not the rounding of the fp32 one"
    if o16pe is not None:
        got = o16pe if dest is None else o16pe[dest.cuda()]
        judge(tag + " out16_pe", got, ref["pe"], NP.allow_out16(ref["pe"], a32 + NP.ulp32(ref["pe"]), dtype))


def run(L, x, e, eps, dtype, rows=None, want32=True, want16=True, rows16=None, wide16=1, pe=None, group=None, **kw):
    """one guarded launch -> (out32, out16, out16_pe); group = (xg, rows_per_group[, colsum_part]) takes la_layernorm_g"""
    gamma, beta = (t.cuda() for t in weights(e))
    rows = x.shape[0] if rows is None else rows
    rows16 = rows if rows16 is None else rows16
    b32, o32 = guarded(rows, e) if want32 else (None, None)
    b16, o16 = guarded(rows16, wide16 * e, dtype=dtype) if want16 else (None, None)
    bpe, ope = guarded(rows16, wide16 * e, dtype=dtype) if pe is not None else (None, None)
    dt = L.LA_F16X2 if wide16 == 2 else L._DT[dtype]
    if group is not None:
        L.layernorm_g(x, group[0], group[1], gamma, beta, eps, out32=o32, out16=o16, colsum_part=group[2] if len(group) > 2 else None, dt=dt, **kw)
    else:
        L.layernorm(x, gamma, beta, eps, out32=o32, out16=o16, out16_pe=ope, pe=pe, dt=dt, **kw)
    torch.cuda.synchronize()
    full = rows16 == rows or kw.get("window", 0) == 0
    for buf, view in ((b32, o32), (b16, o16), (bpe, ope)):
        if buf is None:
            continue
        if full or view is o32:
            check_guards(buf, view)
        else:
            n = view.numel()
            assert bool(torch.isnan(torch.cat([buf[:GUARD], buf[GUARD + n:]])).all()), "guard elements were overwritten"
    return o32, o16, ope


# =========================================================================================================================
# every reachable instance, every output type, contiguous and strided input, on the mixed matrix
# =========================================================================================================================
@pytest.mark.parametrize("dt", list(DT))
@pytest.mark.parametrize("e", NP.E_DIRECT)
def test_every_instance_on_mixed_rows(L, e, dt):
    """la_layernorm on the instance of the table above: contiguous x with eps 1e-6, x as a column slice (ldx = E + 8) with eps 1e-12."""
    dtype = DT[dt]
    gamma, _ = weights(e)
    x = rows_of("mixed", ROWS, e)
    lpr, nvt, exact = NP.ln_instance(e)
    assert ROWS % (256 // lpr) != 0
    for layout, eps in (("contiguous", 1e-6), ("column slice", 1e-12)):
        xd = x.cuda() if layout == "contiguous" else column_slice(x)
        assert (xd.stride(0) > e) == (layout != "contiguous")
        o32, o16, _ = run(L, xd, e, eps, dtype)
        ref = reference("mixed", ROWS, e, eps)
        judge_outputs(f"E={e} <{lpr},{nvt},{'exact' if exact else 'tail'}> {dt} {layout}", ref, gamma, dtype, o32, o16)


# =========================================================================================================================
# options
# =========================================================================================================================
@pytest.mark.parametrize("e", E_OPTIONS)
def test_second_input_must_share_the_row_stride(L, e):
    """x2: the row normalised is fl32(x + x2).  Contiguous pair, a pair of column slices of one stride (the same bits), and the
    mismatch - contiguous x2 beside a strided x, which the kernel would index with x's stride - is refused by the wrapper."""
    gamma, beta = weights(e)
    x = rows_of("mixed", ROWS, e)
    x2 = 0.25 * torch.randn(ROWS, e, generator=torch.Generator().manual_seed(e))
    ref = NP.layernorm64(x, gamma, beta, eps32(1e-6), x2=x2)
    o32, o16, _ = run(L, x.cuda(), e, 1e-6, torch.float16, x2=x2.cuda())
    judge_outputs(f"E={e} x2", ref, gamma, torch.float16, o32, o16)
    s32, s16, _ = run(L, column_slice(x), e, 1e-6, torch.float16, x2=column_slice(x2, fill=-1.0e30))
    assert torch.equal(s32, o32) and torch.equal(s16, o16)
    with pytest.raises(RuntimeError):
        run(L, column_slice(x), e, 1e-6, torch.float16, x2=x2.cuda())
    with pytest.raises(RuntimeError):
        run(L, x.cuda(), e, 1e-6, torch.float16, x2=column_slice(x2))


@pytest.mark.parametrize("e", E_OPTIONS)
def test_group_vector_gelu_and_position_output(L, e):
    """la_layernorm_g with groups of 33 rows (no multiple of the workgroup's 4 or 16 rows; the last group is short); GELU; out16_pe with
    pe_mod = 50 (299 = 5 x 50 + 49)."""
    gamma, beta = weights(e)
    g = torch.Generator().manual_seed(e + 1)
    x = rows_of("mixed", ROWS, e)
    xg = 0.25 * torch.randn(-(-ROWS // 33), e, generator=g)
    ref = NP.layernorm64(x, gamma, beta, eps32(1e-6), x2=xg, x2_group=33)
    for dt in ("f16", "f32"):
        o32, o16, _ = run(L, x.cuda(), e, 1e-6, DT[dt], group=(xg.cuda(), 33))
        judge_outputs(f"E={e} x2_group=33 {dt}", ref, gamma, DT[dt], o32, o16)
    for dt in ("bf16", "f32"):
        o32, o16, _ = run(L, x.cuda(), e, 1e-12, DT[dt], gelu=True)
        judge_outputs(f"E={e} gelu {dt}", reference("mixed", ROWS, e, 1e-12, True), gamma, DT[dt], o32, o16, gelu=True)
    pe = torch.randn(50, e, generator=g)
    ref = NP.layernorm64(x, gamma, beta, eps32(1e-6), pe=pe, pe_mod=50)
    for dt in ("f16", "bf16"):
        o32, o16, ope = run(L, x.cuda(), e, 1e-6, DT[dt], pe=pe.cuda(), pe_mod=50)
        judge_outputs(f"E={e} pe_mod=50 {dt}", ref, gamma, DT[dt], o32, o16, ope)


@pytest.mark.parametrize("e", E_OPTIONS)
def test_row_maps(L, e):
    """window = 4 on 7 x 9 maps (neither a multiple of the window: pad rows stay untouched); window = -1 (16-bit output into the interior
    of zero-bordered maps, plain and as plane pairs) and -2 (input rows from such maps, the borders holding 1e30)."""
    gamma, beta = weights(e)
    b, h, w, ws = 2, 7, 9, 4
    rows = b * h * w
    x = rows_of("mixed", rows, e)
    ref = reference("mixed", rows, e, 1e-6)
    a32 = NP.allow_out32(ref, gamma)
    total = NP.window_rows_total(rows, h, w, ws)
    dest = NP.window_rows(rows, h, w, ws)
    o32, o16, _ = run(L, x.cuda(), e, 1e-6, torch.float16, rows16=total, window=ws, H=h, W=w)
    judge_outputs(f"E={e} window=4", ref, gamma, torch.float16, o32, o16, dest=dest)
    pad = torch.ones(total, dtype=torch.bool)
    pad[dest] = False
    assert bool(torch.isnan(o16[pad.cuda()]).all()) and not bool(torch.isnan(o16[dest.cuda()]).any()), "window pad rows written / rows missing"
    assert torch.equal(o16[dest.cuda()], o32.half())
    # the padded maps
    maps = b * (h + 2) * (w + 2)
    dest = NP.padded_rows(rows, h, w)
    border = torch.ones(maps, dtype=torch.bool)
    border[dest] = False
    _, o16, _ = run(L, x.cuda(), e, 1e-6, torch.float16, want32=False, rows16=maps, window=-1, H=h, W=w)
    assert bool(torch.isnan(o16[border.cuda()]).all()), "window = -1 wrote the border"
    judge(f"E={e} window=-1 out16", o16[dest.cuda()], ref["out"], NP.allow_out16(ref["out"], a32, torch.float16))
    inner = o16[dest.cuda()]
    _, o2, _ = run(L, x.cuda(), e, 1e-6, torch.float16, want32=False, rows16=maps, wide16=2, window=-1, H=h, W=w)
    assert bool(torch.isnan(o2[border.cuda()]).all()) and torch.equal(o2[dest.cuda()][:, :e], inner)
    xin = torch.full((maps, e), 1.0e30)
    xin[dest] = x
    o32, o16, _ = run(L, xin.cuda(), e, 1e-6, torch.bfloat16, rows=rows, window=-2, H=h, W=w)
    judge_outputs(f"E={e} window=-2", ref, gamma, torch.bfloat16, o32, o16)


@pytest.mark.parametrize("e", E_OPTIONS)
def test_split_output_and_output_subsets(L, e):
    """LA_F16X2: hi = rn16 of the fp32 result exactly, hi + lo within max(2^-22 |v|, 2^-25) of it (lo = rn16(v - hi) is an fp16 number
    itself: below |v| = 2^-3 it is subnormal, spacing 2^-24 - no fp16 pair resolves 2^-22 |v| there).  out32 alone, out16 alone and both
    give the same bits."""
    gamma, beta = weights(e)
    x = rows_of("mixed", ROWS, e)
    ref = reference("mixed", ROWS, e, 1e-6)
    pe = torch.randn(ROWS, e, generator=torch.Generator().manual_seed(e + 2))
    o32, o2, ope = run(L, x.cuda(), e, 1e-6, torch.float16, wide16=2, pe=pe.cuda())
    judge(f"E={e} split out32", o32, ref["out"], NP.allow_out32(ref, gamma))
    assert torch.equal(o2[:, :e], o32.half()), "hi plane is not rn16 of the fp32 result"
    v = o32.double()
    slack = torch.maximum(2.0 ** -22 * v.abs(), torch.tensor(2.0 ** -25, device="cuda", dtype=torch.float64))
    err = float(((o2[:, :e].double() + o2[:, e:].double() - v).abs() / slack).max())
    print(f"  [ln] E={e} split: |hi + lo - v| at {err:.3g} of max(2^-22 |v|, 2^-25)")
    assert err <= 1.0
    vpe = (o32 + pe.cuda())
    assert torch.equal(ope[:, :e], vpe.half())
    slack = torch.maximum(2.0 ** -22 * vpe.double().abs(), torch.tensor(2.0 ** -25, device="cuda", dtype=torch.float64))
    assert float(((ope[:, :e].double() + ope[:, e:].double() - vpe.double()).abs() / slack).max()) <= 1.0
    for dt in ("f16", "bf16", "f32"):
        both32, both16, _ = run(L, x.cuda(), e, 1e-6, DT[dt])
        only32, _, _ = run(L, x.cuda(), e, 1e-6, DT[dt], want16=False)
        _, only16, _ = run(L, x.cuda(), e, 1e-6, DT[dt], want32=False)
        assert torch.equal(only32, both32) and torch.equal(only16, both16), dt
        # (recorded, not asserted: the three output types are three instantiations of the kernel, and nothing promises one contraction
        # of (v - mean) rstd gamma + beta across them)
        print(f"  [ln] E={e} {dt}: out32 differs from the LA_F16X2 launch's in {int((both32 != o32).sum())} of {o32.numel()} elements")


# =========================================================================================================================
# column sums (la_layernorm_g, CS instances)
# =========================================================================================================================
@pytest.mark.parametrize("rpg", [33, 901])
@pytest.mark.parametrize("e", [36, 132, 2048])
def test_column_sums(L, e, rpg):
    """colsum_part on a narrow (LPR 16), a predicated (LPR 64) and the LN_MAXV instance, two groups of 33 / 901 rows: every partial
    against the fp64 column sum of the stored fp32 values it covers (workgroup (g, ch) takes the rows RPB (ch + it chunks) + rl of group
    g), n fp32 additions allowed for n rows; outputs bit-identical to the launch without column sums."""
    gamma, beta = weights(e)
    groups, rows = 2, 2 * rpg
    x = rows_of("mixed", rows, e)
    xg = 0.25 * torch.randn(groups, e, generator=torch.Generator().manual_seed(e + rpg))
    ref = NP.layernorm64(x, gamma, beta, eps32(1e-6), x2=xg, x2_group=rpg)
    chunks = L.ln_cs_chunks(rpg)
    pbuf, part = guarded(groups * chunks, e)
    o32, o16, _ = run(L, x.cuda(), e, 1e-6, torch.float16, group=(xg.cuda(), rpg, part))
    check_guards(pbuf, part)
    judge_outputs(f"E={e} rpg={rpg} with column sums", ref, gamma, torch.float16, o32, o16)
    p32, p16, _ = run(L, x.cuda(), e, 1e-6, torch.float16, group=(xg.cuda(), rpg))
    assert torch.equal(p32, o32) and torch.equal(p16, o16)
    rpb = 256 // NP.ln_instance(e)[0]
    r = torch.arange(rows)
    owner = (r // rpg) * chunks + ((r % rpg) // rpb) % chunks
    stored = o32.double().cpu()
    want = torch.zeros(groups * chunks, e, dtype=torch.float64).index_add_(0, owner, stored)
    mass = torch.zeros(groups * chunks, e, dtype=torch.float64).index_add_(0, owner, stored.abs())
    n = torch.zeros(groups * chunks, dtype=torch.float64).index_add_(0, owner, torch.ones(rows, dtype=torch.float64))
    judge(f"E={e} rpg={rpg} partial sums", part, want, n[:, None] * U * mass + 1e-300)
    assert float((part.double().cpu().view(groups, chunks, e).sum(1) - stored.view(groups, rpg, e).sum(1)).abs().max()) <= \
        float((rpg * U * mass.view(groups, chunks, e).sum(1)).max())


# =========================================================================================================================
# grid-stride row loop
# =========================================================================================================================
def test_grid_stride_row_loop(L):
    """32768 + 5 rows at E = 132 (LPR 64, 4 rows a workgroup, 8192 workgroups): the last five rows come from a second round of the row
    loop and are held to the same bounds as the first."""
    e, rows = 132, 32768 + 5
    gamma, _ = weights(e)
    x = rows_of("mixed", rows, e)
    ref = reference("mixed", rows, e, 1e-6)
    o32, o16, _ = run(L, x.cuda(), e, 1e-6, torch.float16)
    judge_outputs("32773 x 132", ref, gamma, torch.float16, o32, o16)
    tail = {k: (v[-5:] if isinstance(v, torch.Tensor) and v.shape[:1] == (rows,) else v) for k, v in ref.items()}
    judge_outputs("32773 x 132, rows 32768 ..", tail, gamma, torch.float16, o32[-5:], o16[-5:])


# =========================================================================================================================
# la_norm_stats
# =========================================================================================================================
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("e", [512, 772, 1280, 2048])
def test_norm_stats(L, e, dt):
    """x16 = rn16(x) exactly; mean within 2 C_mean u (|mu| + sigma); rstd within 2 C_two u of the rstd of the variance ABOUT THE KERNEL'S
    MEAN, sigma^2 + (mu - mean)^2 (exact for the two-pass form: on a constant row of 1000.3 the mean's rounding alone moves 1 / sqrt(eps)
    by orders of magnitude, and finite garbage beyond that fails)."""
    c = NP.constants()
    x = rows_of("mixed", ROWS, e)
    mpad = -(-ROWS // 256) * 256
    for layout, eps in (("contiguous", 1e-6), ("column slice", 1e-12)):
        xd = x.cuda() if layout == "contiguous" else column_slice(x)
        xbuf, x16 = guarded(ROWS, e, dtype=DT[dt])
        mbuf, mr = guarded(mpad, 2)
        L.norm_stats(xd, eps, x16, mr)
        check_guards(xbuf, x16)
        assert bool(torch.isnan(torch.cat([mbuf[:GUARD], mbuf[GUARD + 2 * mpad:]])).all()) and bool(torch.isnan(mr[ROWS:]).all())
        assert torch.equal(x16.cpu(), x.to(DT[dt]))
        f = NP.row_figures(x, eps32(eps))
        mean, rstd = mr[:ROWS, 0].double().cpu(), mr[:ROWS, 1].double().cpu()
        judge(f"E={e} {dt} {layout} mean", mean, f["mu"], 2 * c["C_mean"] * U * (f["mu"].abs() + f["sigma"]) + 1e-300)
        about = (f["sigma"] ** 2 + (f["mu"] - mean) ** 2 + eps32(eps)).rsqrt()
        judge(f"E={e} {dt} {layout} rstd", rstd, about, 2 * c["C_two"] * U * about)


# =========================================================================================================================
# row independence
# =========================================================================================================================
@pytest.mark.parametrize("e", E_OPTIONS)
def test_rows_do_not_depend_on_their_tile_neighbours(L, e):
    """The rows of the mixed matrix come out bit-identical when each profile's rows are launched alone."""
    x = rows_of("mixed", ROWS, e)
    o32, o16, _ = run(L, x.cuda(), e, 1e-6, torch.float16)
    for kind in NP.KINDS:
        rows = NP.rows_of_kind("mixed", ROWS, kind)
        a32, a16, _ = run(L, x[rows].cuda(), e, 1e-6, torch.float16)
        assert torch.equal(a32, o32[rows.cuda()]) and torch.equal(a16, o16[rows.cuda()]), kind
