"""CPU: la_gemm_plan against a literal table of what la_gemm launched BEFORE the plan existed.

Every row is one call and the launch the commit before gemm_plan.h made for it: kernel template with its template arguments, grid and
workgroup size come from one kernel trace of those calls on an MI355X (256 CUs) at that commit (profiles/r11_gemm_dispatch.md holds the raw
list); what a trace does not show - tile grouping, K chunks, dynamic LDS - and the rows marked HAND (shapes beside the traced ones) were read
off that commit's launchers.  Nothing here is produced by the code under test.  The table straddles every threshold of the dispatch.
"""
import pytest

from labelanything_amd import _lib as L

NCU = 256
A, W, BIAS, RES, O32, O16, VT, AUX, NSO, RVEC, NSI, NCOL = (0x7000_0000_0000 + i * 0x10_0000_0000 for i in range(12))      # 16-byte aligned "addresses"
F16, BF16, F32 = L.LA_F16, L.LA_BF16, L.LA_F32
BIG = 131072
NT, DMA128, DMA256x128, T256, T256P, T256Q, T256W, F32_N32, F32_N128, F32_SMALL, SKINNY = range(11)
LDS = {NT: 65536, DMA128: 67584, DMA256x128: 73728, (T256, 1): 139264, (T256, 2): 147456, (T256P, 1): 151552, (T256P, 2): 163840, T256Q: 151552,
       T256W: 163840, F32_N32: 40960, F32_N128: 67584, F32_SMALL: 0, SKINNY: 0}


def plan(kernel, grid, epi=0, planes=1, direct=0, ragged=0, gm=None, ksplit=1, kchunk=None, block=None):
    """Expected LaGemmPlan fields; gm / block / lds of the kernel family unless given (kchunk None = K)."""
    if gm is None:
        gm = {DMA128: 8, DMA256x128: 8, T256: 2, T256P: 2, T256Q: 2, T256W: 2}.get(kernel, 0)
    if block is None:
        block = 512 if kernel in (T256, T256P, T256Q) else 256
    return dict(kernel=kernel, epi=epi, planes=planes, direct=direct, ragged=ragged, gm=gm, ksplit=ksplit, kchunk=kchunk, grid=grid, block=block,
                lds_bytes=LDS.get((kernel, planes), LDS.get(kernel)))


def call(m, n, k, dt=F16, a=A, lda=None, ldw=None, variant=2, **epi):
    return dict(m=m, n=n, k=k, dt=dt, a=a, lda=k if lda is None else lda, ldw=k if ldw is None else ldw, variant=variant, epi=epi)


def p16(m, n, k, **kw):
    return call(m, n, k, bias=BIAS, out16=O16, **kw)


def f32(m, n, k):
    return call(m, n, k, dt=F32, bias=BIAS, out32=O32)


def nst(m, **kw):
    return call(m, 256, 256, bias=BIAS, **kw)


VTKW = dict(vt=VT, vt_T=4096, vt_Tpad=4096, vt_hd=64, vt_heads=4)
W4 = dict(direct=1)
TABLE = [
    # --- rounds of 256 x 256 tiles: 511 / 512 with one plane, 127 / 128 with two ----------------------------------------------------
    ("pp511_1plane", p16(BIG - 256, 256, 256), plan(DMA256x128, 1022)),
    ("pp512_1plane", p16(BIG, 256, 256), plan(T256W, 256, epi=1, **W4)),
    ("pp512_1plane_gelu", p16(BIG, 256, 256, act=L.ACT_GELU), plan(T256W, 256, epi=2, **W4)),
    ("pp512_1plane_bf16", p16(BIG, 256, 256, dt=BF16), plan(T256W, 256, epi=1, **W4)),                                  # HAND
    ("pp127_2plane", call(127 * 256, 256, 256, lda=128, bias=BIAS, out32=O32, a_kmod=128), plan(DMA128, 508)),
    ("pp128_2plane_k256", call(128 * 256, 256, 256, lda=128, bias=BIAS, out32=O32, a_kmod=128), plan(T256, 128, epi=0, planes=2)),
    ("pp128_2plane_k512", call(128 * 256, 256, 512, lda=256, bias=BIAS, out32=O32, a_kmod=256), plan(T256P, 128, epi=3, planes=2)),
    # --- rounds of 256 x 128 tiles below that: 510 / 512 at K <= 1536, and K = 1600 -------------------------------------------------
    ("t256x128_510_k128", p16(255 * 256, 256, 128), plan(DMA128, 1020)),
    ("t256x128_512_k128", p16(256 * 256, 256, 128), plan(DMA256x128, 512)),
    ("t256x128_512_k1536", p16(256 * 256, 256, 1536), plan(DMA256x128, 512)),
    ("t256x128_512_k1600", p16(256 * 256, 256, 1600), plan(DMA128, 1024)),
    # --- N % 256 != 0, K / 32 < 8: no persistent kernel ------------------------------------------------------------------------------
    ("n128_512tiles", p16(BIG, 128, 256), plan(T256, 512, epi=1)),
    ("n384_512tiles_gelu", p16(65536, 384, 256, act=L.ACT_GELU), plan(T256, 512, epi=2)),
    ("k64", p16(BIG, 256, 64), plan(T256, 512, epi=1)),
    ("k128", p16(BIG, 256, 128), plan(T256, 512, epi=1)),
    ("k192", p16(BIG, 256, 192), plan(T256, 512, epi=1)),
    ("k256", p16(BIG, 256, 256), plan(T256W, 256, epi=1, **W4)),
    ("k320_a_kmod_k", p16(BIG, 256, 320, a_kmod=320), plan(T256W, 256, epi=1, **W4)),                                   # HAND: a_kmod % 64 == 0
    # --- rows that are not 16 bytes, V^T columns off the 256 grid, operands the LDS-DMA cannot take ---------------------------------
    ("ld16_260", p16(BIG, 256, 256, ld16=260), plan(NT, 2048)),
    ("vt_col0_128", p16(BIG, 384, 256, vt_col0=128, **VTKW), plan(DMA256x128, 1536)),
    ("vt_col0_256_slab", p16(BIG, 512, 256, vt_col0=256, **VTKW), plan(T256W, 256, epi=1)),
    ("unaligned_a", p16(BIG, 256, 256, a=A + 8), plan(NT, 2048)),
    ("a_over_4gib", p16(4096, 256, 128, lda=1 << 19), plan(NT, 64)),
    ("w_over_4gib", p16(33, 4096, 128, ldw=1 << 19), plan(NT, 32)),                                                      # HAND
    # --- output row maps, ReLU, residual periods --------------------------------------------------------------------------------------
    ("scatter_slab", p16(BIG, 256, 256, map=L.MAP_WINDOW_PART, p=(16, 4, 4, 64, 64)), plan(T256W, 256, epi=1)),
    ("group_map", p16(BIG, 256, 256, map=L.MAP_GROUP, p=(4096, 4097, 1, 0, 0)), plan(T256, 512, epi=0)),
    ("relu_persistent_shape", p16(BIG, 256, 256, act=L.ACT_RELU), plan(T256, 512, epi=0)),
    ("resmod_whole_tiles", call(BIG, 256, 256, bias=BIAS, res=RES, res_mod=1024, out32=O32), plan(T256W, 256, epi=3, **W4)),
    ("resmod_ragged", call(BIG + 8, 256, 256, bias=BIAS, res=RES, res_mod=1024, out32=O32), plan(T256, 513, epi=0)),
    ("ragged_direct", p16(BIG + 8, 256, 256), plan(T256W, 256, epi=1, direct=1, ragged=1)),
    ("res_out32_out16", call(BIG, 256, 256, bias=BIAS, res=RES, out32=O32, out16=O16), plan(T256W, 256, epi=3, **W4)),
    ("lin1_group_m_8", p16(BIG, 3072, 768, act=L.ACT_GELU), plan(T256W, 256, epi=2, gm=8, **W4)),                       # HAND: N >= 2560
    # --- few rows --------------------------------------------------------------------------------------------------------------------
    ("m32", p16(32, 256, 256), plan(SKINNY, 16)),
    ("m33", p16(33, 256, 256), plan(DMA128, 2)),
    ("f32_128x256", f32(128, 256, 256), plan(SKINNY, 64)),
    ("f32_129x256", f32(129, 256, 256), plan(F32_SMALL, 12)),
    ("f32_512x256", f32(512, 256, 256), plan(F32_SMALL, 32)),
    ("f32_513x256", f32(513, 256, 256), plan(F32_N128, 10, epi=1)),
    ("f32_384x2688", f32(384, 2688, 256), plan(F32_SMALL, 252)),                                                         # 63 tiles of 128 x 128
    ("f32_512x2048", f32(512, 2048, 256), plan(F32_N128, 64, epi=1)),                                                    # 64
    ("f32_1024x32", f32(1024, 32, 256), plan(F32_N32, 8, epi=1)),
    ("f32_1024x40", f32(1024, 40, 256), plan(F32_N128, 8, epi=1)),
    ("f32_240x256x2048", f32(240, 256, 2048), plan(F32_SMALL, 64)),
    ("f32_20x256x2048", f32(20, 256, 2048), plan(SKINNY, 64)),
    ("f32_129_unaligned", call(129, 256, 256, dt=F32, a=A + 8, bias=BIAS, out32=O32), plan(SKINNY, 16 * 5)),             # HAND
    ("f32_1024x36_scalar_epilogue", f32(1024, 36, 256), plan(F32_N128, 8, epi=0)),                                       # HAND: N % 8 != 0
    # --- split-K: K = 46912 (733 k-tiles) on 9 output tiles -> 256 / 9 = 28 chunks wanted, 27 k-tiles each ----------------------------
    ("ksplit_46912", call(768, 768, 46912, out32=O32, ksplit=1), plan(T256Q, 252, epi=4, ksplit=28, kchunk=27 * 64)),
    # --- the fused epilogues of the four-wave kernel --------------------------------------------------------------------------------
    ("aux16_gelu", p16(BIG, 256, 256, aux16=AUX, act=L.ACT_GELU), plan(T256W, 256, epi=5, **W4)),
    ("aux16_gelu_bwd", call(BIG + 8, 256, 256, out16=O16, aux16=AUX, act=L.ACT_GELU_BWD), plan(T256W, 256, epi=6, direct=1, ragged=1)),
    ("nstat_in", nst(4096, out16=O16, nstat_in=NSI, ncol=NCOL), plan(T256W, 16, epi=8, **W4)),
    ("nstat_in_gelu_ragged", nst(4104, out16=O16, nstat_in=NSI, ncol=NCOL, act=L.ACT_GELU), plan(T256W, 17, epi=9, direct=1, ragged=1)),
    ("nstat_out_res_planes", nst(4096, out16=O16, aux16=AUX, res=RES, res_mod=1024, nstat_out=NSO), plan(T256W, 16, epi=7, **W4)),
    ("nstat_out_inplace", nst(4096, out16=O16, aux16=AUX, nstat_out=NSO), plan(T256W, 16, epi=11, **W4)),
    ("nstat_out_inplace_rvec256", nst(4096, out16=O16, aux16=AUX, nstat_out=NSO, rvec=RVEC, rvec_rpg=256), plan(T256W, 16, epi=11, **W4)),
    ("nstat_out_inplace_rvec192", nst(4096, out16=O16, aux16=AUX, nstat_out=NSO, rvec=RVEC, rvec_rpg=192), plan(T256W, 16, epi=12, **W4)),
    ("nstat_out_f32", nst(4096, out32=O32, out16=O16, res=RES, nstat_out=NSO), plan(T256W, 16, epi=7, **W4)),
    ("nstat_out_f32_rvec512", nst(4096, out32=O32, out16=O16, res=RES, nstat_out=NSO, rvec=RVEC, rvec_rpg=512), plan(T256W, 16, epi=7, **W4)),
    ("nstat_out_f32_rvec192", nst(4096, out32=O32, out16=O16, res=RES, nstat_out=NSO, rvec=RVEC, rvec_rpg=192), plan(T256W, 16, epi=10, **W4)),
    # --- la_gemm_variant on one persistent shape ------------------------------------------------------------------------------------
    ("variant1", p16(BIG, 256, 256, variant=1), plan(T256Q, 256, epi=1)),
    ("variant0", p16(BIG, 256, 256, variant=0), plan(T256P, 256, epi=1)),
    ("variant1_two_planes", call(128 * 256, 256, 512, lda=256, bias=BIAS, out32=O32, a_kmod=256, variant=1), plan(T256P, 128, epi=3, planes=2)),   # HAND
]

ERRORS = [
    ("null pointer", call(64, 64, 64, a=None, out32=O32)),
    ("bad shape M=0", call(0, 64, 64, out32=O32)),
    ("leading dimensions must be below 4194304", call(64, 64, 64, out32=O32, ld32=1 << 22)),
    ("multiples of 8", call(4, 4, 12, out32=O32)),
    ("multiples of 4", call(4, 4, 6, dt=F32, out32=O32)),
    ("no output", call(64, 64, 64)),
    ("a_kmod=72 must be a multiple of 64", call(64, 64, 144, out32=O32, a_kmod=72)),
    ("a_kmod=128 must be", call(32, 64, 256, out32=O32, a_kmod=128)),                      # M > 32
    ("bad dtype 3", call(64, 64, 64, dt=L.LA_F16X2, out32=O32)),
    ("amap must be", call(64, 64, 64, out32=O32, amap=L.MAP_WINDOW_PART, map=L.MAP_GROUP)),
    ("LA_ACT_GELU_BWD needs aux16", p16(BIG, 256, 256, act=L.ACT_GELU_BWD)),
    ("aux16 goes with LA_ACT_GELU", p16(BIG, 256, 256, aux16=AUX)),
    ("la_gemm_fused_act_ok", p16(BIG - 256, 128, 256, aux16=AUX, act=L.ACT_GELU)),
    ("la_gemm_fused_act_ok", p16(255 * 256, 256, 256, aux16=AUX, act=L.ACT_GELU)),        # 255 tiles on 256 CUs
    ("la_gemm_fused_act_ok", p16(BIG, 256, 256, aux16=AUX, act=L.ACT_GELU, variant=1)),
    ("aux16 forms write out16 only", p16(BIG, 256, 256, aux16=AUX, act=L.ACT_GELU, res=RES)),
    ("LA_ACT_GELU_BWD takes no bias", p16(BIG, 256, 256, aux16=AUX, act=L.ACT_GELU_BWD)),
    ("nstat_out / nstat_in need fp16 operands", nst(4096, dt=BF16, out16=O16, nstat_in=NSI, ncol=NCOL)),
    ("not both at once", nst(4096, out16=O16, nstat_in=NSI, ncol=NCOL, nstat_out=NSO)),
    ("nstat_in writes out16 only", nst(4096, out16=O16, nstat_in=NSI)),
    ("writes plane pairs only", nst(4096, out16=O16, aux16=AUX, res=RES, nstat_out=NSO, rvec=RVEC, rvec_rpg=256)),
    ("periodic residual needs res_mod", nst(4096 + 8, out16=O16, aux16=AUX, res=RES, res_mod=1024, nstat_out=NSO)),
    ("updates a plane-pair stream in place", nst(4096, out16=O16, nstat_out=NSO)),
    ("aux16 only with nstat_out", nst(4096, out16=O16, aux16=AUX, nstat_out=NSO, ldaux=260)),
    ("rvec needs a 16-byte aligned vector", nst(4096, out16=O16, aux16=AUX, nstat_out=NSO, rvec=RVEC, rvec_rpg=64)),
    ("nstat_out goes with out32 + out16", nst(4096, out32=O32, res=RES, nstat_out=NSO)),
    ("transposed-V epilogue is 16-bit only", call(1024, 256, 256, dt=F32, out16=O16, vt=VT, vt_T=1024, vt_Tpad=1024, vt_heads=4)),
    ("ksplit accumulates the bare product", call(768, 768, 1024, out32=O32, bias=BIAS, ksplit=1)),
    ("ksplit needs N % 256 == 0", call(768, 768, 64, out32=O32, ksplit=1)),
]


def ask(c):
    prev = L.gemm_variant(c["variant"])
    try:
        return L.gemm_plan(c["a"], c["lda"], W, c["ldw"], c["m"], c["n"], c["k"], c["dt"], NCU, **c["epi"])
    finally:
        L.gemm_variant(prev)


@pytest.mark.parametrize("name,c,want", TABLE, ids=[t[0] for t in TABLE])
def test_plan_is_the_launch_the_dispatcher_made(name, c, want):
    got = ask(c)
    if want["kchunk"] is None:
        want = dict(want, kchunk=c["k"])
    assert {f: getattr(got, f) for f in want} == want


@pytest.mark.parametrize("text,c", ERRORS, ids=[f"{i}-{e[0][:24]}" for i, e in enumerate(ERRORS)])
def test_plan_raises_la_gemms_errors(text, c):
    import re
    with pytest.raises(RuntimeError, match=re.escape(text)):
        ask(c)


def test_cu_count_is_an_argument():
    """Persistent grids and the one-round thresholds follow ncu: 304 CUs take 304 workgroups and refuse aux16 below 304 tiles."""
    c = p16(BIG, 256, 256)
    assert L.gemm_plan(A, 256, W, 256, BIG, 256, 256, F16, 304, **c["epi"]).grid == 304
    assert L.gemm_plan(A, 256, W, 256, 300 * 256, 256, 256, F16, 256, aux16=AUX, act=L.ACT_GELU, **c["epi"]).grid == 256
    with pytest.raises(RuntimeError, match="la_gemm_fused_act_ok"):
        L.gemm_plan(A, 256, W, 256, 300 * 256, 256, 256, F16, 304, aux16=AUX, act=L.ACT_GELU, **c["epi"])


def test_ping_pong_condition_implied_the_256x256_kernels():
    """Why gemm_pp_kernel could go: its condition - K > 1536, >= 512 tiles of 256 x 256, V^T columns on the 256 grid - sends every call
    that la_gemm lets through to the 256 x 256 kernels, which were tested first.  Swept over shapes, planes and epilogues."""
    n_checked = 0
    for m in (BIG - 256, BIG, BIG + 8, 4 * BIG):
        for n in (128, 256, 384, 1024, 3072):
            for k in (1664, 2048, 3072):
                for kw in (dict(out16=O16), dict(out16=O16, act=L.ACT_GELU), dict(out32=O32, res=RES), dict(out16=O16, act=L.ACT_RELU),
                           dict(out32=O32, a_kmod=k // 2), dict(out16=O16, vt_col0=n - 256, **VTKW), dict(out16=O16, vt_col0=n - 128, **VTKW),
                           dict(out16=O16, map=L.MAP_GROUP, p=(4096, 4097, 1, 0, 0)), dict(out32=O32, res=RES, res_mod=1024)):
                    if "vt" in kw and kw["vt_col0"] < 0:
                        continue
                    for dt in (F16, BF16):
                        p = L.gemm_plan(A, k, W, k, m, n, k, dt, NCU, bias=BIAS, **kw)
                        pp = k > 1536 and -(-m // 256) * -(-n // 256) >= 512 and ("vt" not in kw or kw["vt_col0"] % 256 == 0)
                        if pp:
                            n_checked += 1
                            assert p.kernel in (T256, T256P, T256Q, T256W), (m, n, k, kw, L.GEMM_KERNELS[p.kernel])
    assert n_checked > 500
