"""CPU: la_attn_fwd_plan / la_attn_bwd_plan against a literal table of what the attention entry points launched BEFORE the plan existed.

Every row is one call and the launch the commit before attn_plan.h made for it - kernel, MODE / BIAS, NH, VROW, grid, workgroup size,
dynamic LDS - read off that commit's launchers (launch_attn, launch_attn_nh, launch_window in attn_enc.hip; launch_attn_bwd_nh and
la_relpos_bwd in attn_bwd.hip); profiles/attn_plan.md holds the raw list with the arithmetic.  Nothing here is produced by the code under
test.  The last test ties the instantiations the launchers name to the cases tests/test_attention_conditioning_gpu.py runs on the GPU.
"""
import re

import pytest

from labelanything_amd import _lib as L
from tests import softmax_profiles as SP

P = {n: 0x7000_0000_0000 + i * 0x10_0000_0000 for i, n in enumerate(L._ATTN_CALL_PTRS)}       # "addresses": only tested for None
F16, BF16 = L.LA_F16, L.LA_BF16
PLAIN, RELPOS, WIN16 = L.ATTN_PLAIN, L.ATTN_RELPOS, L.ATTN_RELPOS_WIN16
FWD, WINDOW, DQ, DKV, RB_ROWS, RB = range(6)                                                   # LaAttnLaunch.kernel
NOBIAS, TERMS, TERMS_ROW64, TABLES_WIN, TABLES_ROW64, TABLES_WIN16 = range(6)                  # attn_fwd_kernel MODE
B_NOBIAS, B_TERMS, B_ROW64, B_WIN16 = range(4)                                                 # attn_bwd_dq_kernel BIAS
D_NOBIAS, D_TERMS, D_STAGED = range(3)                                                         # attn_bwd_dkv_kernel BIAS


def ptrs(*names):
    return {n: P[n] for n in names}


def call(entry, b, heads, t, tpad, g, hd, dt=F16, mode=PLAIN, **kw):
    """One entry-point call: LaAttnCall fields (E = heads * hd)."""
    return entry, dict(B=b, heads=heads, T=t, Tpad=tpad, G=g, E=heads * hd, dt=dt, mode=mode, **kw)


def fwd(b, heads, t, tpad, g, hd, dt=F16, mode=PLAIN, **kw):
    return call("attn_fwd", b, heads, t, tpad, g, hd, dt, mode, **{**ptrs("qkv", "vt", "out16"), **kw})


def rows(b, heads, t, tpad, g, hd, dt=F16, mode=PLAIN, **kw):
    return call("attn_fwd_rows", b, heads, t, tpad, g, hd, dt, mode, **{**ptrs("qkv", "out16"), **kw})


def lse(b, heads, t, tpad, hd, dt=F16, **kw):
    return call("attn_fwd_lse", b, heads, t, tpad, 0, hd, dt, PLAIN, **{**ptrs("qkv", "vt", "out16", "lse"), **kw})


def rlse(b, heads, g, tpad, hd, dt=F16, **kw):
    return call("attn_fwd_relpos_lse", b, heads, g * g, tpad, g, hd, dt, RELPOS, **{**ptrs("qkv", "vt", "out16", "relh", "relw", "lse"), **kw})


def bwd(b, heads, t, tpad, hd, dt=F16, **kw):
    return call("attn_bwd", b, heads, t, tpad, 0, hd, dt, **{**ptrs("qkv", "out16", "dout16", "lse", "dvec", "dqkv"), **kw})


def bwdr(b, heads, g, tpad, hd, dt=F16, **kw):
    return call("attn_bwd_relpos", b, heads, g * g, tpad, g, hd, dt,
                **{**ptrs("qkv", "out16", "dout16", "lse", "dvec", "dqkv", "relh", "relw", "drelh", "drelw"), **kw})


def rbwd(b, heads, g, hd, dt=F16, **kw):
    return call("relpos_bwd", b, heads, 0, 0, g, hd, dt, **{**ptrs("qkv", "dqkv", "drelh", "drelw", "tabh", "tabw", "dtabh", "dtabw"), **kw})


TABS, TERMS_IN = ptrs("tabh", "tabw"), ptrs("relh", "relw")


def k(kernel, mode, nh, vrow, grid, lds):
    return dict(kernel=kernel, mode=mode, nh=nh, vrow=vrow, grid=grid, block=256, lds_bytes=lds)


# dynamic LDS of the parent's launchers.  Forward: two stages of (K tile + V tile) = 2 x 16384 per 64-wide half, then the bias tables
S1, S2 = 2 * 16384, 2 * 2 * 16384
TAB4 = 4 * 32 * 33 * 4                    # 16896: MODE 4 / MODE 5, one 32 x 33 fp32 table per wave
TAB8 = 4 * 2 * 32 * 33 * 4                # 33792: MODE 3 / attn_window_kernel, two per wave (+ Tpad ints)
ROW65 = 4 * 32 * 65 * 4                   # 33280: MODE 2

FORWARD = [
    # --- plain: T = 200 -> two query blocks x 2 x 2 image-heads ------------------------------------------------------------------------
    ("plain_64_f16", fwd(2, 2, 200, 256, 0, 64), [k(FWD, NOBIAS, 1, 0, 8, S1)]),
    ("plain_128_bf16", fwd(2, 2, 200, 256, 0, 128, BF16), [k(FWD, NOBIAS, 2, 0, 8, S2)]),
    ("plain_64_bh8", fwd(4, 2, 200, 256, 0, 64), [k(FWD, NOBIAS, 1, 0, 16, S1)]),                  # BH % 8 == 0: same grid, the kernel reorders
    ("plain_rows_64_bf16", rows(2, 2, 200, 256, 0, 64, BF16), [k(FWD, NOBIAS, 1, 1, 8, S1)]),
    ("plain_rows_128_f16", rows(2, 2, 200, 256, 0, 128), [k(FWD, NOBIAS, 2, 1, 8, S2)]),
    ("plain_lse_64_f16", lse(2, 2, 200, 256, 64), [k(FWD, NOBIAS, 1, 0, 8, S1)]),
    ("plain_lse_128_bf16", lse(2, 2, 200, 256, 128, BF16), [k(FWD, NOBIAS, 2, 0, 8, S2)]),
    ("plain_cs_64", fwd(2, 2, 200, 256, 0, 64, cspart=P["cspart"]), [k(FWD, NOBIAS, 1, 0, 8, S1)]),
    # --- WIN16: G = 14 (T = 196, Tpad = 256) and G = 16, slot order (V^T) and rows form, image order ---------------------------------
    ("win16_g14_slots", fwd(2, 2, 196, 256, 14, 64, mode=WIN16, **TABS), [k(FWD, TABLES_WIN16, 1, 0, 8, S1 + TAB4)]),
    ("win16_g14_rows", rows(2, 2, 196, 256, 14, 64, mode=WIN16, **TABS), [k(FWD, TABLES_WIN16, 1, 1, 8, 49664)]),                # anchor
    ("win16_g14_rows_128", rows(2, 2, 196, 256, 14, 128, mode=WIN16, **TABS), [k(FWD, TABLES_WIN16, 2, 1, 8, 82432)]),           # anchor
    ("win16_g16_slots_bf16", fwd(2, 2, 256, 256, 16, 64, BF16, WIN16, **TABS), [k(FWD, TABLES_WIN16, 1, 0, 8, S1 + TAB4)]),
    ("win16_g16_rows", rows(2, 2, 256, 256, 16, 64, mode=WIN16, **TABS), [k(FWD, TABLES_WIN16, 1, 1, 8, S1 + TAB4)]),
    ("win16_g14_image_order", rows(25, 2, 196, 256, 14, 64, mode=WIN16, imgH=64, imgW=64, padrow=P["padrow"], **TABS),
     [k(FWD, TABLES_WIN16, 1, 1, 100, S1 + TAB4)]),
    ("win16_g14_cs_image_grid", fwd(25, 2, 196, 256, 14, 64, mode=WIN16, cspart=P["cspart"], csH=64, csW=64, **TABS),
     [k(FWD, TABLES_WIN16, 1, 0, 100, S1 + TAB4)]),
    # --- RELPOS with the tables, G <= 16: the window kernel at 64 wide, the LDS-staged MODE 3 at 128 ----------------------------------
    ("tables_g8_64", fwd(1, 2, 64, 64, 8, 64, mode=RELPOS, **TABS), [k(WINDOW, TABLES_WIN, 1, 0, 1, 34048)]),                    # anchor
    ("tables_g8_128", fwd(1, 2, 64, 64, 8, 128, mode=RELPOS, **TABS), [k(FWD, TABLES_WIN, 2, 0, 2, S2 + TAB8 + 64 * 4)]),
    ("tables_g14_64_bf16", fwd(2, 2, 196, 256, 14, 64, BF16, RELPOS, **TABS), [k(WINDOW, TABLES_WIN, 1, 0, 7, 256 * 4 + TAB8)]),   # 28 waves
    ("tables_g14_64_terms_too", fwd(2, 2, 196, 256, 14, 64, mode=RELPOS, **TABS, **TERMS_IN), [k(WINDOW, TABLES_WIN, 1, 0, 7, 256 * 4 + TAB8)]),
    # --- RELPOS at G = 64: tables (MODE 4) before terms (MODE 2); V^T and rows forms ---------------------------------------------------
    ("g64_tables", fwd(1, 2, 4096, 4096, 64, 64, mode=RELPOS, **TABS), [k(FWD, TABLES_ROW64, 1, 0, 64, S1 + TAB4)]),
    ("g64_tables_and_terms", fwd(1, 2, 4096, 4096, 64, 64, mode=RELPOS, **TABS, **TERMS_IN), [k(FWD, TABLES_ROW64, 1, 0, 64, S1 + TAB4)]),
    ("g64_terms", fwd(1, 2, 4096, 4096, 64, 64, mode=RELPOS, **TERMS_IN), [k(FWD, TERMS_ROW64, 1, 0, 64, S1 + ROW65)]),
    ("g64_terms_128_bf16", fwd(1, 2, 4096, 4096, 64, 128, BF16, RELPOS, **TERMS_IN), [k(FWD, TERMS_ROW64, 2, 0, 64, S2 + ROW65)]),
    ("g64_tables_128", fwd(1, 2, 4096, 4096, 64, 128, mode=RELPOS, **TABS), [k(FWD, TABLES_ROW64, 2, 0, 64, S2 + TAB4)]),
    ("g64_rows", rows(1, 2, 4096, 4096, 64, 64, mode=RELPOS, **TABS), [k(FWD, TABLES_ROW64, 1, 1, 64, S1 + TAB4)]),
    ("g64_rows_128_bf16", rows(1, 2, 4096, 4096, 64, 128, BF16, RELPOS, **TABS), [k(FWD, TABLES_ROW64, 2, 1, 64, S2 + TAB4)]),
    # --- RELPOS with terms on other grids (MODE 1): 4 waves x 2 tables x 32 x (G + 1) fp32 + Tpad ints --------------------------------
    ("terms_g32", fwd(1, 2, 1024, 1024, 32, 64, mode=RELPOS, **TERMS_IN), [k(FWD, TERMS, 1, 0, 16, S1 + 1024 * 33 + 4096)]),
    ("terms_g14", fwd(2, 2, 196, 256, 14, 64, mode=RELPOS, **TERMS_IN), [k(FWD, TERMS, 1, 0, 8, S1 + 1024 * 15 + 1024)]),
    ("terms_g20_tables_unused", fwd(2, 2, 400, 448, 20, 128, mode=RELPOS, **TABS, **TERMS_IN), [k(FWD, TERMS, 2, 0, 16, S2 + 1024 * 21 + 1792)]),
    ("relpos_lse_g14", rlse(2, 2, 14, 256, 64), [k(FWD, TERMS, 1, 0, 8, S1 + 1024 * 15 + 1024)]),
    ("relpos_lse_g64_bf16", rlse(1, 2, 64, 4096, 64, BF16), [k(FWD, TERMS_ROW64, 1, 0, 64, S1 + ROW65)]),
]

# backward: dq = two stages of K | V tiles (2 x 2 x NH x 8192) + bias; dk / dv = 2 x (2 x NH x 8192 + 512 [+ 16384 + 1024 staged terms])
Q1, Q2 = 32768, 65536
KV1, KV2, KV1S, KV2S = 2 * (16384 + 512), 2 * (32768 + 512), 2 * (16384 + 512 + 17408), 2 * (32768 + 512 + 17408)
E_T = 32 * (256 * 2 + 16) + 256 * 4       # BIAS 3 at Tpad = 256: E^T [32][Tpad] 16 bit, rows + 16 bytes, + Tpad ints
G64 = (2 * 64 * 65 + 127 * 64) * 4 + 64 * 64 * 2        # relpos_bwd_kernel at G = 64: 73984
BACKWARD = [
    ("plain_64", bwd(2, 2, 200, 256, 64), [k(DQ, B_NOBIAS, 1, 0, 8, Q1), k(DKV, D_NOBIAS, 1, 0, 8, KV1)]),
    ("plain_128_bf16", bwd(2, 2, 200, 256, 128, BF16), [k(DQ, B_NOBIAS, 2, 0, 8, Q2), k(DKV, D_NOBIAS, 2, 0, 8, KV2)]),
    ("g14_64", bwdr(2, 2, 14, 256, 64), [k(DQ, B_WIN16, 1, 0, 8, Q1 + E_T), k(DKV, D_STAGED, 1, 0, 8, KV1S)]),
    ("g14_128", bwdr(2, 2, 14, 256, 128), [k(DQ, B_WIN16, 2, 0, 8, Q2 + E_T), k(DKV, D_STAGED, 2, 0, 8, KV2S)]),
    ("g15_64_odd", bwdr(2, 2, 15, 256, 64), [k(DQ, B_WIN16, 1, 0, 8, Q1 + E_T), k(DKV, D_TERMS, 1, 0, 8, KV1)]),
    ("g15_128_odd_bf16", bwdr(2, 2, 15, 256, 128, BF16), [k(DQ, B_WIN16, 2, 0, 8, Q2 + E_T), k(DKV, D_TERMS, 2, 0, 8, KV2)]),
    ("g20_64", bwdr(2, 2, 20, 448, 64), [k(DQ, B_TERMS, 1, 0, 16, Q1 + 2048 * 21 + 1792), k(DKV, D_STAGED, 1, 0, 16, KV1S)]),
    ("g32_64", bwdr(1, 2, 32, 1024, 64), [k(DQ, B_TERMS, 1, 0, 16, Q1 + 2048 * 33 + 4096), k(DKV, D_STAGED, 1, 0, 16, KV1S)]),
    ("g32_128", bwdr(1, 2, 32, 1024, 128), [k(DQ, B_TERMS, 2, 0, 16, Q2 + 2048 * 33 + 4096), k(DKV, D_STAGED, 2, 0, 16, KV2S)]),
    ("g64_64", bwdr(1, 2, 64, 4096, 64), [k(DQ, B_ROW64, 1, 0, 64, Q1), k(DKV, D_STAGED, 1, 0, 64, KV1S)]),
    ("g64_128", bwdr(1, 2, 64, 4096, 128), [k(DQ, B_ROW64, 2, 0, 64, Q2), k(DKV, D_STAGED, 2, 0, 64, KV2S)]),
]
# la_relpos_bwd: (launch, repeat, ry).  Rows path: 64 x 64 fp32 + 4 waves x (2 x 32 x G fp32 + 32 x 64 16 bit); a wave per 32 queries
RELPOS_BWD = [
    ("rows_g14", rbwd(2, 2, 14, 64), k(RB_ROWS, 0, 1, 0, 7, 16384 + 4 * (2 * 32 * 14 * 4 + 4096)), 1, 1),                        # 28 units
    ("rows_g14_512_cap", rbwd(100, 12, 14, 64, BF16), k(RB_ROWS, 0, 1, 0, 512, 47104), 1, 1),                                    # 8400 units
    ("rows_g14_128_two_launches", rbwd(2, 2, 14, 128), k(RB_ROWS, 0, 1, 0, 7, 47104), 2, 1),
    ("rows_g16", rbwd(2, 2, 16, 64), k(RB_ROWS, 0, 1, 0, 8, 16384 + 4 * (4096 + 4096)), 1, 1),
    ("generic_g20", rbwd(2, 2, 20, 64), k(RB, 0, 1, 0, 80, (2 * 20 * 21 + 39 * 64) * 4 + 20 * 128), 1, 1),
    ("g64_ry1", rbwd(1, 2, 64, 64), k(RB, 0, 1, 0, 128, G64), 1, 1),                                # 2 x 32 row pairs < 768
    ("g64_ry1_below", rbwd(1, 23, 64, 64), k(RB, 0, 1, 0, 23 * 64, G64), 1, 1),                     # 23 x 32 = 736 < 768
    ("g64_ry2", rbwd(2, 12, 64, 64, BF16), k(RB, 0, 1, 0, 24 * 32, G64), 1, 2),                     # 24 x 32 = 768 -> 2; 24 x 16 < 768
    ("g64_ry4", rbwd(4, 12, 64, 64), k(RB, 0, 1, 0, 48 * 16, G64), 1, 4),                           # 48 x 16 = 768 -> 4; 48 x 8 < 768
    ("g64_128_two_launches", rbwd(1, 2, 64, 128), k(RB, 0, 1, 0, 128, G64), 2, 1),
]


def ask(c):
    entry, kw = c
    return (L.attn_fwd_plan if entry.startswith("attn_fwd") else L.attn_bwd_plan)(entry, **kw)


def launches(plan):
    return [{f: getattr(plan.launch[i], f) for f, _ in L.LaAttnLaunch._fields_} for i in range(plan.n)]


@pytest.mark.parametrize("name,c,want", FORWARD + BACKWARD, ids=[t[0] for t in FORWARD] + ["bwd_" + t[0] for t in BACKWARD])
def test_plan_is_the_launch_the_entry_point_made(name, c, want):
    got = ask(c)
    assert launches(got) == want and got.repeat == 1


@pytest.mark.parametrize("name,c,want,repeat,ry", RELPOS_BWD, ids=[t[0] for t in RELPOS_BWD])
def test_relpos_bwd_plan_is_the_launch_loop_the_entry_point_ran(name, c, want, repeat, ry):
    got = ask(c)
    assert launches(got) == [want] and (got.repeat, got.ry) == (repeat, ry)


BAD_DT = L.LA_F32
ERRORS = [
    # la_attn_fwd / la_attn_fwd_cs
    ("la_attn_fwd: null pointer", fwd(2, 2, 200, 256, 0, 64, vt=None)),
    ("la_attn_fwd: needs head_dim 64 or 128 - pad other widths with zero columns (E=160 heads=2)", fwd(2, 2, 200, 256, 0, 80)),
    ("la_attn_fwd: Tpad=192 must be a multiple of 64 covering T=200", fwd(2, 2, 200, 192, 0, 64)),
    ("la_attn_fwd: bad dtype 2", fwd(2, 2, 200, 256, 0, 64, BAD_DT)),
    ("la_attn_fwd: WIN16 needs the tables, T == G*G, G <= 16 and Tpad >= 16*G (T=169 G=13 Tpad=192)", fwd(2, 2, 169, 192, 13, 64, mode=WIN16, **TABS)),
    ("la_attn_fwd: rel-pos needs T == G*G, G <= 64 (T=200 G=14)", fwd(2, 2, 200, 256, 14, 64, mode=RELPOS, **TERMS_IN)),
    ("la_attn_fwd: rel-pos terms missing (run la_relpos_terms", fwd(2, 2, 400, 448, 20, 64, mode=RELPOS, **TABS)),
    ("la_attn_fwd: bad mode 7", fwd(2, 2, 200, 256, 0, 64, mode=7)),
    # la_attn_fwd_rows
    ("la_attn_fwd_rows: null pointer", rows(2, 2, 200, 256, 0, 64, out16=None)),
    ("la_attn_fwd_rows: needs head_dim 64 or 128 - pad other widths with zero columns (E=64 heads=2)", rows(2, 2, 200, 256, 0, 32)),
    ("la_attn_fwd_rows: Tpad=200 must be a multiple of 64 covering T=200", rows(2, 2, 200, 200, 0, 64)),
    ("la_attn_fwd_rows: bad dtype 3", rows(2, 2, 200, 256, 0, 64, L.LA_F16X2)),
    ("la_attn_fwd_rows: WIN16 needs the tables, T == G*G, G <= 16 and Tpad >= 16*G (T=196 G=14 Tpad=256)", rows(2, 2, 196, 256, 14, 64, mode=WIN16)),
    ("la_attn_fwd_rows: image-order windows need imgW, padrow and B = images * 25 windows",
     rows(24, 2, 196, 256, 14, 64, mode=WIN16, imgH=64, imgW=64, padrow=P["padrow"], **TABS)),
    ("la_attn_fwd_rows: rel-pos form needs the tables and the 64 x 64 grid (G=32 T=1024)", rows(1, 2, 1024, 1024, 32, 64, mode=RELPOS, **TABS)),
    ("la_attn_fwd_rows: bad mode 3", rows(2, 2, 200, 256, 0, 64, mode=3)),
    # la_attn_fwd_lse
    ("la_attn_fwd_lse: null pointer", lse(2, 2, 200, 256, 64, lse=None)),
    ("la_attn_fwd_lse: needs head_dim 64 or 128 - other widths zero-padded (E=160 heads=2)", lse(2, 2, 200, 256, 80)),
    ("la_attn_fwd_lse: Tpad=128 must be a multiple of 64 covering T=200", lse(2, 2, 200, 128, 64)),
    ("la_attn_fwd_lse: bad dtype 2", lse(2, 2, 200, 256, 64, BAD_DT)),
    # la_attn_fwd_relpos_lse
    ("la_attn_fwd_relpos_lse: null pointer", rlse(2, 2, 14, 256, 64, relw=None)),
    ("la_attn_fwd_relpos_lse: needs head_dim 64 or 128 - other widths zero-padded (E=0 heads=2)", rlse(2, 2, 14, 256, 0)),
    ("la_attn_fwd_relpos_lse: Tpad=250 must be a multiple of 64 covering T=196", rlse(2, 2, 14, 250, 64)),
    ("la_attn_fwd_relpos_lse: rel-pos needs T == G*G, G <= 64 (T=4225 G=65)", rlse(1, 2, 65, 4288, 64, dt=BAD_DT)),       # (before the dtype)
    ("la_attn_fwd_relpos_lse: bad dtype 2", rlse(2, 2, 14, 256, 64, BAD_DT)),
    # la_attn_bwd
    ("la_attn_bwd: null pointer", bwd(2, 2, 200, 256, 64, dvec=None)),
    ("la_attn_bwd: needs head_dim 64 or 128 - other widths zero-padded (E=192 heads=2)", bwd(2, 2, 200, 256, 96)),
    ("la_attn_bwd: Tpad=192 must be a multiple of 64 covering T=200", bwd(2, 2, 200, 192, 64)),
    ("la_attn_bwd: bad dtype 2", bwd(2, 2, 200, 256, 64, BAD_DT)),
    # la_attn_bwd_relpos
    ("la_attn_bwd_relpos: null pointer", bwdr(2, 2, 14, 256, 64, drelh=None)),
    ("la_attn_bwd_relpos: needs head_dim 64 or 128 - other widths zero-padded (E=192 heads=2)", bwdr(2, 2, 14, 256, 96)),
    ("la_attn_bwd_relpos: Tpad=196 must be a multiple of 64 covering T=196", bwdr(2, 2, 14, 196, 64)),
    ("la_attn_bwd_relpos: T == G*G with G <= 32 or G == 64 (T=1600 G=40)", bwdr(1, 2, 40, 1600, 64, dt=BAD_DT)),          # (before the dtype)
    ("la_attn_bwd_relpos: bad dtype 2", bwdr(2, 2, 14, 256, 64, BAD_DT)),
    # la_relpos_bwd
    ("la_relpos_bwd: null pointer", rbwd(2, 2, 14, 64, dtabw=None)),
    ("la_relpos_bwd: needs head_dim 64 or 128 (tables [(2 G - 1), head_dim] fp32), G <= 64 (E=128 heads=2 G=65)", rbwd(2, 2, 65, 64)),
    ("la_relpos_bwd: bad dtype 2", rbwd(2, 2, 14, 64, BAD_DT)),
]


@pytest.mark.parametrize("text,c", ERRORS, ids=[f"{i}-{e[0][:40]}" for i, e in enumerate(ERRORS)])
def test_plan_raises_the_entry_points_errors(text, c):
    with pytest.raises(RuntimeError, match=re.escape(text)):
        ask(c)


# ---- the instantiations the launchers name, and the ones the GPU suite runs -----------------------------------------------------------
DTS = (F16, BF16)
NAMED = ({(FWD, m, nh, 0, dt) for m in range(6) for nh in (1, 2) for dt in DTS}                              # launch_attn_fwd, V^T form
         | {(FWD, m, nh, 1, dt) for m in (NOBIAS, TABLES_ROW64, TABLES_WIN16) for nh in (1, 2) for dt in DTS}      # ... V-row form
         | {(WINDOW, TABLES_WIN, 1, 0, dt) for dt in DTS}
         | {(DQ, b, nh, 0, dt) for b in range(4) for nh in (1, 2) for dt in DTS}                                # launch_attn_bwd
         | {(DKV, b, nh, 0, dt) for b in range(3) for nh in (1, 2) for dt in DTS}
         | {(kern, 0, 1, 0, dt) for kern in (RB_ROWS, RB) for dt in DTS})                                       # launch_relpos_bwd
# named, but run by no case of tests/test_attention_conditioning_gpu.py (profiles/attn_plan.md says what each is)
NOT_IN_THE_CONDITIONING_SUITE = (
    {(FWD, TERMS, 2, 0, dt) for dt in DTS}                                      # terms on a window grid, 128-wide heads
    | {(FWD, TABLES_WIN, 1, 0, dt) for dt in DTS}                               # 64-wide heads take attn_window_kernel (measurement library: LA_WINDOW_PATH)
    | {(FWD, m, 2, v, BF16) for m, v in ((TERMS_ROW64, 0), (TABLES_ROW64, 0), (TABLES_ROW64, 1))}     # G = 64, 128-wide heads, bf16
    | {(FWD, TABLES_WIN16, 2, v, dt) for v in (0, 1) for dt in DTS}             # slot-order windows, 128-wide heads
    | {(DQ, B_NOBIAS, 2, 0, BF16), (DKV, D_NOBIAS, 2, 0, BF16)}                 # plain backward, 128-wide heads, bf16
    | {(DQ, B_TERMS, 1, 0, BF16), (DQ, B_ROW64, 1, 0, BF16)}                    # rel-pos backward in bf16 beyond the 14 x 14 windows
    | {(DQ, b, 2, 0, dt) for b in (B_TERMS, B_ROW64, B_WIN16) for dt in DTS}    # rel-pos backward, 128-wide heads
    | {(DKV, D_TERMS, nh, 0, dt) for nh in (1, 2) for dt in DTS}                # odd G
    | {(DKV, D_STAGED, 2, 0, dt) for dt in DTS}
    | {(RB, 0, 1, 0, BF16)})


def conditioning_suite_calls():
    """The library calls of tests/test_attention_conditioning_gpu.py that reach an attention plan, case by case."""
    calls = []
    for fam, kind, t, g, hd, dt, order, b, heads in SP.forward_cases():
        d, tpad = {"f16": F16, "bf16": BF16}.get(dt), (t + 63) // 64 * 64
        if fam == "plain":
            calls += [fwd(b, heads, t, tpad, 0, hd, d), rows(b, heads, t, tpad, 0, hd, d), fwd(b, heads, t, tpad, 0, hd, d, cspart=P["cspart"]),
                      lse(b, heads, t, tpad, hd, d)]
        elif fam == "terms":
            calls += [fwd(b, heads, t, tpad, g, hd, d, RELPOS, **TERMS_IN), rlse(b, heads, g, tpad, hd, d)]
        elif fam == "tables":
            calls += [fwd(b, heads, t, tpad, g, hd, d, RELPOS, **TABS)]
        elif fam == "global":
            calls += [fwd(b, heads, t, t, g, hd, d, RELPOS, **TERMS_IN), fwd(b, heads, t, t, g, hd, d, RELPOS, **TABS),
                      rows(b, heads, t, t, g, hd, d, RELPOS, **TABS)]
        elif fam == "win16":
            tp = (16 * g + 63) // 64 * 64
            calls += [fwd(b, heads, t, tp, g, hd, d, WIN16, **TABS), rows(b, heads, t, tp, g, hd, d, WIN16, **TABS)]
        else:
            assert fam == "fp8"               # la_attn_fwd_fp8: one kernel, no plan
    for d in DTS:                             # test_windows_in_image_order_with_a_spike_on_the_pad_row: a 20 x 27 image in 14 x 14 windows
        calls.append(rows(4, 2, 196, 256, 14, 64, d, WIN16, imgH=20, imgW=27, padrow=P["padrow"], **TABS))
    for fam, kind, t, g, hd, dt, b, heads in SP.backward_cases():
        d, tpad = {"f16": F16, "bf16": BF16}[dt], (t + 63) // 64 * 64
        if fam == "plain":
            calls += [lse(b, heads, t, tpad, hd, d), bwd(b, heads, t, tpad, hd, d)]
        else:
            calls += [rlse(b, heads, g, tpad, hd, d), bwdr(b, heads, g, tpad, hd, d), rbwd(b, heads, g, hd, d)]
    return calls


def test_launchers_name_what_the_conditioning_suite_runs_plus_a_stated_list():
    reached = set()
    for c in conditioning_suite_calls():
        plan = ask(c)
        for l in launches(plan):
            reached.add((l["kernel"], l["mode"], l["nh"], l["vrow"], c[1]["dt"]))
    assert reached <= NAMED, sorted(reached - NAMED)
    assert not (reached & NOT_IN_THE_CONDITIONING_SUITE), sorted(reached & NOT_IN_THE_CONDITIONING_SUITE)
    assert reached | NOT_IN_THE_CONDITIONING_SUITE == NAMED, sorted(NAMED - reached - NOT_IN_THE_CONDITIONING_SUITE)
