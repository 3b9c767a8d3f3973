// What an encoder-attention call launches, as one pure function of its arguments: argument checks, kernel family, template arguments,
// grid, workgroup size, dynamic LDS - forward (attn_enc.hip) and backward (attn_bwd.hip).  Host only: no environment, no statics, no device
// queries, pointers are only tested for null - the same plan comes out on a machine without a GPU (la_attn_fwd_plan / la_attn_bwd_plan,
// tests/test_attn_plan_cpu.py).  The entry points launch what the plan says.
#pragma once
#include <cstddef>
#include <cstdio>
#include "../../include/la_hip.h"

namespace la {

// ---- attn_fwd_kernel<T, MODE, NH, VROW>: where the rel-pos bias of a score comes from (LaAttnLaunch.mode of LA_ATTN_K_FWD) --------------
constexpr int ATTN_NOBIAS = 0;          // plain softmax(q k^T scale) v
constexpr int ATTN_TERMS = 1;           // terms from la_relpos_terms, any G <= 64: per-wave LDS tables indexed by (key / G, key % G)
constexpr int ATTN_TERMS_ROW64 = 2;     // terms from la_relpos_terms, G == 64: a 64-key tile is one key row - relw in registers, relh[q][tile] one LDS read
constexpr int ATTN_TABLES_WIN = 3;      // 16-bit tables, G <= 16 (SAM windows, token order): U[r][q] = R[r] . q on MFMA in the prologue, no la_relpos_terms pass
constexpr int ATTN_TABLES_ROW64 = 4;    // 16-bit tables, G == 64: ATTN_TERMS_ROW64 with the terms computed in the prologue of each query tile
constexpr int ATTN_TABLES_WIN16 = 5;    // 16-bit tables, G <= 16, keys in 16-wide slot order (LA_ATTN_RELPOS_WIN16): padding carries NEG_BIG, no masking pass

// ---- attn_bwd_dq_kernel<T, BIAS, NH> (LaAttnLaunch.mode of LA_ATTN_K_BWD_DQ) --------------------------------------------------------------
constexpr int ATTN_BWD_NOBIAS = 0;
constexpr int ATTN_BWD_TERMS = 1;       // 16 < G <= 32: per-wave LDS tables as ATTN_TERMS, gradients scatter-added into a second pair (ds_add_f32)
constexpr int ATTN_BWD_ROW64 = 2;       // G == 64: relh[q][tile] one scalar per tile, relw / d relw in registers
constexpr int ATTN_BWD_WIN16 = 3;       // G <= 16: bias and its gradient as products with a 0 / 1 matrix on the matrix pipe
// ---- attn_bwd_dkv_kernel<T, BIAS, NH> (LaAttnLaunch.mode of LA_ATTN_K_BWD_DKV) ------------------------------------------------------------
constexpr int ATTN_DKV_NOBIAS = 0;
constexpr int ATTN_DKV_TERMS = 1;       // the two terms of a score read from global memory (odd G: rows of 64 queries are not 16-byte aligned)
constexpr int ATTN_DKV_STAGED = 2;      // the terms of a tile's 64 queries staged in LDS beside the tile (even G)

constexpr int ATTN_BLOCK = 256;                   // every attention kernel: four waves
constexpr int TILE_B = 64 * 64 * 2;               // one 64 x 64 16-bit tile: 8 KiB, 128-byte rows, XOR swizzled
constexpr int KV_STAGE = 2 * TILE_B;              // forward: K tile + V tile of one 64-wide half, 16 KiB

#define LA_PLAN_CHECK(cond, ...) \
  do { if (!(cond)) { snprintf(err, errsz, __VA_ARGS__); return -1; } } while (0)

static inline const char* attn_entry_name(int entry) {
  static const char* const names[] = {"la_attn_fwd", "la_attn_fwd_rows", "la_attn_fwd_lse", "la_attn_fwd_relpos_lse",
                                      "la_attn_bwd", "la_attn_bwd_relpos", "la_relpos_bwd"};
  return entry >= 0 && entry <= LA_ATTN_EP_RELPOS_BWD ? names[entry] : "la_attn";
}
static inline int attn_nh(const LaAttnCall& c) { return c.E == c.heads * 128 ? 2 : 1; }       // head width / 64
static inline int attn_blocks128(const LaAttnCall& c) { return (c.T + 127) / 128 * c.B * c.heads; }      // one workgroup per 128 rows of an image-head

// the checks every forward and attention-backward entry point shares (la_relpos_bwd has its own)
static inline int attn_check_shape(const char* who, bool fwd_api, const LaAttnCall& c, char* err, size_t errsz) {
  LA_PLAN_CHECK(c.B > 0 && c.heads > 0 && c.T > 0 && (c.E == c.heads * 64 || c.E == c.heads * 128), "%s: needs head_dim 64 or 128 - %s (E=%d heads=%d)",
                who, fwd_api ? "pad other widths with zero columns" : "other widths zero-padded", c.E, c.heads);
  LA_PLAN_CHECK(c.Tpad >= c.T && (c.Tpad % 64) == 0, "%s: Tpad=%d must be a multiple of 64 covering T=%d", who, c.Tpad, c.T);
  return 0;
}

// dynamic LDS of attn_fwd_kernel behind its K / V stages: the bias tables of the four waves
static inline int attn_fwd_bias_lds(int mode, int G, int Tpad) {
  const int tab = 32 * 33 * (int)sizeof(float);       // one table of a wave's 32 queries: 32 rows padded to 33 fp32
  const int keyinfo = Tpad * (int)sizeof(int);        // key -> (key row, key column) lookup, shared by the waves
  switch (mode) {
    case ATTN_TERMS: return 4 * 2 * 32 * (G + 1) * (int)sizeof(float) + keyinfo;      // relh | relw rows of the wave's queries, [32][G + 1] each
    case ATTN_TERMS_ROW64: return 4 * 32 * 65 * (int)sizeof(float);                   // relh rows of the wave's queries, 32 x 65
    case ATTN_TABLES_WIN: return 4 * 2 * tab + keyinfo;                               // U_h | U_w per wave
    case ATTN_TABLES_ROW64: return 4 * tab;                                           // relh half-row table per wave (also the U_w bounce)
    case ATTN_TABLES_WIN16: return 4 * tab;                                           // one table per wave, used for U_w then U_h
    default: return 0;
  }
}
// attn_fwd_kernel<T, mode, nh, vrow>: one workgroup per 128 query rows of an image-head; two K / V stages per 64-wide half + the bias tables
static inline LaAttnLaunch attn_fwd_tile_launch(int mode, bool vrow, const LaAttnCall& c) {
  const int nh = attn_nh(c);
  return LaAttnLaunch{LA_ATTN_K_FWD, mode, nh, vrow ? 1 : 0, attn_blocks128(c), ATTN_BLOCK, 2 * KV_STAGE * nh + attn_fwd_bias_lds(mode, c.G, c.Tpad)};
}
// attn_window_kernel<T> (64-wide heads only): one WAVE per (window, head, 32-query tile), no K / V staging - the key lookup + U_h | U_w per wave
static inline LaAttnLaunch attn_window_launch(const LaAttnCall& c) {
  const int njobs = c.B * c.heads * ((c.T + 31) / 32);
  return LaAttnLaunch{LA_ATTN_K_WINDOW, ATTN_TABLES_WIN, 1, 0, (njobs + 3) / 4, ATTN_BLOCK, attn_fwd_bias_lds(ATTN_TABLES_WIN, c.G, c.Tpad)};
}

// la_attn_fwd / la_attn_fwd_cs (entry LA_ATTN_EP_FWD), la_attn_fwd_rows, la_attn_fwd_lse (c.mode = LA_ATTN_PLAIN), la_attn_fwd_relpos_lse
// (c.mode = LA_ATTN_RELPOS, no tables)
static inline int attn_fwd_plan(int entry, const LaAttnCall& c, LaAttnPlan* p, char* err, size_t errsz) {
  *p = LaAttnPlan{};
  const char* who = attn_entry_name(entry);
  const bool rows = entry == LA_ATTN_EP_FWD_ROWS;
  LA_PLAN_CHECK(entry >= LA_ATTN_EP_FWD && entry <= LA_ATTN_EP_FWD_RELPOS_LSE, "la_attn_fwd_plan: bad entry point %d", entry);
  LA_PLAN_CHECK(c.qkv && c.out16 && (rows || c.vt) && ((entry != LA_ATTN_EP_FWD_LSE && entry != LA_ATTN_EP_FWD_RELPOS_LSE) || c.lse) &&
                    (entry != LA_ATTN_EP_FWD_RELPOS_LSE || (c.relh && c.relw)),
                "%s: null pointer", who);
  if (attn_check_shape(who, entry <= LA_ATTN_EP_FWD_ROWS, c, err, errsz) != 0) return -1;
  const int G = c.G, T = c.T;
  const bool grid_ok = G > 0 && G <= 64 && G * G == T;
  if (entry == LA_ATTN_EP_FWD_RELPOS_LSE) LA_PLAN_CHECK(grid_ok, "%s: rel-pos needs T == G*G, G <= 64 (T=%d G=%d)", who, T, G);
  LA_PLAN_CHECK(c.dt == LA_F16 || c.dt == LA_BF16, "%s: bad dtype %d", who, c.dt);
  const bool tables = c.tabh && c.tabw;
  p->n = 1, p->repeat = 1;
  if (c.mode == LA_ATTN_PLAIN) {
    p->launch[0] = attn_fwd_tile_launch(ATTN_NOBIAS, rows, c);
  } else if (c.mode == LA_ATTN_RELPOS_WIN16 && entry <= LA_ATTN_EP_FWD_ROWS) {
    LA_PLAN_CHECK(tables && G > 0 && G <= 16 && G * G == T && c.Tpad >= 16 * G,
                  "%s: WIN16 needs the tables, T == G*G, G <= 16 and Tpad >= 16*G (T=%d G=%d Tpad=%d)", who, T, G, c.Tpad);
    if (rows && c.imgH > 0) {       // windows addressed in image order
      const int nw = ((c.imgH + G - 1) / G) * ((c.imgW + G - 1) / G);
      LA_PLAN_CHECK(c.imgW > 0 && c.padrow && c.B % nw == 0, "%s: image-order windows need imgW, padrow and B = images * %d windows", who, nw);
    }
    p->launch[0] = attn_fwd_tile_launch(ATTN_TABLES_WIN16, rows, c);
  } else if (c.mode == LA_ATTN_RELPOS && rows) {
    LA_PLAN_CHECK(tables && G == 64 && T == 4096, "%s: rel-pos form needs the tables and the 64 x 64 grid (G=%d T=%d)", who, G, T);
    p->launch[0] = attn_fwd_tile_launch(ATTN_TABLES_ROW64, true, c);
  } else if (c.mode == LA_ATTN_RELPOS) {
    LA_PLAN_CHECK(grid_ok, "%s: rel-pos needs T == G*G, G <= 64 (T=%d G=%d)", who, T, G);
    if (tables && G <= 16) {          // windows: bias terms computed in-kernel from the tables (the no-LDS window kernel is 64-wide only)
      p->launch[0] = attn_nh(c) == 1 ? attn_window_launch(c) : attn_fwd_tile_launch(ATTN_TABLES_WIN, false, c);
    } else if (tables && G == 64) {   // global blocks: terms computed in the prologue of each query tile
      p->launch[0] = attn_fwd_tile_launch(ATTN_TABLES_ROW64, false, c);
    } else {
      LA_PLAN_CHECK(c.relh && c.relw, "%s: rel-pos terms missing (run la_relpos_terms, or pass the tables for G <= 16 / G == 64)", who);
      p->launch[0] = attn_fwd_tile_launch(G == 64 ? ATTN_TERMS_ROW64 : ATTN_TERMS, false, c);
    }
  } else {
    LA_PLAN_CHECK(false, "%s: bad mode %d", who, c.mode);
  }
  return 0;
}

// la_attn_bwd, la_attn_bwd_relpos: attn_bwd_dq_kernel (first: it writes D), then attn_bwd_dkv_kernel; one workgroup per 128 rows each.
// la_relpos_bwd: one launch per 64-column block of the head (p->repeat), all with the same kernel, grid and LDS
static inline int attn_bwd_plan(int entry, const LaAttnCall& c, LaAttnPlan* p, char* err, size_t errsz) {
  *p = LaAttnPlan{};
  const char* who = attn_entry_name(entry);
  const int G = c.G;
  LA_PLAN_CHECK(entry >= LA_ATTN_EP_BWD && entry <= LA_ATTN_EP_RELPOS_BWD, "la_attn_bwd_plan: bad entry point %d", entry);
  p->n = 1, p->repeat = 1, p->ry = 1;
  if (entry == LA_ATTN_EP_RELPOS_BWD) {
    LA_PLAN_CHECK(c.qkv && c.dqkv && c.drelh && c.drelw && c.tabh && c.tabw && c.dtabh && c.dtabw, "%s: null pointer", who);
    LA_PLAN_CHECK(c.B > 0 && c.heads > 0 && G > 0 && G <= 64 && (c.E == c.heads * 64 || c.E == c.heads * 128),
                  "%s: needs head_dim 64 or 128 (tables [(2 G - 1), head_dim] fp32), G <= 64 (E=%d heads=%d G=%d)", who, c.E, c.heads, G);
    LA_PLAN_CHECK(c.dt == LA_F16 || c.dt == LA_BF16, "%s: bad dtype %d", who, c.dt);
    p->repeat = attn_nh(c);
    if (G <= 16) {      // the windows: dense products over units of 32 queries, a wave per unit
      // the tables Rh | Rw as [64][64] fp32 (later their gradients) + per wave: drelh | drelw [32][G] fp32 and the q rows [32][64] 16 bit of its unit
      const int lds = 64 * 64 * (int)sizeof(float) + 4 * (2 * 32 * G * (int)sizeof(float) + 32 * 64 * 2);
      const int nunits = c.B * c.heads * ((G * G + 31) / 32);
      const int grid = nunits / 4 < 512 ? (nunits + 3) / 4 : 512;          // (256 / 512 / 768 workgroups on 100 x 12 windows: 135 / 117 / 132 us)
      p->launch[0] = LaAttnLaunch{LA_ATTN_K_RELPOS_BWD_ROWS, 0, 1, 0, grid, ATTN_BLOCK, lds};
      return 0;
    }
    // drelh | drelw of a row's queries [G][G + 1] fp32 each + dRh of the workgroup's rows [(2 G - 1)][64] fp32 + the row's q [G][64] 16 bit:
    // 73 KiB at G = 64, two workgroups per CU
    const int lds = (2 * G * (G + 1) + (2 * G - 1) * 64) * (int)sizeof(float) + G * 64 * 2;
    // rows per workgroup.  Large grids (G == 64: 4 image-heads x 64 rows per CU): as many as keep >= ~3 workgroups per CU in the launch - the
    // table atomics shrink by that factor.  Windows (G <= 32, tables of a few KiB, workgroups of 10 KiB): one row each - a row's three
    // dependent global round trips (operands in, dq read-modify-write) are what it waits for, and only more resident workgroups hide them
    // (measured on 100 x 12 windows of 14 x 14: 471 us with 14 rows per workgroup)
    int ry = 1;
    while (G > 32 && ry < G && (long)c.B * c.heads * ((G + 2 * ry - 1) / (2 * ry)) >= 768) ry *= 2;
    p->ry = ry;
    p->launch[0] = LaAttnLaunch{LA_ATTN_K_RELPOS_BWD, 0, 1, 0, c.B * c.heads * ((G + ry - 1) / ry), ATTN_BLOCK, lds};
    return 0;
  }
  const bool relpos = entry == LA_ATTN_EP_BWD_RELPOS;
  LA_PLAN_CHECK(c.qkv && c.out16 && c.dout16 && c.lse && c.dvec && c.dqkv && (!relpos || (c.relh && c.relw && c.drelh && c.drelw)), "%s: null pointer", who);
  if (attn_check_shape(who, false, c, err, errsz) != 0) return -1;
  if (relpos) LA_PLAN_CHECK(G * G == c.T && (G <= 32 || G == 64), "%s: T == G*G with G <= 32 or G == 64 (T=%d G=%d)", who, c.T, G);
  LA_PLAN_CHECK(c.dt == LA_F16 || c.dt == LA_BF16, "%s: bad dtype %d", who, c.dt);
  const int nh = attn_nh(c), nblk = attn_blocks128(c);
  const int bias = !relpos ? ATTN_BWD_NOBIAS : G == 64 ? ATTN_BWD_ROW64 : G <= 16 ? ATTN_BWD_WIN16 : ATTN_BWD_TERMS;
  const int keyinfo = c.Tpad * (int)sizeof(int);
  // dq: two stages of K rows | V rows (nh tiles each) + TERMS: relh | relw | d relh | d relw rows [32][G + 1] fp32 per wave; WIN16: the 0 / 1
  // matrix E^T [32][Tpad] 16 bit, rows padded by 16 bytes; both with the key lookup
  const int lds_dq = 2 * 2 * nh * TILE_B + (bias == ATTN_BWD_TERMS   ? 4 * 4 * 32 * (G + 1) * (int)sizeof(float) + keyinfo
                                            : bias == ATTN_BWD_WIN16 ? 32 * (c.Tpad * 2 + 16) + keyinfo
                                                                     : 0);
  // dk / dv: two stages of Q rows | dO rows (nh tiles each) + LSE | D of the tile's 64 queries (512 B); staged bias terms (even G: 16-byte
  // aligned rows of 64 queries) add relw 16 KiB + relh 1 KiB per stage - 67 KiB: two workgroups per CU (wide heads: 99 KiB, one)
  const bool staged = relpos && (G & 1) == 0;
  const int lds_dkv = 2 * (2 * nh * TILE_B + 512 + (staged ? 16384 + 1024 : 0));
  p->n = 2;
  p->launch[0] = LaAttnLaunch{LA_ATTN_K_BWD_DQ, bias, nh, 0, nblk, ATTN_BLOCK, lds_dq};
  p->launch[1] = LaAttnLaunch{LA_ATTN_K_BWD_DKV, staged ? ATTN_DKV_STAGED : relpos ? ATTN_DKV_TERMS : ATTN_DKV_NOBIAS, nh, 0, nblk, ATTN_BLOCK, lds_dkv};
  return 0;
}

#undef LA_PLAN_CHECK
}  // namespace la
