// Which kernel a la_gemm call gets, as one pure function of its arguments: argument checks, kernel family, compile-time epilogue, grid.
// Host only: no environment, no statics, no device queries, and the operand pointers are only tested for null and alignment - the same
// plan comes out on a machine without a GPU (la_gemm_plan, tests/test_gemm_plan_cpu.py).  la_gemm launches what the plan says.
#pragma once
#include <cstdint>
#include <cstdio>
#include "../../include/la_hip.h"

namespace la {

#define LA_PLAN_CHECK(cond, ...) \
  do { if (!(cond)) { snprintf(err, errsz, __VA_ARGS__); return -1; } } while (0)

template <typename P> static inline bool al16(P p) { return ((uintptr_t)p & 15) == 0; }      // a pointer or an address
static inline long tiles_of(int M, int N, int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn); }

// the 64-deep main loops (t256q, t256w): whole 64-wide k-tiles, at least two of them, and A periods that do not cut one
static inline bool k64_ok(int K, int a_kmod) { return (K % 64) == 0 && K >= 128 && (a_kmod == 0 || (a_kmod % 64) == 0); }

// the LDS-staged / slab epilogues move 8 columns per lane: 16-byte aligned rows of every buffer they touch
static inline bool epi_vec_ok(int N, const LaGemmEpilogue& e, int elt_bytes) {
  return (N % 8) == 0 && (!e.bias || al16(e.bias)) && (!e.res || (al16(e.res) && (e.ldr % 4) == 0)) &&
         (!e.out32 || (al16(e.out32) && (e.ld32 % 4) == 0)) && (!e.out16 || (al16(e.out16) && (e.ld16 % (16 / elt_bytes)) == 0)) &&
         (e.map != LA_MAP_CONVT2X2 || (e.p2 % 8) == 0) && (!e.vt || ((e.vt_col0 % 128) == 0 && (e.vt_Tpad % 4) == 0 && al16(e.vt)));
}

// LDS-DMA operands: 16-byte aligned, and every row reachable with a 32-bit byte offset from the base
static inline bool dma_operands_ok(uintptr_t A, int lda, uintptr_t W, int ldw, int M, int N) {
  return (size_t)M * lda * 2 < (1ull << 32) && (size_t)N * ldw * 2 < (1ull << 32) && al16(A) && al16(W);
}
static inline bool fast_ok(uintptr_t A, int lda, uintptr_t W, int ldw, int M, int N, int K, const LaGemmEpilogue& e) {
  return (K % 64) == 0 && dma_operands_ok(A, lda, W, ldw, M, N) && epi_vec_ok(N, e, 2);
}

// (the persistent four-wave kernel pays off from one 256 x 256 tile per CU)
static inline bool fused_act_ok(int M, int N, int K, int ncu, int variant) {
  return M > 0 && (N % 256) == 0 && k64_ok(K, 0) && tiles_of(M, N, 256, 256) >= ncu && (variant & 0xff) == 2;
}

// row panels per tile group (tile_coords); measured flat within +-2 % for 1..16 on the 256 x 128 / 128 x 128 kernels (8)
// and ~2 % better at 1..4 for the 256 x 256 kernels (2 there) - except, on the 64-deep ones, with >= 10 column tiles (lin1: N = 3072), where 8 row
// panels per group fetch 25 % less through the L2 (1.77 -> 1.33 M KiB of FETCH_SIZE per launch, tools/gemm_group_m.sh: with 2 row panels
// per group an XCD streams the whole 4.7 MB weight for every pair of panels) and run 1.3 % faster; lin2 / proj (3 column tiles) fetch
// and run worse beyond 2.  0: the kernel takes its tiles in row-major order
static inline int group_m(int kernel, int N) {
  if (kernel == LA_GEMM_DMA128 || kernel == LA_GEMM_DMA256x128) return 8;
  if (kernel == LA_GEMM_T256Q || kernel == LA_GEMM_T256W) return N >= 2560 ? 8 : 2;
  return kernel == LA_GEMM_T256 || kernel == LA_GEMM_T256P ? 2 : 0;
}

// MFMA shape of the four-wave main loop (LaGemmPlan.mfma): 1 = v_mfma_f32_16x16x32 instead of 32x32x16 - same sums bit for bit
// (tests/test_mfma_shape_gpu.py), half the passes per instruction, and a higher clock under the power limit.  Only the direct epilogue
// has the 16 x 16 accumulator layout; EPI 12 and the ragged EPI 9 instance spill on that shape (hipcc -S: 16 / 8 bytes of scratch, the
// former reloaded inside the tile loop) and stay as they are.  MEASURED per launch against the parent build (fp16, 393216 rows = whole
// tiles, three alternations, kept where the median gain exceeds twice the larger min-to-max range; profiles/r12_mfma_shape.md):
// q | k | v (EPI 1, 8) + 4.5 - 5.6 %, lin1 (EPI 2, 9) + 2.9 - 4.4 %, lin2 (K = 3072; EPI 3, 7, 11) + 4.9 - 5.5 %, the bare 8192^3 + 5.9 %;
// NOT the short products behind a residual epilogue (proj, N = K = 768: EPI 3 + 1.2 %, plane pairs in place + 1.5 % - inside twice
// the ranges; the epilogue's HBM round trips bound them), which stay on 32x32x16 below K = 1536.  EXTRAPOLATED from those, not timed
// (same main loop, an epilogue whose only shape-dependent step is the slab dump): EPI 5 / 6 (the training GELU forms), EPI 10 from
// K = 1536, every ragged instance (hipcc -S epilogue instruction counts equal to the 32x32x16 twins except ragged EPI 7, + 244 of 5171, and
// ragged EPI 10, + 49 - both only from K = 1536, where a tile's main loop is ~130 k cycles), and all bf16 instances
static inline int w4_mfma_shape(int direct, int epi, int ragged, int K, int variant) {
  const bool res_epi = epi == 3 || epi == 7 || epi == 10 || epi == 11;
  return direct && epi != 12 && !(epi == 9 && ragged) && !(res_epi && K < 1536) && !(variant & LA_GEMM_VARIANT_MFMA32) ? 1 : 0;
}

// persistent kernels: one workgroup per CU walks the tiles
static inline int persistent_grid(long ntiles, int ncu) { return ntiles < ncu ? (int)ntiles : ncu; }

// split-K (t256q EPI 4): nkt k-tiles in chunks of c (every chunk, the last included, at least 2 deep), `want` chunks = ONE round of
// tiles over the chip.  Every chunk ends in 64 K fp32 atomics on its output tile, and the chunks of a tile serialise on them in L2: with
// K = 46912 and 9 output tiles, 16 / 28 / 32 / 64 / 114 chunks measured 97 / - / 131 / 155 / 210 us (more than one round also pays the
// tile quantisation)
static inline void ksplit_chunks(int nkt, int want, LaGemmPlan* p) {
  if (want > nkt / 2) want = nkt / 2;
  if (want < 1) want = 1;
  int c = (nkt + want - 1) / want;
  if (c < 2) c = 2;
  while (c < nkt && (nkt % c) == 1) ++c;
  if (c > nkt) c = nkt;
  p->kchunk = c * 64;
  p->ksplit = (nkt + c - 1) / c;
}

// the two-dimensional grids.  gemm_f32_small: 32 x 32 wave tiles, one per workgroup when its four waves split K (K >= 1024), else 2 x 2;
// gemm_skinny: a wave per 4 columns - one (K >= 1024: the lanes stride K four wide) or four waves' columns per workgroup - and 32 rows
struct dim2 { int x, y; };
static inline dim2 f32_small_grid(int M, int N, int K) {
  return K >= 1024 ? dim2{(N + 31) / 32, (M + 31) / 32} : dim2{(N + 63) / 64, (M + 63) / 64};
}
static inline dim2 skinny_grid(int M, int N, int K) {
  const int groups = (N + 3) / 4;
  return dim2{K >= 1024 ? groups : (groups + 3) / 4, M > 32 ? (M + 31) / 32 : 1};
}

// tile, threads and dynamic LDS (one / two weight planes) of the tile kernels, by LaGemmPlan.kernel
struct KernelShape { int bm, bn, block, lds, lds2; };
constexpr KernelShape KERNEL_SHAPE[] = {
    {128, 128, 256, 65536, 0},                                                // NT: two 32 KiB stages
    {128, 128, 256, 128 * 132 * 4, 0},                                        // DMA128: two stages < the fp32 [128][132] epilogue chunk
    {256, 128, 256, 3 * 24576, 0},                                            // DMA256x128: three 24 KiB stages >= 67.5 KiB epilogue chunk
    {256, 256, 512, 136 * 1024, 3 * 49152},                                   // T256: ring 128 / 144 KiB; epilogue: two staging buffers of 65 KiB
    {256, 256, 512, 4 * 32768 + 8 * 512 + 8 * 2048, 3 * 49152 + 8 * 2048},    // T256P: ring + 2 KiB slab per wave (+ row tables): 148 / 160 KiB
    {256, 256, 512, 2 * 65536 + 8 * 2048 + 8 * 512, 0},                       // T256Q: two k-tile buffers + 2 KiB slab per wave + row tables: 148 KiB
    {256, 256, 256, 4 * 32768 + 4 * 8192, 0},                                 // T256W: two k-tile buffers + 8 KiB slab per wave: all 160 KiB
    {128, 32, 256, 2 * (128 + 32) * 128, 0},                                  // F32_N32: two stages of (128 + BN) 128-byte rows ...
    {128, 128, 256, 128 * 132 * 4, 0},                                        // F32_N128: ... / the fp32 [128][BN + 4] epilogue chunk
};

// grid, block, dynamic LDS and tile grouping of `kernel` (p->planes, p->ksplit set)
static inline void plan_launch(LaGemmPlan* p, int kernel, int M, int N, int K, int ncu, int variant) {
  p->kernel = kernel;
  p->gm = group_m(kernel, N);
  if (kernel == LA_GEMM_F32_SMALL || kernel == LA_GEMM_SKINNY) {
    const dim2 g = kernel == LA_GEMM_SKINNY ? skinny_grid(M, N, K) : f32_small_grid(M, N, K);
    p->grid = g.x * g.y, p->block = 256, p->lds_bytes = 0;
    return;
  }
  const KernelShape& s = KERNEL_SHAPE[kernel];
  const long tiles = tiles_of(M, N, s.bm, s.bn) * p->ksplit;
  p->grid = kernel >= LA_GEMM_T256P && kernel <= LA_GEMM_T256W ? persistent_grid(tiles, ncu) : (int)tiles;
  p->block = s.block, p->lds_bytes = p->planes == 2 ? s.lds2 : s.lds;
  if (kernel == LA_GEMM_T256Q) p->gm |= variant & 0x800500;
}

// The 256 x 256 tile kernels (K = depth of ONE plane).  The compile-time epilogue that covers the call (see epilogue_t256), then the main loop:
// persistent workgroups when the epilogue is one of the hot three and the tiles are whole in N, and among the persistent kernels the 64-deep
// ones on single-plane shapes (la_gemm_variant: 2 (default) = the four-wave kernel - gemm_w4.hip; its own epilogue on interior unmapped tiles -
// lin1, lin2, proj - and epilogue_wave elsewhere: measured ahead of the eight-wave kernel on every encoder shape, profiles/r05_notes.md -,
// 1 = the eight-wave quadrant-phase kernel, 0 = the BK 32 kernel everywhere)
static inline void plan_t256(LaGemmPlan* p, int planes, int M, int N, int K, const LaGemmEpilogue& e, int ncu, int variant, bool persistent = true) {
  const int var = variant & 0xff;
  const bool plain = e.map == LA_MAP_NONE && e.res_mod == 0;
  const bool only16 = !e.res && !e.out32 && e.out16;
  const bool plain16 = plain && only16 && e.act == LA_ACT_NONE, gelu16 = plain && only16 && e.act == LA_ACT_GELU && !e.vt;
  // qkv of a SAM window block from image-order tokens: rows scattered into window order by the epilogue (no padded rows multiplied)
  const bool scatter = e.map == LA_MAP_WINDOW_PART && e.res_mod == 0 && e.amap == LA_MAP_NONE && only16 && e.act == LA_ACT_NONE &&
                       (planes == 1 || (e.vt && e.vt_col0 == 0)) &&
                       (!e.vt || (size_t)((M + e.vt_T - 1) / e.vt_T + 4096) * e.vt_heads * e.vt_hd * e.vt_Tpad < (1ull << 32));
  // a residual that repeats every res_mod rows (the patch embedding's position table: one row per token of the image) stays on the
  // persistent four-wave kernel when whole 256-row tiles sit inside one period - its direct epilogue takes the residual rows modulo
  const bool w4_resmod = planes == 1 && e.map == LA_MAP_NONE && e.res_mod > 0 && (e.res_mod % 256) == 0 && (M % 256) == 0 && e.res && var == 2 &&
                         k64_ok(K, e.a_kmod) && !((variant >> 8) & 1);
  // (fp32 atomics from the accumulator layout instead of the read-modify-write through the slab were measured in round 4 and are
  // slower: profiles/r04_notes.md 1)
  const bool f32 = (plain || w4_resmod) && e.act == LA_ACT_NONE && e.out32 && !e.vt && (e.ld32 % 4) == 0 && (!e.res || (e.ldr % 4) == 0);
  const int pepi = (plain16 || scatter) ? 1 : gelu16 ? 2 : f32 ? 3 : 0;
  p->planes = planes, p->epi = pepi;
  if (!(persistent && pepi && (N % 256) == 0 && K / 32 >= 8 && (e.ld16 % 8) == 0)) {
    p->epi = plain16 ? 1 : gelu16 ? 2 : (plain && e.act == LA_ACT_NONE && e.res && e.out32 && !e.vt) ? 3 : 0;
    return plan_launch(p, LA_GEMM_T256, M, N, K, ncu, variant);
  }
  const bool k64 = planes == 1 && k64_ok(K, e.a_kmod);
  plan_launch(p, k64 && var == 2 ? LA_GEMM_T256W : k64 && var >= 1 ? LA_GEMM_T256Q : LA_GEMM_T256P, M, N, K, ncu, variant);
  if (p->kernel == LA_GEMM_T256W) {
    // (a ragged last row tile - M % 256 != 0: the HF encoders' 57664 = 225.25 tiles - stays on the direct epilogue: its loads and stores are
    // predicated on the row; a residual modulo res_mod needs whole tiles inside a period and is only sent here with M % 256 == 0)
    p->gm |= variant & 0xf500;
    p->direct = e.map == LA_MAP_NONE && !e.vt && !((variant >> 8) & 1);
    p->ragged = p->direct && (M & 255) != 0;
    p->mfma = w4_mfma_shape(p->direct, p->epi, p->ragged, K, variant);
  }
}

// the fused epilogues of the four-wave kernel (EPI 5 - 12: direct epilogue only)
static inline void plan_w4_fused(LaGemmPlan* p, int epi, int M, int N, int K, int ncu, int variant) {
  p->epi = epi, p->direct = 1, p->ragged = (M & 255) != 0;
  p->mfma = w4_mfma_shape(1, epi, p->ragged, K, variant);
  plan_launch(p, LA_GEMM_T256W, M, N, K, ncu, variant);
}

// the 16-bit tile kernels, by shape
static inline void plan_tiles16(LaGemmPlan* p, uintptr_t A, int lda, uintptr_t W, int ldw, int M, int N, int K, const LaGemmEpilogue& e, int ncu,
                                int variant) {
  if (!fast_ok(A, lda, W, ldw, M, N, K, e)) return plan_launch(p, LA_GEMM_NT, M, N, K, ncu, variant);       // register staged: any K % 8, N, alignment
  // two weight planes against one A ([W_hi | W_lo], a_kmod = K / 2): the 256 x 256 two-plane kernel, which reuses every A fragment
  // for both planes ... and, measured on MI355X (tools/gemm_planes_bench.py), its single-plane form beats the 256 x 128 and the 128 x 128
  // kernel on every shape with >= 2 full rounds of 256 x 256 tiles (K = 768: +10-15 %, K = 3072: equal)
  const int planes = (e.a_kmod > 0 && K == 2 * e.a_kmod) ? 2 : 1;
  if (tiles_of(M, N, 256, 256) >= (planes == 2 ? 128 : 512) && (!e.vt || (e.vt_col0 % 256) == 0)) return plan_t256(p, planes, M, N, K / planes, e, ncu, variant);
  // measured on MI355X (profiles/r01_gemm_variants.log): the 256x128 / 128x64-per-wave kernel wins by ~5 % on the short-K
  // (K = 768) shapes once there are >= 2 full waves of tiles; the 128x128 kernel wins on long K and small grids.
  plan_launch(p, K <= 1536 && tiles_of(M, N, 256, 128) >= 512 ? LA_GEMM_DMA256x128 : LA_GEMM_DMA128, M, N, K, ncu, variant);
}

// exact-fp32 MFMA tiles (also la_conv3x3_f32)
static inline void plan_f32(LaGemmPlan* p, int M, int N, int K, const LaGemmEpilogue& e) {
  p->epi = epi_vec_ok(N, e, 4) ? 1 : 0;
  plan_launch(p, N <= 32 ? LA_GEMM_F32_N32 : LA_GEMM_F32_N128, M, N, K, 0, 0);
}

static inline LaGemmPlan plan_default(int K) { return LaGemmPlan{LA_GEMM_NT, 0, 1, 0, 0, 0, 1, K, 0, 256, 0}; }

static inline int gemm_plan(uintptr_t A, int lda, uintptr_t W, int ldw, int M, int N, int K, const LaGemmEpilogue& e, int dt, int ncu, int variant,
                            LaGemmPlan* p, char* err, size_t errsz) {
  *p = plan_default(K);
  LA_PLAN_CHECK(A && W, "la_gemm: null pointer");
  LA_PLAN_CHECK(M > 0 && N > 0 && K > 0, "la_gemm: bad shape M=%d N=%d K=%d", M, N, K);
  // (the four-wave epilogue reaches the 128 rows of a wave's block with 32-bit byte offsets from the tile's base: 128 x ld x 4 B < 2^31)
  LA_PLAN_CHECK(e.ld16 < (1 << 22) && e.ldaux < (1 << 22) && e.ld32 < (1 << 22) && e.ldr < (1 << 22) && N < (1 << 22),
                "la_gemm: output / residual leading dimensions must be below %d elements", 1 << 22);
  const int kq = (dt == LA_F32) ? 4 : 8;
  LA_PLAN_CHECK((K % kq) == 0 && (lda % kq) == 0 && (ldw % kq) == 0, "la_gemm: K, lda, ldw must be multiples of %d (K=%d lda=%d ldw=%d)", kq, K,
                lda, ldw);
  LA_PLAN_CHECK(e.out32 || e.out16 || e.vt, "la_gemm: no output");
  LA_PLAN_CHECK(e.a_kmod == 0 || (dt != LA_F32 && e.a_kmod > 0 && (e.a_kmod % 64) == 0 && e.a_kmod <= K && lda >= e.a_kmod && M > 32),
                "la_gemm: a_kmod=%d must be a multiple of 64, <= K=%d and <= lda=%d (16-bit operands, M > 32)", e.a_kmod, K, lda);
  LA_PLAN_CHECK(dt == LA_F16 || dt == LA_BF16 || dt == LA_F32, "la_gemm: bad dtype %d", dt);
  LA_PLAN_CHECK(e.amap == LA_MAP_NONE || (e.amap == LA_MAP_WINDOW_PART && e.map == LA_MAP_NONE && dt != LA_F32) ||
                    (e.amap == LA_MAP_CONV3X3 && e.map == LA_MAP_NONE && dt == LA_F16 && e.a_kmod == 0 && e.p1 > 0 && (e.p1 % 64) == 0 &&
                     K == 27 * e.p1 && e.p2 == lda && lda == 2 * e.p1 && e.p0 > 2 && (N % 256) == 0 && !e.vt && e.ksplit == 0 && M > 512),
                "la_gemm: amap must be LA_MAP_NONE, LA_MAP_WINDOW_PART (16-bit operands, no output map) or LA_MAP_CONV3X3 (fp16 plane pairs, p0 = padded "
                "width, p1 = C %% 64 == 0, p2 = lda = 2 C, K = 27 C, N %% 256 == 0), got amap=%d map=%d dt=%d", e.amap, e.map, dt);
  LA_PLAN_CHECK(e.act != LA_ACT_GELU_BWD || e.aux16, "la_gemm: LA_ACT_GELU_BWD needs aux16 (the saved pre-activation)");
  const bool rows16 = (e.ld16 % 8) == 0 && e.ld16 >= N && al16(e.out16);      // (NULL is aligned: out16 itself is tested where it is required)
  if (e.aux16 && !e.nstat_out) {
    // the training forms of the MLP's GELU (see LaGemmEpilogue.aux16): the direct epilogue of the persistent four-wave kernel only
    LA_PLAN_CHECK(e.act == LA_ACT_GELU || e.act == LA_ACT_GELU_BWD, "la_gemm: aux16 goes with LA_ACT_GELU (written) or LA_ACT_GELU_BWD (read)");
    LA_PLAN_CHECK(dt != LA_F32 && fused_act_ok(M, N, K, ncu, variant) && fast_ok(A, lda, W, ldw, M, N, K, e),
                  "la_gemm: aux16 needs 16-bit operands and a shape la_gemm_fused_act_ok() accepts (M=%d N=%d K=%d)", M, N, K);
    LA_PLAN_CHECK(e.out16 && !e.out32 && !e.res && !e.vt && e.map == LA_MAP_NONE && e.amap == LA_MAP_NONE && e.a_kmod == 0 && e.ksplit == 0 && rows16 &&
                      (e.ldaux % 8) == 0 && e.ldaux >= N && al16(e.aux16),
                  "la_gemm: aux16 forms write out16 only (no residual / fp32 output / maps / V^T / planes), rows 16-byte aligned");
    LA_PLAN_CHECK(e.act == LA_ACT_GELU || !e.bias, "la_gemm: LA_ACT_GELU_BWD takes no bias");
    plan_w4_fused(p, e.act == LA_ACT_GELU ? 5 : 6, M, N, K, ncu, variant);
    return 0;
  }
  if (e.nstat_out || e.nstat_in || e.rvec) {
    // LayerNorm folded into its neighbour GEMMs (see LaGemmEpilogue.nstat_out): the direct epilogue of the persistent four-wave kernel only
    LA_PLAN_CHECK(dt == LA_F16 && (N % 256) == 0 && k64_ok(K, e.a_kmod) && fast_ok(A, lda, W, ldw, M, N, K, e) && (variant & 0xff) == 2,
                  "la_gemm: nstat_out / nstat_in need fp16 operands, N %% 256 == 0, K %% 64 == 0, K >= 128, 16-byte aligned rows (M=%d N=%d K=%d)", M,
                  N, K);
    LA_PLAN_CHECK(!e.vt && e.map == LA_MAP_NONE && e.amap == LA_MAP_NONE && e.ksplit == 0 && !(e.nstat_out && e.nstat_in) &&
                      (!e.aux16 || (e.nstat_out && (e.ldaux % 8) == 0 && e.ldaux >= N && al16(e.aux16))),
                  "la_gemm: nstat_out / nstat_in take no row maps / V^T / ksplit, not both at once; aux16 only with nstat_out (the lo plane, 16-byte aligned rows)");
    const bool stat8 = (reinterpret_cast<uintptr_t>(e.nstat_out) & 7) == 0;
    const bool rvec_ok = !e.rvec || (e.rvec_rpg > 0 && al16(e.rvec) && ((e.rvec_rpg % 256) == 0 || e.rvec_rpg >= 128));
    const bool rvec_split = e.rvec && (e.rvec_rpg % 256) != 0;       // groups that end inside a 256-row tile
    int epi;
    if (e.nstat_in) {
      LA_PLAN_CHECK(e.ncol && e.out16 && !e.out32 && !e.res && !e.rvec && (e.act == LA_ACT_NONE || e.act == LA_ACT_GELU) && rows16 && al16(e.nstat_in) &&
                        al16(e.ncol) && e.a_kmod == 0,
                    "la_gemm: nstat_in writes out16 only (act NONE / GELU), needs ncol, one weight plane");
      epi = e.act == LA_ACT_GELU ? 9 : 8;
    } else if (e.nstat_out && !e.out32 && e.res && e.aux16) {
      // fp32 residual in (the position table of the patch embedding), plane pairs out, no fp32 matrix at all
      LA_PLAN_CHECK(e.out16 && e.act == LA_ACT_NONE && rows16 && (e.ldr % 4) == 0 && stat8 && !e.rvec,
                    "la_gemm: nstat_out with a residual and no out32 writes plane pairs only (out16 + aux16), no group vector");
      LA_PLAN_CHECK(e.res_mod == 0 || ((e.res_mod % 256) == 0 && (M % 256) == 0),
                    "la_gemm: nstat_out with a periodic residual needs res_mod %% 256 == 0 and M %% 256 == 0 (res_mod=%d M=%d)", e.res_mod, M);
      epi = 7;
    } else if (e.nstat_out && !e.out32 && !e.res) {
      // the stream as fp16 plane pairs, read-modify-written in place: out16 = hi plane, aux16 = lo plane (see LaGemmEpilogue.nstat_out)
      LA_PLAN_CHECK(e.out16 && e.aux16 && e.act == LA_ACT_NONE && rows16 && (e.ldaux % 8) == 0 && e.ldaux >= N && al16(e.aux16) && stat8 && e.res_mod == 0,
                    "la_gemm: nstat_out without out32 / res updates a plane-pair stream in place: out16 (hi) and aux16 (lo), 16-byte aligned rows");
      LA_PLAN_CHECK(rvec_ok, "la_gemm: rvec needs a 16-byte aligned vector and groups of whole 256-row tiles or of at least 128 rows (rvec_rpg=%d)",
                    e.rvec_rpg);
      epi = rvec_split ? 12 : 11;
    } else {
      LA_PLAN_CHECK(e.nstat_out && e.out32 && e.out16 && e.act == LA_ACT_NONE && rows16 && (e.ld32 % 4) == 0 && e.ld32 >= N && al16(e.out32) &&
                        (!e.res || (e.ldr % 4) == 0) && stat8,
                    "la_gemm: nstat_out goes with out32 + out16 (no activation), 16-byte aligned rows");
      LA_PLAN_CHECK(e.res_mod == 0 || ((e.res_mod % 256) == 0 && (M % 256) == 0 && e.res),
                    "la_gemm: nstat_out with a periodic residual needs res_mod %% 256 == 0 and M %% 256 == 0 (res_mod=%d M=%d)", e.res_mod, M);
      LA_PLAN_CHECK(rvec_ok, "la_gemm: rvec needs a 16-byte aligned vector and groups of whole 256-row tiles or of at least 128 rows (rvec_rpg=%d)",
                    e.rvec_rpg);
      epi = rvec_split ? 10 : 7;
    }
    plan_w4_fused(p, epi, M, N, K, ncu, variant);
    return 0;
  }
  // up to 512 fp32 rows (decoder tokens of many prompt pairs): an MFMA grid of 128 x 128 tiles is a handful of workgroups and leaves the
  // chip idle (240 x 256 x 2048: 155 us on four tiles) - 32 x 32 wave tiles (gemm_f32_small_kernel) above 128 rows, the VALU kernel below
  // (from 129 rows: up to 128 rows - the per-image vectors of the encoder's token-mean corrections, one row per image - stay on the VALU
  // kernel, whose lane-parallel partial sums round 4 x closer to fp64 than the MFMA's serial chain (9e-8 against 4e-7 on 52 x 768 x 1536);
  // the corrections accumulate over every block of the encoder and a 26- and a 52-image batch must not take different kernels:
  // tests/test_model_gpu.py::test_full_geometry_episode_properties measured 2.7e-4 on the cfg3 logits between the two)
  const bool few_rows = M <= 32 || (dt == LA_F32 && M <= 512 && tiles_of(M, N, 128, 128) < 64);
  if (few_rows && (K % 8) == 0 && e.map == LA_MAP_NONE && e.amap == LA_MAP_NONE && !e.vt) {
    // (K, lda, ldw are multiples of 4 with fp32 operands: float4 loads from 16-byte aligned bases)
    plan_launch(p, dt == LA_F32 && M > 128 && al16(A | W) ? LA_GEMM_F32_SMALL : LA_GEMM_SKINNY, M, N, K, ncu, variant);
    return 0;
  }
  if (dt == LA_F32) {
    LA_PLAN_CHECK(!e.vt, "la_gemm: the transposed-V epilogue is 16-bit only");
    plan_f32(p, M, N, K, e);
    return 0;
  }
  if (e.ksplit > 0) {
    // split-K accumulate (weight gradients): out32 += A . W^T with fp32 atomics, K cut into independent chunks: dW[N, K] = dY^T X over
    // 10^4 - 10^5 tokens has 9 - 36 output tiles only, the chunks are what fills the chip
    LA_PLAN_CHECK(e.out32 && !e.out16 && !e.res && !e.bias && !e.vt && e.act == LA_ACT_NONE &&
                      (e.map == LA_MAP_NONE || (e.map == LA_MAP_GROUP && e.p0 > 0)) && e.amap == LA_MAP_NONE && e.a_kmod == 0,
                  "la_gemm: ksplit accumulates the bare product into out32 (no bias / residual / activation / second output; row map none or LA_MAP_GROUP)");
    LA_PLAN_CHECK((N % 256) == 0 && k64_ok(K, 0) && dma_operands_ok(A, lda, W, ldw, M, N),
                  "la_gemm: ksplit needs N %% 256 == 0, K %% 64 == 0, K >= 128, 16-byte aligned operands below 4 GiB (M=%d N=%d K=%d)", M, N, K);
    p->epi = 4;
    ksplit_chunks(K / 64, ncu / (int)tiles_of(M, N, 256, 256), p);
    plan_launch(p, LA_GEMM_T256Q, M, N, K, ncu, variant);
    return 0;
  }
  plan_tiles16(p, A, lda, W, ldw, M, N, K, e, ncu, variant);
  return 0;
}

#undef LA_PLAN_CHECK
}  // namespace la
