// Fused stream MLP of the OneWayTransformer (models/transformer.py:149-152, common.py:19-37): on every row of the (B, hw, D) fp32 image
// stream,  x <- LayerNorm(x + relu(x W1^T + b1) W2^T + b2),  in place.  The H-wide hidden layer never reaches global memory.
//
// Numerics are those of la_twoway_i2t (twoway.hip): x and the hidden activations are split on the fly into fp16 planes (v = hi + lo), the
// weights arrive pre-split (hi = rn(W), lo = rn(W - hi)), every product is hi.hi + lo.hi + hi.lo on the fast MFMA with fp32 accumulation,
// the residual is the fp32 row as loaded and the LayerNorm (biased variance, fp32) is that kernel's epilogue.
//
// Shape.  A workgroup owns 128 rows and walks the hidden layer in chunks of 128 units:
//   phase A  h = x W1[chunk]^T          16 k16 slabs of the chunk's W1 rows; the x planes are staged 128 columns of K at a time from the rows
//                                       held in registers (as in twoway.hip: the planes of the whole tile would not leave room for a ring)
//   relu     relu(h + b1) -> [hi | lo] planes in the MFMA A-operand image, over the x planes
//   phase B  y += h W2[:, chunk]^T      8 k16 slabs of W2's columns; the D-wide accumulator lives in registers across all chunks
// and ends with the epilogue  y + b2 -> LDS row-major, one WAVE per row: + x (fp32, read again), LayerNorm, coalesced store.
// The 8 waves form a 4 x 2 grid - wave (rt, ch) multiplies row tile rt (32 rows) against column half ch of every product.  All slabs of
// the kernel, 24 per chunk, travel through ONE ring of three 16 KiB slots (LDS-DMA, issued two steps ahead across the phase and chunk
// boundaries).  Why 128 rows: a tile streams all four planes, 2 H D 2 bytes (4 MiB at H = 2048) against 128 KiB for Wq + Wo of the
// two-way kernel; 64 rows would do 96 FLOP per streamed byte, 128 rows do 192.  LDS: 64 KiB planes + 48 KiB ring, 130 KiB for the
// epilogue's row-major tile; one workgroup = two waves per SIMD, <= 256 registers per lane.  profiles/r12_oneway.md has the figures.
//
// An output row depends on its own input row and the weights alone: rows never mix in a product, the hidden chunks are summed in
// ascending order by one workgroup (no atomics, no second reduction), and rows beyond the end are computed on zeros and never stored.
#include <cstdlib>
#include "la_common.h"
#include "../../include/la_hip.h"

namespace la {

constexpr int SM_ROWS = 128;                  // stream rows per workgroup
constexpr int SM_WAVES = SM_ROWS / 16;        // 8: wave w loads, stages and normalises rows 16 w .. 16 w + 15
constexpr int SM_D = 256;                     // stream width
constexpr int SM_HC = 128;                    // hidden units per chunk
constexpr int SM_APL = SM_ROWS * 64;          // one 32-column plane chunk of the tile: 128 rows x 64 B = 8 KiB
constexpr int SM_PLANES = 2 * 4 * SM_APL;     // [hi | lo][4 chunks] = 128 columns of K: 64 KiB (x planes, then the hidden planes)
constexpr int SM_SLOT = 2 * SM_D * 32;        // a ring slot: the larger slab (W2: [hi | lo][256 rows][32 B]) = 16 KiB
constexpr int SM_YLD = SM_D + 4;
constexpr int SM_NA = SM_D / 16;              // k16 slabs of phase A
constexpr int SM_NB = SM_HC / 16;             // k16 slabs of phase B
constexpr int SM_LDS_MAIN = SM_PLANES + 3 * SM_SLOT;
constexpr int SM_LDS_Y = SM_ROWS * SM_YLD * 4;
constexpr int SM_LDS = SM_LDS_MAIN > SM_LDS_Y ? SM_LDS_MAIN : SM_LDS_Y;
static_assert(SM_LDS <= 160 * 1024, "stream MLP tile does not fit the LDS");

// 64-byte rows (32 halfs): 16-byte chunk c of row r in slot c ^ ((r >> 2) & 3) - conflict-free ds_read_b128 fragments (as twoway.hip)
__device__ __forceinline__ int sm_off(int row, int chunk) { return row * 64 + ((chunk ^ ((row >> 2) & 3)) << 4); }
// 32-byte rows of a k16 weight slab: 16-byte half c of row r in slot c ^ ((r >> 3) & 1)
__device__ __forceinline__ int sm_woff(int row, int c) { return row * 32 + ((c ^ ((row >> 3) & 1)) << 4); }

// hi / lo planes of 4 consecutive values, packed
__device__ __forceinline__ void sm_split4(float4 v, uint2& h, uint2& l) {
  const f16_t ha = (f16_t)v.x, hb = (f16_t)v.y, hc = (f16_t)v.z, hd = (f16_t)v.w;
  h.x = pack2<f16_t>(v.x, v.y);
  h.y = pack2<f16_t>(v.z, v.w);
  l.x = pack2<f16_t>(v.x - (float)ha, v.y - (float)hb);
  l.y = pack2<f16_t>(v.z - (float)hc, v.w - (float)hd);
}

// columns [128 half, +128) of this wave's 16 rows -> A-operand plane chunks [4][128 rows x 64 B] (hi at pa, lo at pa + 4 chunks); the 32
// lanes that hold those columns do the work
__device__ __forceinline__ void sm_stage(char* pa, int wave, int lane, int half, const uint2 (&xh)[16], const uint2 (&xl)[16]) {
  if ((lane >> 5) == half) {
    const int li = lane & 31;
    char* hi = pa + (li >> 3) * SM_APL;
    char* lo = hi + 4 * SM_APL;
    const int sub = (li & 1) * 8, c16 = (li & 7) >> 1;
#pragma unroll
    for (int rr = 0; rr < 16; ++rr) {
      const int off = sm_off(wave * 16 + rr, c16) + sub;
      *reinterpret_cast<uint2*>(hi + off) = xh[rr];
      *reinterpret_cast<uint2*>(lo + off) = xl[rr];
    }
  }
}

// One k16 slab of two weight planes with NR rows each: 16 consecutive K columns starting at k0 of rows [r0, r0 + NR), [plane][row][32 B]
// (sm_woff) at LDS byte address dst.  Pieces of 32 rows (1 KiB); the 8 waves take pieces wave, wave + 8, ...
template <int NR>
__device__ __forceinline__ void sm_dma_slab(const f16_t* hi, const f16_t* lo, int ldw, int r0, int k0, unsigned dst, int wave, int lane) {
  constexpr int PIECES = 2 * NR / 32;
  static_assert(PIECES % SM_WAVES == 0, "a slab is whole rounds of the workgroup's waves");
#pragma unroll
  for (int i = 0; i < PIECES / SM_WAVES; ++i) {
    const int piece = i * SM_WAVES + wave;
    const int plane = piece / (NR / 32), r = (piece % (NR / 32)) * 32 + (lane >> 1);
    const int c = (lane & 1) ^ ((r >> 3) & 1);
    dma16((plane ? lo : hi) + (size_t)(r0 + r) * ldw + k0 + c * 8, dst + piece * 1024);
  }
}

struct SmArgs {
  float* x;                          // [rows, D] in / out
  const f16_t *w1_hi, *w1_lo;        // [H, D]
  const f16_t *w2_hi, *w2_lo;        // [D, H]
  const float *b1, *b2, *gamma, *beta;
  float eps;
  long rows;
  int H;
};

__global__ __launch_bounds__(SM_WAVES * 64) void stream_mlp_kernel(SmArgs a) {
  constexpr int D = SM_D;
  constexpr int PWA = 2 * SM_HC / 32 / SM_WAVES, PWB = 2 * D / 32 / SM_WAVES;   // DMA pieces per wave of a W1 / W2 slab: 1, 2
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* pa = smem;                                   // x planes (phase A), hidden planes (phase B)
  float* yt = reinterpret_cast<float*>(smem);        // epilogue: [128][YLD]
  const int tid = threadIdx.x, lane0 = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rt = wave >> 1, ch = wave & 1;
  const long row0 = (long)blockIdx.x * SM_ROWS;
  const int H = a.H, NC = H / SM_HC;
  const unsigned lds_w = lds_addr_of(smem + SM_PLANES);

  // slab i of chunk c: i < 16 the W1 slab of K columns [16 i, +16), else the W2 slab of the chunk's hidden columns [16 (i - 16), +16);
  // slab s = 24 c + i of the kernel sits in ring slot s % 3 (24 % 3 == 0: the slot depends on i alone)
  auto issue = [&](int c, int i, int lane) {
    const unsigned dst = lds_w + (i % 3) * SM_SLOT;
    if (i < SM_NA) sm_dma_slab<SM_HC>(a.w1_hi, a.w1_lo, D, c * SM_HC, i * 16, dst, wave, lane);
    else sm_dma_slab<D>(a.w2_hi, a.w2_lo, H, 0, c * SM_HC + (i - SM_NA) * 16, dst, wave, lane);
  };
  issue(0, 0, lane0);
  issue(0, 1, lane0);
  // this wave's 16 rows: lane -> columns 4 lane .. 4 lane + 3 (rows beyond the end read as zero).  Phase A of EVERY chunk stages them, so
  // what the registers hold through the chunk loop is their packed fp16 planes (the split is done once); the epilogue reads the fp32
  // rows again for the residual - nothing has written them since - instead of holding another 64 registers per lane
  uint2 xh[16], xl[16];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const long row = row0 + wave * 16 + rr;
    const long rc = row < a.rows ? row : a.rows - 1;
    float4 v = *reinterpret_cast<const float4*>(a.x + (size_t)rc * D + lane0 * 4);
    if (row >= a.rows) v = make_float4(0.f, 0.f, 0.f, 0.f);
    sm_split4(v, xh[rr], xl[rr]);
  }
  f32x16 yacc[D / 64];
#pragma unroll
  for (int j = 0; j < D / 64; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) yacc[j][r] = 0.f;

  for (int c = 0; c < NC; ++c) {
    const bool last = c + 1 == NC;
    // (the lane index is laundered once per chunk: every LDS / DMA offset below is loop-invariant, and hoisted out of the chunk loop those
    // ~40 registers per lane pushed the accumulators into scratch memory)
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int fr = lane & 31, fh = lane >> 5;
    float bb[SM_HC / 64];
#pragma unroll
    for (int j = 0; j < SM_HC / 64; ++j) bb[j] = a.b1[c * SM_HC + ch * (SM_HC / 2) + j * 32 + fr];
    f32x16 hacc[SM_HC / 64];
#pragma unroll
    for (int j = 0; j < SM_HC / 64; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) hacc[j][r] = 0.f;
    // ---- phase A: h = x W1[chunk]^T ---------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int kk = 0; kk < SM_NA; ++kk) {
      // slab kk landed (slab kk + 1 may still travel: one piece per wave of a W1 slab, two of a W2 slab)
      if (kk + 1 < SM_NA) dma_wait<PWA>();
      else dma_wait<PWB>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                  // ... for every wave, and every wave is done with the step before
      asm volatile("" ::: "memory");
      issue(c, kk + 2, lane);                              // (kk + 2 <= 17: this chunk's slabs)
      if ((kk & 7) == 0) {                           // next 128 columns of the rows -> planes (the first time: waits for the row burst)
        sm_stage(pa, wave, lane, kk >> 3, xh, xl);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
      }
      const char* pw = smem + SM_PLANES + (kk % 3) * SM_SLOT;
      const char* pah = pa + ((kk >> 1) & 3) * SM_APL;
      const uint4 ah = *reinterpret_cast<const uint4*>(pah + sm_off(rt * 32 + fr, (kk & 1) * 2 + fh));
      const uint4 al = *reinterpret_cast<const uint4*>(pah + 4 * SM_APL + sm_off(rt * 32 + fr, (kk & 1) * 2 + fh));
#pragma unroll
      for (int j = 0; j < SM_HC / 64; ++j) {
        const int wr = ch * (SM_HC / 2) + j * 32 + fr;
        const uint4 wh = *reinterpret_cast<const uint4*>(pw + sm_woff(wr, fh));
        const uint4 wl = *reinterpret_cast<const uint4*>(pw + SM_HC * 32 + sm_woff(wr, fh));
        hacc[j] = Half16<f16_t>::mfma32(ah, wh, hacc[j]);
        hacc[j] = Half16<f16_t>::mfma32(al, wh, hacc[j]);
        hacc[j] = Half16<f16_t>::mfma32(ah, wl, hacc[j]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                    // every wave is done with the x planes: the hidden planes may overwrite them
    asm volatile("" ::: "memory");
    // ---- relu(h + b1) -> [hi | lo] planes in the A-operand image of the chunk's 32-column block oc: row = rt 32 + (r & 3) + 8 (r >> 2) +
    // 4 fh, column fr.  Lane pairs (fr, fr ^ 1) hold neighbouring columns: they trade halves over DPP, the even lane stores the hi dword
    // and the odd lane the lo dword of the pair (as the O planes of la_twoway_i2t)
#pragma unroll
    for (int j = 0; j < SM_HC / 64; ++j) {
      const int oc = ch * (SM_HC / 64) + j;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float hv0 = fmaxf(hacc[j][r] + bb[j], 0.f);
        const float hv = (float)(f16_t)hv0, lv = hv0 - hv;
        const float hn = dpp_mov<0xB1>(hv), ln = dpp_mov<0xB1>(lv);          // the neighbour's values
        const int row = rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        const int off = oc * SM_APL + sm_off(row, fr >> 3) + (fr & 6) * 2;
        const bool odd = fr & 1;
        const uint32_t w = odd ? pack2<f16_t>(ln, lv) : pack2<f16_t>(hv, hn);
        *reinterpret_cast<uint32_t*>(pa + (odd ? 4 * SM_APL : 0) + off) = w;
      }
    }
    // ---- phase B: y += h W2[:, chunk]^T -----------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int kk = 0; kk < SM_NB; ++kk) {
      if (kk + 1 < SM_NB) dma_wait<PWB>();
      else if (!last) dma_wait<PWA>();               // the next chunk's first W1 slab may still travel
      else dma_wait<0>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                  // (kk == 0: also orders the hidden planes of every wave before the first read)
      asm volatile("" ::: "memory");
      if (kk + 2 < SM_NB) issue(c, SM_NA + kk + 2, lane);
      else if (!last) issue(c + 1, kk + 2 - SM_NB, lane);
      const char* pw = smem + SM_PLANES + ((SM_NA + kk) % 3) * SM_SLOT;
      const char* pah = pa + (kk >> 1) * SM_APL;
      const uint4 ah = *reinterpret_cast<const uint4*>(pah + sm_off(rt * 32 + fr, (kk & 1) * 2 + fh));
      const uint4 al = *reinterpret_cast<const uint4*>(pah + 4 * SM_APL + sm_off(rt * 32 + fr, (kk & 1) * 2 + fh));
#pragma unroll
      for (int j = 0; j < D / 64; ++j) {
        const int wr = ch * (D / 2) + j * 32 + fr;
        const uint4 wh = *reinterpret_cast<const uint4*>(pw + sm_woff(wr, fh));
        const uint4 wl = *reinterpret_cast<const uint4*>(pw + D * 32 + sm_woff(wr, fh));
        yacc[j] = Half16<f16_t>::mfma32(ah, wh, yacc[j]);
        yacc[j] = Half16<f16_t>::mfma32(al, wh, yacc[j]);
        yacc[j] = Half16<f16_t>::mfma32(ah, wl, yacc[j]);
      }
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                      // every wave is done with the planes and the ring: the y tile may overwrite them
  asm volatile("" ::: "memory");
  int lane1 = lane0;                                 // (laundered again: the store addresses are not kept alive from the row burst on)
  asm volatile("" : "+v"(lane1));
  const int fr = lane1 & 31, fh = lane1 >> 5;
  // ---- epilogue: + bias -> LDS row-major, then a wave per row: residual (the fp32 rows, read again), LayerNorm, store ---------------------
  float4 xs[16];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const long row = row0 + wave * 16 + rr;
    const long rc = row < a.rows ? row : a.rows - 1;
    xs[rr] = *reinterpret_cast<const float4*>(a.x + (size_t)rc * D + lane1 * 4);
  }
#pragma unroll
  for (int j = 0; j < D / 64; ++j) {
    const int col = ch * (D / 2) + j * 32 + fr;
    const float bv = a.b2[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) yt[(rt * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh) * SM_YLD + col] = yacc[j][r] + bv;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                      // a row's columns come from two waves (ch 0 / 1); its reader is a third
  asm volatile("" ::: "memory");
  const float4 gm = reinterpret_cast<const float4*>(a.gamma)[lane1];
  const float4 bt = reinterpret_cast<const float4*>(a.beta)[lane1];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const float4 y = *reinterpret_cast<const float4*>(&yt[(wave * 16 + rr) * SM_YLD + lane1 * 4]);
    xs[rr].x += y.x; xs[rr].y += y.y; xs[rr].z += y.z; xs[rr].w += y.w;
  }
  float mu[16], rs[16];
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) mu[rr] = wave_sum_dpp((xs[rr].x + xs[rr].y) + (xs[rr].z + xs[rr].w)) * (1.0f / D);
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    xs[rr].x -= mu[rr]; xs[rr].y -= mu[rr]; xs[rr].z -= mu[rr]; xs[rr].w -= mu[rr];
    rs[rr] = wave_sum_dpp((xs[rr].x * xs[rr].x + xs[rr].y * xs[rr].y) + (xs[rr].z * xs[rr].z + xs[rr].w * xs[rr].w));
  }
#pragma unroll
  for (int rr = 0; rr < 16; ++rr) {
    const long row = row0 + wave * 16 + rr;
    const float rstd = 1.0f / sqrtf(rs[rr] * (1.0f / D) + a.eps);
    if (row < a.rows)
      *reinterpret_cast<float4*>(a.x + (size_t)row * D + lane1 * 4) =
          make_float4(xs[rr].x * rstd * gm.x + bt.x, xs[rr].y * rstd * gm.y + bt.y, xs[rr].z * rstd * gm.z + bt.z, xs[rr].w * rstd * gm.w + bt.w);
  }
}

}  // namespace la

extern "C" int la_stream_mlp_ok(int D, int H) { return D == la::SM_D && H >= 128 && H <= 4096 && H % la::SM_HC == 0; }

extern "C" int la_stream_mlp(float* x, const void* w1_hi, const void* w1_lo, const float* b1, const void* w2_hi, const void* w2_lo,
                             const float* b2, const float* gamma, const float* beta, float eps, long rows, int D, int H, void* stream) {
  LA_CHECK_ARG(x && w1_hi && w1_lo && b1 && w2_hi && w2_lo && b2 && gamma && beta, "la_stream_mlp: null pointer");
  LA_CHECK_ARG(la_stream_mlp_ok(D, H), "la_stream_mlp: built for D = 256 and H a multiple of 128 from 128 to 4096 (got D=%d H=%d)", D, H);
  LA_CHECK_ARG(rows >= 1 && rows <= 0x7fffffffL * la::SM_ROWS, "la_stream_mlp: rows=%ld out of range", rows);
  la::SmArgs a{x, (const la::f16_t*)w1_hi, (const la::f16_t*)w1_lo, (const la::f16_t*)w2_hi, (const la::f16_t*)w2_lo, b1, b2, gamma, beta,
               eps, rows, H};
  static unsigned long long attr_mask = 0;
  la::ensure_dyn_lds(reinterpret_cast<const void*>(la::stream_mlp_kernel), la::SM_LDS, attr_mask);
  hipLaunchKernelGGL(la::stream_mlp_kernel, dim3((unsigned)((rows + la::SM_ROWS - 1) / la::SM_ROWS)), dim3(la::SM_WAVES * 64), la::SM_LDS,
                     reinterpret_cast<hipStream_t>(stream), a);
  LA_CHECK_LAUNCH("la_stream_mlp");
  return 0;
}
