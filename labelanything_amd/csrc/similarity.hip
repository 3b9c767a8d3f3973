// Cosine-similarity few-shot segmenter (models/similarity.py:105-195): operand preparation, class membership bits and the fused masked
// maximum of the query x support score matrix.  The [Q, K] score matrix lives in MFMA accumulators only.
#include "la_common.h"
#include "../../include/la_hip.h"

namespace la {
namespace sim {

// ---- la_sim_prepare ------------------------------------------------------------------------------------------------------------------
// torch's upsample_bicubic2d (align_corners=False): source coordinate scale * (dst + 0.5) - 0.5 with scale = in / out in fp32, NOT clamped
// at zero, the four taps floor - 1 .. floor + 2 clamped to the border, Keys' cubic with A = -0.75.
__device__ __forceinline__ void cubic_taps(int dst, float scale, int in, int idx[4], float w[4]) {
  const float real = scale * ((float)dst + 0.5f) - 0.5f;
  const float fl = floorf(real);
  const float t = real - fl, u = 1.0f - t;
  const int i0 = (int)fl;
  const float A = -0.75f;
  w[0] = ((A * (t + 1.0f) - 5.0f * A) * (t + 1.0f) + 8.0f * A) * (t + 1.0f) - 4.0f * A;
  w[1] = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  w[2] = ((A + 2.0f) * u - (A + 3.0f)) * u * u + 1.0f;
  w[3] = ((A * (u + 1.0f) - 5.0f * A) * (u + 1.0f) + 8.0f * A) * (u + 1.0f) - 4.0f * A;
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = min(max(i0 - 1 + j, 0), in - 1);
}

// One output pixel per group of `tpp` threads (a power of two, 16 .. 256, >= D / 4), four channels per thread: the 16 taps applied
// separably (columns, then rows), the squared norm summed over the group, x / max(|x|, 1e-12) rounded once to fp16.
__global__ __launch_bounds__(256) void prepare_kernel(const float* __restrict__ x, long total, int gin, int cs, int D, int tpp,
                                                      f16_t* __restrict__ out) {
  __shared__ float part[4];
  const int tid = threadIdx.x;
  const int ppb = 256 / tpp;
  const long pix = (long)blockIdx.x * ppb + tid / tpp;
  const int d4 = tid % tpp;
  const bool active = pix < total && d4 < (D >> 2);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active) {
    const int hw = cs * cs;
    const long img = pix / hw;
    const int rem = (int)(pix - img * hw);
    const int oy = rem / cs, ox = rem - oy * cs;
    const float4* src = reinterpret_cast<const float4*>(x) + img * gin * gin * (D >> 2) + d4;
    const int ld = D >> 2;
    if (gin == cs) {
      v = src[(long)(oy * gin + ox) * ld];
    } else {
      const float scale = (float)gin / (float)cs;
      int iy[4], ix[4];
      float wy[4], wx[4];
      cubic_taps(oy, scale, gin, iy, wy);
      cubic_taps(ox, scale, gin, ix, wx);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float4* row = src + (long)iy[i] * gin * ld;
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 a = row[(long)ix[j] * ld];
          r.x += wx[j] * a.x;
          r.y += wx[j] * a.y;
          r.z += wx[j] * a.z;
          r.w += wx[j] * a.w;
        }
        v.x += wy[i] * r.x;
        v.y += wy[i] * r.y;
        v.z += wy[i] * r.z;
        v.w += wy[i] * r.w;
      }
    }
  }
  float ss = v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
  ss = wave_sum(ss, tpp < 64 ? tpp : 64);
  if (tpp > 64) {                       // block-uniform: a pixel's group spans tpp / 64 whole waves
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    const int first = (tid / tpp) * (tpp >> 6);
    ss = 0.f;
    for (int i = 0; i < (tpp >> 6); ++i) ss += part[first + i];
  }
  if (active) {
    const float inv = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
    store4v<f16_t>(out + pix * D + 4 * d4, v.x * inv, v.y * inv, v.z * inv, v.w * inv);
  }
}

// ---- la_sim_class_bits ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void class_bits_kernel(const float* __restrict__ masks, int P, int N, int Hm, int Wm, int cs,
                                                         uint32_t* __restrict__ bits) {
  const long total = (long)P * cs * cs;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int x = (int)(i % cs), y = (int)((i / cs) % cs);
    const long p = i / ((long)cs * cs);
    const long at = (long)nearest_src(y, Hm, cs) * Wm + nearest_src(x, Wm, cs);
    const float* m = masks + p * N * Hm * Wm + at;
    uint32_t b = 0;
    for (int n = 1; n < N; ++n)
      if (m[(long)n * Hm * Wm] != 0.0f) b |= 1u << n;
    bits[i] = b ? b : 1u;
  }
}

// ---- la_sim_max ----------------------------------------------------------------------------------------------------------------------
// A workgroup (4 waves) owns TQ = 128 query columns and walks its share of the keys in blocks of TK = 128 rows.  Scores are computed
// keys x queries (keys = A rows, queries = B columns) on the 32x32x16 fp16 MFMA, so a lane holds ONE query column and 16 key rows of a
// tile in its accumulator registers: the running maximum over keys is register-local.  Wave (wk, wq) owns key rows wk * 64 .. + 64 and
// query columns wq * 64 .. + 64 of the block tile (2 x 2 MFMA tiles).  Both operands travel global -> registers -> LDS in 64-deep chunks,
// two LDS buffers, one barrier per chunk.
//
// Class handling: per 32-key MFMA tile the OR and the AND of the keys' class words are wave-uniform.  A class absent from the tile
// (OR bit clear) costs nothing; a class that owns the whole tile (AND bit set) takes the plain maximum of the 16 registers; only a tile
// that a class boundary crosses pays a select per score.  NB = 8 classes are carried per pass; more classes run further passes.
constexpr int TK = 128, TQ = 128, BK = 64, NB = 8;
constexpr int TILE_BYTES = TK * BK * 2;                               // 16 KiB: one operand's chunk
constexpr int LDS_BITS = 4 * TILE_BYTES;                              // class words of the key block, two parities
constexpr int LDS_ANY = LDS_BITS + 2 * TK * 4, LDS_ALL = LDS_ANY + 2 * 4 * 4;
constexpr int LDS_TOTAL = LDS_ALL + 2 * 4 * 4;

__device__ __forceinline__ float max16(const f32x16& a) {
  const float m0 = __builtin_fmaxf(__builtin_fmaxf(a[0], a[1]), a[2]);
  const float m1 = __builtin_fmaxf(__builtin_fmaxf(a[3], a[4]), a[5]);
  const float m2 = __builtin_fmaxf(__builtin_fmaxf(a[6], a[7]), a[8]);
  const float m3 = __builtin_fmaxf(__builtin_fmaxf(a[9], a[10]), a[11]);
  const float m4 = __builtin_fmaxf(__builtin_fmaxf(a[12], a[13]), a[14]);
  return __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(m0, m1), __builtin_fmaxf(m2, m3)), __builtin_fmaxf(m4, a[15]));
}

__global__ __launch_bounds__(256) void sim_max_kernel(const f16_t* __restrict__ q16, const f16_t* __restrict__ k16,
                                                      const uint32_t* __restrict__ bits, int Q, int K, int D, int N, int nqt, int ksplit,
                                                      int kb_per, int nkb, int npass, float* __restrict__ dst, long split_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wk = wave & 1, wq = wave >> 1, r = lane & 31, h = lane >> 5;
  int bid = blockIdx.x;
  const int qt = bid % nqt;
  bid /= nqt;
  const int split = bid % ksplit;
  bid /= ksplit;
  const int pass = bid % npass, b = bid / npass;
  const int c0 = pass * NB, q0 = qt * TQ;
  const int kb_begin = split * kb_per, kb_end = min(nkb, kb_begin + kb_per);
  const int nch = D / BK;
  const float ninf = -__builtin_inff();

  const f16_t* qb = q16 + (long)b * Q * D;
  const f16_t* kbase = k16 + (long)b * K * D;
  const uint32_t* bitsb = bits + (long)b * K;
  uint32_t* sbits = reinterpret_cast<uint32_t*>(smem + LDS_BITS);
  uint32_t* sany = reinterpret_cast<uint32_t*>(smem + LDS_ANY);
  uint32_t* sall = reinterpret_cast<uint32_t*>(smem + LDS_ALL);

  // staging: thread -> 16-byte piece c of rows (tid >> 3) + 32 i of either operand's [128, 64] chunk (rows past the end re-read the last row:
  // padded keys carry a zero class word, padded queries are not stored)
  const int c = tid & 7, srow = tid >> 3;
  const f16_t* qsrc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) qsrc[i] = qb + (long)min(q0 + srow + 32 * i, Q - 1) * D + c * 8;
  uint4 stq0, stq1, stq2, stq3, stk0, stk1, stk2, stk3;
  uint32_t stb = 0;
  const int koff = c * 8;
  unsigned char* const sm = smem;

#define SIM_GLOAD(kb_, dc_)                                                                                           \
  do {                                                                                                                \
    const int k0_ = (kb_) * TK, d0_ = (dc_) * BK;                                                                     \
    stq0 = *reinterpret_cast<const uint4*>(qsrc[0] + d0_);                                                            \
    stq1 = *reinterpret_cast<const uint4*>(qsrc[1] + d0_);                                                            \
    stq2 = *reinterpret_cast<const uint4*>(qsrc[2] + d0_);                                                            \
    stq3 = *reinterpret_cast<const uint4*>(qsrc[3] + d0_);                                                            \
    stk0 = *reinterpret_cast<const uint4*>(kbase + (long)min(k0_ + srow, K - 1) * D + d0_ + koff);                    \
    stk1 = *reinterpret_cast<const uint4*>(kbase + (long)min(k0_ + srow + 32, K - 1) * D + d0_ + koff);               \
    stk2 = *reinterpret_cast<const uint4*>(kbase + (long)min(k0_ + srow + 64, K - 1) * D + d0_ + koff);               \
    stk3 = *reinterpret_cast<const uint4*>(kbase + (long)min(k0_ + srow + 96, K - 1) * D + d0_ + koff);               \
    if ((dc_) == 0 && tid < TK) stb = (k0_ + tid < K) ? bitsb[k0_ + tid] : 0u;                                        \
  } while (0)
  // (the class words: waves 0 and 1 whole, one key per lane, a 32-key MFMA tile per half wave)
#define SIM_LWRITE(buf_, kb_, dc_)                                                                                    \
  do {                                                                                                                \
    unsigned char* kt_ = sm + (buf_) * 2 * TILE_BYTES;                                                                \
    unsigned char* qt_ = kt_ + TILE_BYTES;                                                                            \
    *reinterpret_cast<uint4*>(kt_ + swz_off(srow, c)) = stk0;                                                         \
    *reinterpret_cast<uint4*>(kt_ + swz_off(srow + 32, c)) = stk1;                                                    \
    *reinterpret_cast<uint4*>(kt_ + swz_off(srow + 64, c)) = stk2;                                                    \
    *reinterpret_cast<uint4*>(kt_ + swz_off(srow + 96, c)) = stk3;                                                    \
    *reinterpret_cast<uint4*>(qt_ + swz_off(srow, c)) = stq0;                                                         \
    *reinterpret_cast<uint4*>(qt_ + swz_off(srow + 32, c)) = stq1;                                                    \
    *reinterpret_cast<uint4*>(qt_ + swz_off(srow + 64, c)) = stq2;                                                    \
    *reinterpret_cast<uint4*>(qt_ + swz_off(srow + 96, c)) = stq3;                                                    \
    if ((dc_) == 0 && tid < TK) {                                                                                     \
      const int par_ = (kb_) & 1;                                                                                     \
      sbits[par_ * TK + tid] = stb;                                                                                   \
      uint32_t o_ = stb, a_ = stb;                                                                                    \
      for (int off_ = 16; off_ > 0; off_ >>= 1) {                                                                     \
        o_ |= (uint32_t)__shfl_xor((int)o_, off_, 64);                                                                \
        a_ &= (uint32_t)__shfl_xor((int)a_, off_, 64);                                                                \
      }                                                                                                               \
      if ((tid & 31) == 0) {                                                                                          \
        sany[par_ * 4 + (tid >> 5)] = o_;                                                                             \
        sall[par_ * 4 + (tid >> 5)] = a_;                                                                             \
      }                                                                                                               \
    }                                                                                                                 \
  } while (0)

  f32x16 acc[2][2];
  float m[NB][2];
#pragma unroll
  for (int n = 0; n < NB; ++n) m[n][0] = m[n][1] = ninf;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int total = (kb_end - kb_begin) * nch;
  if (total > 0) {
    SIM_GLOAD(kb_begin, 0);
    SIM_LWRITE(0, kb_begin, 0);
  }
  __syncthreads();
  int kb = kb_begin, dc = 0;
  for (int t = 0; t < total; ++t) {
    int nkbi = kb, ndc = dc + 1;
    if (ndc == nch) {
      ndc = 0;
      ++nkbi;
    }
    const bool more = t + 1 < total;
    if (more) SIM_GLOAD(nkbi, ndc);

    const unsigned char* kt = smem + (t & 1) * 2 * TILE_BYTES;
    const unsigned char* qtile = kt + TILE_BYTES;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      uint4 a[2], bq[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *reinterpret_cast<const uint4*>(kt + swz_off(wk * 64 + i * 32 + r, 2 * s + h));
        bq[i] = *reinterpret_cast<const uint4*>(qtile + swz_off(wq * 64 + i * 32 + r, 2 * s + h));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = Half16<f16_t>::mfma32(a[i], bq[j], acc[i][j]);
    }

    if (dc == nch - 1) {                // the key block is complete: fold its scores into the running maxima
      const int par = kb & 1;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int sub = wk * 2 + ks;
        const uint32_t any = ((uint32_t)__builtin_amdgcn_readfirstlane((int)sany[par * 4 + sub]) >> c0) & ((1u << NB) - 1u);
        const uint32_t all = (uint32_t)__builtin_amdgcn_readfirstlane((int)sall[par * 4 + sub]) >> c0;
        if (any) {
          uint32_t bt[16];                // class word of the key row of accumulator register e: row = (e & 3) + 8 (e >> 2) + 4 h
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const uint4 w = *reinterpret_cast<const uint4*>(sbits + par * TK + sub * 32 + 8 * g + 4 * h);
            bt[4 * g] = w.x >> c0;
            bt[4 * g + 1] = w.y >> c0;
            bt[4 * g + 2] = w.z >> c0;
            bt[4 * g + 3] = w.w >> c0;
          }
#pragma unroll
          for (int n = 0; n < NB; ++n) {
            if (!((any >> n) & 1u)) continue;
            if ((all >> n) & 1u) {
#pragma unroll
              for (int j = 0; j < 2; ++j) m[n][j] = __builtin_fmaxf(m[n][j], max16(acc[ks][j]));
            } else {
#pragma unroll
              for (int e = 0; e < 16; ++e) {
                const bool in = (bt[e] >> n) & 1u;
#pragma unroll
                for (int j = 0; j < 2; ++j) m[n][j] = __builtin_fmaxf(m[n][j], in ? acc[ks][j][e] : ninf);
              }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[ks][j][e] = 0.f;
      }
    }

    if (more) SIM_LWRITE((t + 1) & 1, nkbi, ndc);
    __syncthreads();
    kb = nkbi;
    dc = ndc;
  }

#undef SIM_GLOAD
#undef SIM_LWRITE
  // the two lane halves hold different key rows of the same query column; the two wk waves different key rows again
  float* red = reinterpret_cast<float*>(smem);            // [2 wk][NB][TQ]: the tiles are dead past the loop's last barrier
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float v = __builtin_fmaxf(m[n][j], __shfl_xor(m[n][j], 32, 64));
      if (h == 0) red[(wk * NB + n) * TQ + wq * 64 + j * 32 + r] = v;
    }
  __syncthreads();
  float* o = dst + (long)split * split_stride + (long)b * N * Q;
  for (int i = tid; i < NB * TQ; i += 256) {
    const int n = i / TQ, ql = i % TQ;
    if (c0 + n < N && q0 + ql < Q) o[(long)(c0 + n) * Q + q0 + ql] = __builtin_fmaxf(red[n * TQ + ql], red[(NB + n) * TQ + ql]);
  }
}

// out[i] = max over the key splits of part[s][i]: the maximum does not depend on the order, so the split does not show
__global__ __launch_bounds__(256) void sim_reduce_kernel(const float* __restrict__ part, int ksplit, long n, float* __restrict__ out) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = part[i];
    for (int s = 1; s < ksplit; ++s) v = __builtin_fmaxf(v, part[(long)s * n + i]);
    out[i] = v;
  }
}

struct Plan {
  int nqt, nkb, npass, ksplit, kb_per;
  long long work_floats;
};

static bool plan(int B, int Q, int K, int D, int N, int ncu, Plan& p) {
  if (B <= 0 || Q <= 0 || K <= 0 || N < 1 || N > 32 || D < 64 || D > 1024 || D % 64) return false;
  if (ncu <= 0) ncu = cu_count();
  p.nqt = (Q + TQ - 1) / TQ;
  p.nkb = (K + TK - 1) / TK;
  p.npass = (N + NB - 1) / NB;
  const long base = (long)B * p.nqt * p.npass;
  if (base > (1l << 30)) return false;
  // two workgroups per compute unit (64 KiB of LDS each) and two rounds of them, as long as a split keeps at least two key blocks
  long want = (4l * ncu + base - 1) / base;
  if (want > p.nkb / 2) want = p.nkb / 2;
  if (want < 1) want = 1;
  p.kb_per = (int)((p.nkb + want - 1) / want);
  p.ksplit = (p.nkb + p.kb_per - 1) / p.kb_per;
  if (base * p.ksplit > (1l << 30)) return false;
  p.work_floats = p.ksplit > 1 ? (long long)p.ksplit * B * N * Q : 0;
  return true;
}

}  // namespace sim
}  // namespace la

using namespace la;

extern "C" int la_sim_prepare(const float* x, long n, int gin, int cs, int D, void* out16, void* stream) {
  LA_CHECK_ARG(x && out16 && n > 0 && gin > 0 && cs > 0, "la_sim_prepare: bad arguments");
  LA_CHECK_ARG(D >= 64 && D <= 1024 && D % 64 == 0, "la_sim_prepare: D = %d must be a multiple of 64 in [64, 1024]", D);
  LA_CHECK_ARG(((uintptr_t)x & 15) == 0 && ((uintptr_t)out16 & 7) == 0, "la_sim_prepare: x must be 16-byte, out16 8-byte aligned");
  int tpp = 16;
  while (tpp < D / 4) tpp <<= 1;
  const long total = n * cs * cs;
  const long blocks = (total + 256 / tpp - 1) / (256 / tpp);
  LA_CHECK_ARG(blocks < (1l << 31), "la_sim_prepare: too many pixels");
  hipLaunchKernelGGL(sim::prepare_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, total, gin, cs, D, tpp,
                     reinterpret_cast<f16_t*>(out16));
  LA_CHECK_LAUNCH("la_sim_prepare");
  return 0;
}

extern "C" int la_sim_class_bits(const float* masks, int P, int N, int Hm, int Wm, int cs, unsigned* bits, void* stream) {
  LA_CHECK_ARG(masks && bits && P > 0 && Hm > 0 && Wm > 0 && cs > 0, "la_sim_class_bits: bad arguments");
  LA_CHECK_ARG(N >= 1 && N <= 32, "la_sim_class_bits: N = %d classes, at most 32 fit a class word", N);
  const long total = (long)P * cs * cs;
  const int grid = (int)((total + 255) / 256 < 32768 ? (total + 255) / 256 : 32768);
  hipLaunchKernelGGL(sim::class_bits_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, masks, P, N, Hm, Wm, cs, bits);
  LA_CHECK_LAUNCH("la_sim_class_bits");
  return 0;
}

extern "C" int la_sim_max_plan(int B, int Q, int K, int D, int N, int ncu, int* ksplit, long long* work_floats) {
  sim::Plan p;
  LA_CHECK_ARG(ksplit && work_floats, "la_sim_max_plan: bad arguments");
  LA_CHECK_ARG(sim::plan(B, Q, K, D, N, ncu, p), "la_sim_max_plan: B, Q, K > 0, 1 <= N <= 32 and D a multiple of 64 in [64, 1024] (got D = %d, N = %d)",
               D, N);
  *ksplit = p.ksplit;
  *work_floats = p.work_floats;
  return 0;
}

extern "C" int la_sim_max(const void* q16, const void* k16, const unsigned* bits, int B, int Q, int K, int D, int N, float* work,
                          long long work_floats, float* out, void* stream) {
  sim::Plan p;
  LA_CHECK_ARG(q16 && k16 && bits && out, "la_sim_max: bad arguments");
  LA_CHECK_ARG(sim::plan(B, Q, K, D, N, 0, p), "la_sim_max: B, Q, K > 0, 1 <= N <= 32 and D a multiple of 64 in [64, 1024] (got D = %d, N = %d)", D, N);
  LA_CHECK_ARG((((uintptr_t)q16 | (uintptr_t)k16) & 15) == 0, "la_sim_max: q16 and k16 must be 16-byte aligned");
  LA_CHECK_ARG(p.ksplit == 1 || (work && work_floats >= p.work_floats), "la_sim_max: the key split needs %lld floats of workspace (la_sim_max_plan)",
               p.work_floats);
  const long nout = (long)B * N * Q;
  float* dst = p.ksplit > 1 ? work : out;
  const int grid = (int)((long)B * p.nqt * p.npass * p.ksplit);
  launch_dyn<sim::sim_max_kernel>(grid, 256, sim::LDS_TOTAL, sim::LDS_TOTAL, (hipStream_t)stream, reinterpret_cast<const f16_t*>(q16),
                                  reinterpret_cast<const f16_t*>(k16), reinterpret_cast<const uint32_t*>(bits), Q, K, D, N, p.nqt, p.ksplit, p.kb_per,
                                  p.nkb, p.npass, dst, nout);
  LA_CHECK_LAUNCH("la_sim_max");
  if (p.ksplit > 1) {
    const int rgrid = (int)((nout + 255) / 256 < 32768 ? (nout + 255) / 256 : 32768);
    hipLaunchKernelGGL(sim::sim_reduce_kernel, dim3(rgrid), dim3(256), 0, (hipStream_t)stream, work, p.ksplit, nout, out);
    LA_CHECK_LAUNCH("la_sim_max (reduce)");
  }
  return 0;
}
