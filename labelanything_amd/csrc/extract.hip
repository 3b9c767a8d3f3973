// embedding_extraction = "cross_attention" (EmbeddingTransformer.forward, prompt_encoder.py:289-298; OneWayAttentionBlock.forward,
// transformer.py:140-147; Attention.forward, common.py:105-146): n learned queries per (episode, class) pair attend over the M hw rows of
// the pair's slabs of the prompt encoder's stream, eight heads of width D / 16.
//
// The attention is FOLDED so that the stream is never projected.  With q = q_proj(E), head h and query j, the score of stream row x_l is
// q_hj . (W_k,h x_l + b_k,h) / sqrt(hd); its bias part is constant along l and cancels in the softmax.  With the folded query
// qt_hj = W_k,h^T q_hj / sqrt(hd) in R^D:  p_hjl = softmax_l(qt_hj . x_l),  pooled_hj = sum_l p_hjl x_l in R^D,  head output =
// W_v,h pooled_hj + b_v,h.  Per pair that is R = 8 n folded queries (row h n + j) and R softmax-weighted means of stream rows.
//
//   la_extract_fold    q [BC n, D / 2], W_k [D / 2, D]            -> qt [BC, R, D]
//   la_extract_pool    x [B M C, hw, D], qt [BC, R, D] or [R, D]  -> pooled [BC, R, D]      (the pass over the stream)
//   la_extract_unfold  pooled, W_v [D / 2, D], b_v                -> o [BC n, D / 2]        (what out_proj takes)
// la_extract_pool_lse is la_extract_pool that also hands out lse = max + log(sum) per folded query; the backward of all three lives in
// extract_bwd.hip.
//
// NO KEY IS MASKED.  The reference hands the module a key mask built from flag_examples, but with only a key mask Attention.forward
// builds an all-False score mask (common.py:120-124), so the rows of padded supports take part in the softmax like any others; the
// reference gives bit-identical embeddings with the real flags and with all-ones flags, and so does this.
//
// Everything is fp32: both products of la_extract_pool run on the exact-fp32 MFMA 16x16x4, the exponential is expf.  The rows of a pair
// are split over workgroups in pieces of EX_SPLIT rows - a constant, so that a pair's result does not depend on the batch it is
// computed in - and every sum has a fixed order: no atomics, two runs give the same bits.
//
// MFMA 16x16x4 f32 operand layout (lane l, q = l / 16, n = l % 16): A[row n][k q], B[k q][col n], D register r = [row 4 q + r][col n].
#include "extract_shared.h"
#include "../../include/la_hip.h"

#include <cmath>
#include <cstdint>

namespace la {

constexpr int EX_TK = 64;                 // stream rows per LDS tile: 16 per wave
constexpr int EX_SPLIT = 4 * EX_TK;       // stream rows per workgroup

// ---------------------------------------------------------------------------------------------------------------------------
// One workgroup = one piece of EX_SPLIT rows of one pair z = (b, c) and one chunk of RT row tiles (16 folded queries each).  The four
// waves stage 64 rows x D of the stream in LDS (row stride D + 4: the 16 rows a ds_read_b128 group touches fall on 16 different 16-byte
// slots); wave w owns rows 16 w .. 16 w + 15 of the tile and keeps its OWN running maximum, sum and R x D accumulator (online softmax),
// so the waves meet only at the two barriers around the staging.  Per tile and wave:
//   S^T[key][row] = x[key][:] . qt[row][:]     A = the tile's rows from LDS, B = the folded queries, held in registers for the whole loop;
//                                              D register r = S^T[key 4 q + r][row n]: a lane owns 4 keys of ONE query row,
//   m, p = exp(s - m), sum                     row statistics: 4 values in the lane, then the 4 lanes q of a column,
//   O[row][:] += p[row][key] x[key][:]         A = p exactly as the lane holds it (MFMA step r takes key 4 q + r from lane (q, n)),
//                                              B = x[key 4 q + r][col] from LDS.
// Rows past the end of the pair are zero in LDS and their score is -inf: p = 0, excluded from maximum and sum.  At the end the four waves
// are merged in wave order through LDS and the piece leaves (acc [RT 16][D], (max, sum) [RT 16]) in the scratch buffer.
// ---------------------------------------------------------------------------------------------------------------------------
template <int D, int RT>
__global__ __launch_bounds__(256) void extract_pool_kernel(const float* __restrict__ x, const float* __restrict__ qt, long qt_zstride, int M, int C,
                                                           int hw, int R, int RP, float* __restrict__ pacc, float* __restrict__ pms) {
  constexpr int LDX = D + 4;
  constexpr int NK = D / 16;                 // 16-channel steps of the first product = 16-column tiles of the second
  constexpr int ROWS = RT * 16;
  extern __shared__ __attribute__((aligned(16))) char ex_smem[];
  float* xs = reinterpret_cast<float*>(ex_smem);
  const int z = blockIdx.z, b = z / C, c = z % C;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int r0 = blockIdx.y * ROWS;
  const int Lrows = M * hw;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4, n = lane & 15;

  // folded queries of this chunk as the B operand: row r0 + 16 rt + n, channels k0 + 4 q .. + 3
  float4 bq[RT][NK];
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int row = r0 + rt * 16 + n;
    const float* src = qt + (size_t)z * qt_zstride + (size_t)row * D + 4 * q;
#pragma unroll
    for (int k = 0; k < NK; ++k) bq[rt][k] = row < R ? *reinterpret_cast<const float4*>(src + 16 * k) : zero4;
  }
  f32x4 acc[RT][NK];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[rt][k] = f32x4{0.f, 0.f, 0.f, 0.f};
  float mrun[RT], srun[RT];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    mrun[rt] = -INFINITY;
    srun[rt] = 0.f;
  }

  for (int t = 0; t < EX_SPLIT / EX_TK; ++t) {
    const int lbase = split * EX_SPLIT + t * EX_TK;
    if (lbase >= Lrows) break;                           // (uniform over the workgroup)
    __syncthreads();
    // stage the tile: thread -> (row, 4 channels), coalesced 16-byte loads; row l of the pair lives in slab m = l / hw
    constexpr int C4 = D / 4;
#pragma unroll
    for (int i = 0; i < EX_TK * C4 / 256; ++i) {
      const int idx = i * 256 + tid;
      const int row = idx / C4, c4 = idx % C4;
      const int l = lbase + row;
      float4 v = zero4;
      if (l < Lrows) {
        const int m = l / hw, pix = l - m * hw;
        v = *reinterpret_cast<const float4*>(x + (((size_t)(b * M + m) * C + c) * hw + pix) * D + 4 * c4);
      }
      *reinterpret_cast<float4*>(xs + row * LDX + 4 * c4) = v;
    }
    __syncthreads();
    const int key0 = lbase + 16 * wv;
    if (key0 < Lrows) {                                  // (uniform over the wave; its first key is a real row, so every maximum is finite)
      f32x4 sc[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) sc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* arow = xs + (16 * wv + n) * LDX + 4 * q;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const float4 a = *reinterpret_cast<const float4*>(arow + 16 * k);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) sc[rt] = ex_mfma4(ex_comp(a, j), ex_comp(bq[rt][k], j), sc[rt]);
      }
      float p[RT][4];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        float s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = (key0 + 4 * q + r < Lrows) ? sc[rt][r] : -INFINITY;
        float mx = fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(mrun[rt], mx);
        const float scale = expf(mrun[rt] - mnew);       // 0 on the first tile (mrun = -inf)
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p[rt][r] = expf(s[r] - mnew);
          ps += p[rt][r];
        }
        ps += __shfl_xor(ps, 16, 64);
        ps += __shfl_xor(ps, 32, 64);
        srun[rt] = srun[rt] * scale + ps;
        mrun[rt] = mnew;
        // the accumulator registers of this lane are rows 4 q + r, whose scale lives in the lanes with n = 4 q + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float sr = __shfl(scale, 4 * q + r, 64);
#pragma unroll
          for (int k = 0; k < NK; ++k) acc[rt][k][r] *= sr;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* brow = xs + (16 * wv + 4 * q + r) * LDX + n;
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const float bv = brow[16 * k];
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) acc[rt][k] = ex_mfma4(p[rt][r], bv, acc[rt][k]);
        }
      }
    }
  }

  // merge the four waves in wave order: statistics first, then the accumulators one wave after the other through LDS
  __syncthreads();
  float* ob = xs;                            // [ROWS][D]
  float* st = xs + ROWS * D;                 // [4][ROWS][2]      (ROWS (D + 8) <= 64 (D + 4) floats for every D, RT built)
  if (q == 0) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      st[((wv * ROWS) + rt * 16 + n) * 2 + 0] = mrun[rt];
      st[((wv * ROWS) + rt * 16 + n) * 2 + 1] = srun[rt];
    }
  }
  __syncthreads();
  float f[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rt * 16 + 4 * q + r;
      float mg = st[row * 2];
#pragma unroll
      for (int w = 1; w < 4; ++w) mg = fmaxf(mg, st[(w * ROWS + row) * 2]);      // wave 0 always has rows: finite
      f[rt][r] = expf(st[(wv * ROWS + row) * 2] - mg);                            // a wave without rows: exp(-inf) = 0
    }
  for (int w = 0; w < 4; ++w) {
    if (wv == w) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float* o = ob + (rt * 16 + 4 * q + r) * D + 16 * k + n;
            const float v = acc[rt][k][r] * f[rt][r];
            *o = w == 0 ? v : *o + v;
          }
    }
    __syncthreads();
  }
  const size_t pbase = ((size_t)z * nsplit + split) * RP + r0;
  for (int i = tid; i < ROWS * (D / 4); i += 256) {
    const int row = i / (D / 4), c4 = i % (D / 4);
    *reinterpret_cast<float4*>(pacc + (pbase + row) * D + 4 * c4) = *reinterpret_cast<const float4*>(ob + row * D + 4 * c4);
  }
  if (tid < ROWS) {
    float mg = st[tid * 2];
#pragma unroll
    for (int w = 1; w < 4; ++w) mg = fmaxf(mg, st[(w * ROWS + tid) * 2]);
    float sg = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) sg += st[(w * ROWS + tid) * 2 + 1] * expf(st[(w * ROWS + tid) * 2] - mg);
    pms[(pbase + tid) * 2 + 0] = mg;
    pms[(pbase + tid) * 2 + 1] = sg;
  }
}

// out[z][j][:] = sum_s w_s acc_s / sum_s w_s sum_s with w_s = exp(max_s - max), pieces in index order.  One workgroup per (row, pair).
// lse (la_extract_pool_lse; null otherwise): lse[z][j] = max + log(sum), what the backward rebuilds the weights from.
__global__ void extract_merge_kernel(const float* __restrict__ pacc, const float* __restrict__ pms, int nsplit, int RP, int D, int R,
                                     float* __restrict__ out, float* __restrict__ lse) {
  const int j = blockIdx.x, z = blockIdx.y, d = threadIdx.x;
  const size_t base = (size_t)z * nsplit * RP + j;
  float mg = pms[base * 2];
  for (int s = 1; s < nsplit; ++s) mg = fmaxf(mg, pms[(base + (size_t)s * RP) * 2]);
  float num = 0.f, den = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const size_t o = base + (size_t)s * RP;
    const float w = expf(pms[o * 2] - mg);
    num += w * pacc[o * D + d];
    den += w * pms[o * 2 + 1];
  }
  out[((size_t)z * R + j) * D + d] = num / den;
  if (lse != nullptr && d == 0) lse[(size_t)z * R + j] = mg + logf(den);
}

// qt[z][h n + j][f] = (sum_e q[z n + j][h hd + e] W_k[h hd + e][f]) / sqrt(hd): e in index order, one thread per output channel
__global__ void extract_fold_kernel(const float* __restrict__ qin, const float* __restrict__ Wk, int n, int D, float scale, float* __restrict__ qt) {
  const int row = blockIdx.x, z = blockIdx.y, f = threadIdx.x;
  const int hd = D / 2 / EX_HEADS, h = row / n, j = row % n;
  const float* qr = qin + ((size_t)z * n + j) * (D / 2) + h * hd;
  const float* wr = Wk + (size_t)h * hd * D + f;
  float s = 0.f;
  for (int e = 0; e < hd; ++e) s = fmaf(qr[e], wr[(size_t)e * D], s);
  qt[((size_t)z * EX_HEADS * n + row) * D + f] = s * scale;
}

// o[z n + j][i] = b_v[i] + sum_f W_v[i][f] pooled[z][h n + j][f] with h = i / hd: one wave per output, lanes stride the channels
__global__ __launch_bounds__(256) void extract_unfold_kernel(const float* __restrict__ pooled, const float* __restrict__ Wv, const float* __restrict__ bv,
                                                             int n, int D, float* __restrict__ o) {
  const int j = blockIdx.x, z = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int di = D / 2, hd = di / EX_HEADS;
  for (int i = blockIdx.z * 4 + wv; i < di; i += 4 * gridDim.z) {
    const int h = i / hd;
    const float* pr = pooled + ((size_t)z * EX_HEADS * n + h * n + j) * D;
    const float* wr = Wv + (size_t)i * D;
    float s = 0.f;
    for (int f = lane; f < D; f += 64) s = fmaf(wr[f], pr[f], s);
    s = wave_sum(s);
    if (lane == 0) o[((size_t)z * n + j) * di + i] = s + bv[i];
  }
}

template <int D, int RT> static void launch_pool(const float* x, const float* qt, long qzs, int BC, int M, int C, int hw, int R, int RP, int nsplit,
                                                  int nchunk, float* pacc, float* pms, hipStream_t st) {
  constexpr int LDS = EX_TK * (D + 4) * 4;
  static_assert(RT * 16 * (D + 8) <= EX_TK * (D + 4), "the merge buffers reuse the tile");
  static unsigned long long attr_mask = 0;
  ensure_dyn_lds(reinterpret_cast<const void*>(extract_pool_kernel<D, RT>), LDS, attr_mask);
  hipLaunchKernelGGL((extract_pool_kernel<D, RT>), dim3(nsplit, nchunk, BC), dim3(256), LDS, st, x, qt, qzs, M, C, hw, R, RP, pacc, pms);
}

}  // namespace la

// row tiles of 16 folded queries, in chunks of two per workgroup (one when a single tile holds them all)
static void extract_tiles(int R, int* rt, int* nchunk, int* RP) {
  const int ntile = (R + 15) / 16;
  *rt = ntile >= 2 ? 2 : 1;
  *nchunk = (ntile + *rt - 1) / *rt;
  *RP = *nchunk * *rt * 16;
}

extern "C" int la_extract_pool_plan(int M, int hw, int D, int R, int* split_rows, int* nsplit, long long* scratch_floats_per_pair) {
  LA_CHECK_ARG((R % la::EX_HEADS) == 0, "la_extract_pool_plan: R=%d must be 8 n", R);
  if (!extract_sizes_ok("la_extract_pool_plan", D, R / la::EX_HEADS)) return -1;
  LA_CHECK_ARG(M >= 1 && hw >= 1 && (long long)M * hw <= (1ll << 30), "la_extract_pool_plan: bad sizes M=%d hw=%d (M hw 1..2^30)", M, hw);
  int rt, nchunk, RP;
  extract_tiles(R, &rt, &nchunk, &RP);
  const int ns = (M * hw + la::EX_SPLIT - 1) / la::EX_SPLIT;
  if (split_rows) *split_rows = la::EX_SPLIT;
  if (nsplit) *nsplit = ns;
  if (scratch_floats_per_pair) *scratch_floats_per_pair = (long long)ns * RP * (D + 2);
  return 0;
}

// la_extract_pool and la_extract_pool_lse: the same two launches; lse == nullptr: the merge writes no statistics
static int extract_pool_impl(const char* who, const float* x, const float* qt, int qt_broadcast, int B, int M, int C, int hw, int D, int n,
                             float* scratch, float* out, float* lse, void* stream) {
  LA_CHECK_ARG(x && qt && scratch && out, "%s: null pointer", who);
  if (!extract_sizes_ok(who, D, n)) return -1;
  LA_CHECK_ARG(B >= 1 && C >= 1 && M >= 1 && hw >= 1 && (long long)B * C <= 65535 && (long long)M * hw <= (1ll << 30) &&
                   (long long)B * M * C * hw <= (1ll << 31) - 1,
               "%s: bad sizes B=%d M=%d C=%d hw=%d (B C 1..65535, M hw up to 2^30, B M C hw below 2^31)", who, B, M, C, hw);
  LA_CHECK_ARG(ex_al16(x) && ex_al16(qt) && ex_al16(scratch), "%s: 16-byte aligned x / qt / scratch", who);
  const int R = la::EX_HEADS * n, BC = B * C;
  int rt, nchunk, RP;
  extract_tiles(R, &rt, &nchunk, &RP);
  const int nsplit = (M * hw + la::EX_SPLIT - 1) / la::EX_SPLIT;
  float* pacc = scratch;                                           // [BC][nsplit][RP][D]
  float* pms = scratch + (size_t)BC * nsplit * RP * D;             // [BC][nsplit][RP][2]
  const long qzs = qt_broadcast ? 0 : (long)R * D;
  hipStream_t st = (hipStream_t)stream;
#define LA_EX_LAUNCH(DD)                                                                                        \
  do {                                                                                                          \
    if (rt == 2)                                                                                                \
      la::launch_pool<DD, 2>(x, qt, qzs, BC, M, C, hw, R, RP, nsplit, nchunk, pacc, pms, st);                   \
    else                                                                                                        \
      la::launch_pool<DD, 1>(x, qt, qzs, BC, M, C, hw, R, RP, nsplit, nchunk, pacc, pms, st);                   \
  } while (0)
  if (D == 64)
    LA_EX_LAUNCH(64);
  else if (D == 128)
    LA_EX_LAUNCH(128);
  else
    LA_EX_LAUNCH(256);
#undef LA_EX_LAUNCH
  LA_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(la::extract_merge_kernel, dim3(R, BC), dim3(D), 0, st, pacc, pms, nsplit, RP, D, R, out, lse);
  LA_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int la_extract_pool(const float* x, const float* qt, int qt_broadcast, int B, int M, int C, int hw, int D, int n, float* scratch,
                               float* out, void* stream) {
  return extract_pool_impl("la_extract_pool", x, qt, qt_broadcast, B, M, C, hw, D, n, scratch, out, nullptr, stream);
}

extern "C" int la_extract_pool_lse(const float* x, const float* qt, int qt_broadcast, int B, int M, int C, int hw, int D, int n, float* scratch,
                                   float* out, float* lse, void* stream) {
  LA_CHECK_ARG(lse != nullptr, "la_extract_pool_lse: null pointer");
  return extract_pool_impl("la_extract_pool_lse", x, qt, qt_broadcast, B, M, C, hw, D, n, scratch, out, lse, stream);
}

extern "C" int la_extract_fold(const float* q, const float* Wk, int BC, int n, int D, float* qt, void* stream) {
  LA_CHECK_ARG(q && Wk && qt, "la_extract_fold: null pointer");
  if (!extract_sizes_ok("la_extract_fold", D, n)) return -1;
  LA_CHECK_ARG(BC >= 1 && BC <= 65535, "la_extract_fold: BC=%d must be 1..65535", BC);
  const float scale = 1.0f / sqrtf((float)(D / 2 / la::EX_HEADS));
  hipLaunchKernelGGL(la::extract_fold_kernel, dim3(la::EX_HEADS * n, BC), dim3(D), 0, (hipStream_t)stream, q, Wk, n, D, scale, qt);
  LA_CHECK_LAUNCH("la_extract_fold");
  return 0;
}

extern "C" int la_extract_unfold(const float* pooled, const float* Wv, const float* bv, int BC, int n, int D, float* o, void* stream) {
  LA_CHECK_ARG(pooled && Wv && bv && o, "la_extract_unfold: null pointer");
  if (!extract_sizes_ok("la_extract_unfold", D, n)) return -1;
  LA_CHECK_ARG(BC >= 1 && BC <= 65535, "la_extract_unfold: BC=%d must be 1..65535", BC);
  hipLaunchKernelGGL(la::extract_unfold_kernel, dim3(n, BC, 4), dim3(256), 0, (hipStream_t)stream, pooled, Wv, bv, n, D, o);
  LA_CHECK_LAUNCH("la_extract_unfold");
  return 0;
}
