// Backward of embedding_extraction = "cross_attention" (extract.hip has the forward and the folding): the gradients of the three steps
// between q_proj and out_proj of a OneWayAttentionBlock (transformer.py:140-147; Attention.forward, common.py:105-146) inside
// EmbeddingTransformer.forward (prompt_encoder.py:289-313).
//
//   la_extract_pool_bwd    x, qt, out, lse, dout [BC, R, D]  -> dx [B M C, hw, D], dqt [BC, R, D] or [R, D]   (the second pass over the stream)
//   la_extract_fold_bwd    dqt, q, W_k                        -> dq [BC n, D / 2], dW_k (+=), db_k = 0
//   la_extract_unfold_bwd  do [BC n, D / 2], pooled, W_v      -> dpooled [BC, R, D], dW_v (+=), db_v (+=)
//
// With s_jl = qt_j . x_l, p_jl = exp(s_jl - lse_j), t_jl = dout_j . x_l, delta_j = dout_j . out_j and ds_jl = p_jl (t_jl - delta_j):
//   dx_l = sum_j (p_jl dout_j + ds_jl qt_j)        dqt_j = sum_l ds_jl x_l.
// Everything is fp32: the four products run on the exact-fp32 MFMA 16x16x4, the exponential is expf.  No atomics: every row of dx is written
// once with a plain store, the dqt partials of the 64-row tiles go to scratch and a second launch adds them in index order (and, in the
// broadcast form, the pairs in z order).  The tile size is a constant, so a pair alone gives the bits it gives inside a batch.
#include "extract_shared.h"
#include "../../include/la_hip.h"

#include <cmath>
#include <cstdint>

namespace la {

constexpr int XB_TK = 64;                 // stream rows per workgroup: 16 per wave
constexpr int XB_PT = 20;                 // row stride of the 16 x 16 transposition patches: conflict-free writes, 16-byte aligned rows

constexpr int xb_lds_floats(int D) { return XB_TK * (D + 4) + 2 * 16 * (D + 4) + 16 * D + 4 * 2 * 16 * XB_PT; }

// delta[z][j] = dout[z][j] . out[z][j]: one wave per row, lanes stride the channels, then the butterfly
__global__ __launch_bounds__(64) void extract_delta_kernel(const float* __restrict__ dout, const float* __restrict__ out, int D, float* __restrict__ delta) {
  const size_t row = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  float s = 0.f;
  for (int f = threadIdx.x; f < D; f += 64) s = fmaf(dout[row * D + f], out[row * D + f], s);
  s = wave_sum(s);
  if (threadIdx.x == 0) delta[row] = s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// One workgroup = one tile of XB_TK rows of one pair z = (b, c); the tile is staged once in LDS (row stride D + 4, as in the forward) and
// wave w owns its rows 16 w .. 16 w + 15, whose dx accumulator [16][D] stays in registers (D / 4 per lane) over the whole kernel.  The
// workgroup walks the row tiles of 16 folded queries; qt and dout of a row tile are staged in LDS with the same row stride.  Per row tile
// and wave:
//   S^T[key][row] = x[key] . qt[row],  T^T[key][row] = x[key] . dout[row]     A = the wave's rows, B = the staged tile; one read of x feeds
//                                                                              both; D register r = [key 4 q + r][row n],
//   p = exp(s - lse[row]),  ds = p (t - delta[row])                           in place: a lane owns 4 keys of ONE query row,
//   dqt[row][:] += ds[row][key] x[key][:]                                     A = ds as the lane holds it (step r: key 4 q + r), B = x from LDS,
//   p, ds -> LDS patch -> p^T, ds^T                                           a lane now owns 4 query rows of ONE key,
//   dx[key][:] += p[row][key] dout[row][:] + ds[row][key] qt[row][:]          A = p^T / ds^T (step r: row 4 q + r), B = the staged tiles.
// Keys past the end of the pair and rows past R have p = ds = 0.  The four waves' dqt of the row tile are added in wave order through
// LDS and leave as part[z][tile][row][:]; every wave takes part in every barrier (a wave without rows works on zeros).
// ---------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ __launch_bounds__(256) void extract_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ qt, long qt_zstride,
                                                               const float* __restrict__ dout, const float* __restrict__ lse,
                                                               const float* __restrict__ delta, int M, int C, int hw, int R, int RP,
                                                               float* __restrict__ dx, float* __restrict__ part) {
  constexpr int LDX = D + 4;
  constexpr int NK = D / 16;
  constexpr int C4 = D / 4;
  extern __shared__ __attribute__((aligned(16))) char xb_smem[];
  float* xs = reinterpret_cast<float*>(xb_smem);          // [XB_TK][LDX]   the stream tile; at the end the dx tile
  float* qs = xs + XB_TK * LDX;                           // [16][LDX]      qt of the row tile
  float* gs = qs + 16 * LDX;                              // [16][LDX]      dout of the row tile
  float* mb = gs + 16 * LDX;                              // [16][D]        dqt of the row tile, the waves added in order
  float* pt = mb + 16 * D;                                // [4][2][16][XB_PT]
  const int z = blockIdx.y, b = z / C, c = z % C;
  const int tile = blockIdx.x, ntk = gridDim.x;
  const int Lrows = M * hw;
  const int lbase = tile * XB_TK;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4, n = lane & 15;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  // stage the tile: thread -> (row, 4 channels); row l of the pair lives in slab m = l / hw
#pragma unroll
  for (int i = 0; i < XB_TK * C4 / 256; ++i) {
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

  f32x4 acc[NK];
#pragma unroll
  for (int k = 0; k < NK; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int key0 = lbase + 16 * wv;
  float* pw = pt + wv * (2 * 16 * XB_PT);
  const float* arow = xs + (16 * wv + n) * LDX + 4 * q;
  const int ntile = RP / 16;

  for (int rt = 0; rt < ntile; ++rt) {
    const int r0 = rt * 16;
    __syncthreads();                                       // the tile is staged (rt = 0); the last row tile's readers are done
#pragma unroll
    for (int i = 0; i < 16 * C4 / 256; ++i) {
      const int idx = i * 256 + tid;
      const int row = idx / C4, c4 = idx % C4;
      float4 vq = zero4, vg = zero4;
      if (r0 + row < R) {
        vq = *reinterpret_cast<const float4*>(qt + (size_t)z * qt_zstride + (size_t)(r0 + row) * D + 4 * c4);
        vg = *reinterpret_cast<const float4*>(dout + ((size_t)z * R + r0 + row) * D + 4 * c4);
      }
      *reinterpret_cast<float4*>(qs + row * LDX + 4 * c4) = vq;
      *reinterpret_cast<float4*>(gs + row * LDX + 4 * c4) = vg;
    }
    const bool row_ok = r0 + n < R;
    const float lse_n = row_ok ? lse[(size_t)z * R + r0 + n] : 0.f;
    const float del_n = row_ok ? delta[(size_t)z * R + r0 + n] : 0.f;
    __syncthreads();

    f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f}, tc = f32x4{0.f, 0.f, 0.f, 0.f};
    {
      const float* qrow = qs + n * LDX + 4 * q;
      const float* grow = gs + n * LDX + 4 * q;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const float4 a = *reinterpret_cast<const float4*>(arow + 16 * k);
        const float4 bq = *reinterpret_cast<const float4*>(qrow + 16 * k);
        const float4 bg = *reinterpret_cast<const float4*>(grow + 16 * k);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sc = ex_mfma4(ex_comp(a, j), ex_comp(bq, j), sc);
          tc = ex_mfma4(ex_comp(a, j), ex_comp(bg, j), tc);
        }
      }
    }
    float p[4], dsv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = row_ok && (key0 + 4 * q + r < Lrows);
      p[r] = ok ? expf(sc[r] - lse_n) : 0.f;
      dsv[r] = ok ? p[r] * (tc[r] - del_n) : 0.f;
    }
    // dqt of this wave's 16 keys
    f32x4 dq[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) dq[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* brow = xs + (16 * wv + 4 * q + r) * LDX + n;
#pragma unroll
      for (int k = 0; k < NK; ++k) dq[k] = ex_mfma4(dsv[r], brow[16 * k], dq[k]);
    }
    // [key][row] -> [row][key] through the wave's patch; wave 0 opens the merge buffer meanwhile
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pw[(4 * q + r) * XB_PT + n] = p[r];
      pw[16 * XB_PT + (4 * q + r) * XB_PT + n] = dsv[r];
    }
    if (wv == 0) {
#pragma unroll
      for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) mb[(4 * q + r) * D + 16 * k + n] = dq[k][r];
    }
    __syncthreads();
    const float4 pT = *reinterpret_cast<const float4*>(pw + n * XB_PT + 4 * q);
    const float4 dT = *reinterpret_cast<const float4*>(pw + 16 * XB_PT + n * XB_PT + 4 * q);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float* grow = gs + (4 * q + r) * LDX + n;
      const float* qrow = qs + (4 * q + r) * LDX + n;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        acc[k] = ex_mfma4(ex_comp(pT, r), grow[16 * k], acc[k]);
        acc[k] = ex_mfma4(ex_comp(dT, r), qrow[16 * k], acc[k]);
      }
    }
    for (int w = 1; w < 4; ++w) {
      if (wv == w) {
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
          for (int r = 0; r < 4; ++r) mb[(4 * q + r) * D + 16 * k + n] += dq[k][r];
      }
      __syncthreads();
    }
    const size_t pbase = ((size_t)z * ntk + tile) * RP + r0;
    for (int i = tid; i < 16 * C4; i += 256) {
      const int row = i / C4, c4 = i % C4;
      *reinterpret_cast<float4*>(part + (pbase + row) * D + 4 * c4) = *reinterpret_cast<const float4*>(mb + row * D + 4 * c4);
    }
  }

  // dx of the tile: through LDS (each wave over its own rows of xs, which nobody reads any more) so that the stores are whole rows
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NK; ++k)
#pragma unroll
    for (int r = 0; r < 4; ++r) xs[(16 * wv + 4 * q + r) * LDX + 16 * k + n] = acc[k][r];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < XB_TK * C4 / 256; ++i) {
    const int idx = i * 256 + tid;
    const int row = idx / C4, c4 = idx % C4;
    const int l = lbase + row;
    if (l < Lrows) {
      const int m = l / hw, pix = l - m * hw;
      *reinterpret_cast<float4*>(dx + (((size_t)(b * M + m) * C + c) * hw + pix) * D + 4 * c4) = *reinterpret_cast<const float4*>(xs + row * LDX + 4 * c4);
    }
  }
}

// dqt[z][j][:] = sum over the tiles, in index order; with nz > 1 (the broadcast form: one block of R rows for all pairs) the pairs' sums
// are then added in z order, so that the result is the fp32 sum of the per-pair form's rows.  One workgroup per (row, output pair).
__global__ void extract_dqt_sum_kernel(const float* __restrict__ part, int ntk, int RP, int D, int R, int nz, float* __restrict__ dqt) {
  const int j = blockIdx.x, zo = blockIdx.y, d = threadIdx.x;
  float total = 0.f;
  for (int zi = 0; zi < nz; ++zi) {
    const size_t base = ((size_t)(zo * nz + zi) * ntk) * RP + j;
    float s = 0.f;
    for (int t = 0; t < ntk; ++t) s += part[(base + (size_t)t * RP) * D + d];
    total = zi == 0 ? s : total + s;
  }
  dqt[((size_t)zo * R + j) * D + d] = total;
}

// dq[z n + j][h hd + e] = (sum_f dqt[z][h n + j][f] W_k[h hd + e][f]) / sqrt(hd): one wave per output, lanes stride the channels
__global__ __launch_bounds__(256) void extract_fold_bwd_dq_kernel(const float* __restrict__ dqt, const float* __restrict__ Wk, int n, int D, float scale,
                                                                  float* __restrict__ dq) {
  const int j = blockIdx.x, z = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int di = D / 2, hd = di / EX_HEADS;
  for (int i = blockIdx.z * 4 + wv; i < di; i += 4 * gridDim.z) {
    const int h = i / hd;
    const float* gr = dqt + ((size_t)z * EX_HEADS * n + h * n + j) * D;
    const float* wr = Wk + (size_t)i * D;
    float s = 0.f;
    for (int f = lane; f < D; f += 64) s = fmaf(gr[f], wr[f], s);
    s = wave_sum(s);
    if (lane == 0) dq[((size_t)z * n + j) * di + i] = s * scale;
  }
}

// dW[i][f] += scale sum_(z, j) a[z n + j][i] g[z][h n + j][f], h = i / hd, (z, j) in index order; db[i] += sum_(z, j) a[z n + j][i] where db is
// given.  One workgroup per weight row i, one thread per channel f.  Both weight gradients have this form: fold a = q, g = dqt (scale
// 1 / sqrt(hd)); unfold a = do, g = pooled (scale 1, with db_v).
__global__ void extract_wgrad_kernel(const float* __restrict__ a, const float* __restrict__ g, int BC, int n, int D, float scale, float* __restrict__ dW,
                                     float* __restrict__ db) {
  const int i = blockIdx.x, f = threadIdx.x;
  const int di = D / 2, hd = di / EX_HEADS, h = i / hd;
  float s = 0.f, sb = 0.f;
  for (int z = 0; z < BC; ++z)
    for (int j = 0; j < n; ++j) {
      const float av = a[((size_t)z * n + j) * di + i];
      s = fmaf(av, g[((size_t)z * EX_HEADS * n + h * n + j) * D + f], s);
      sb += av;
    }
  dW[(size_t)i * D + f] += s * scale;
  if (db != nullptr && f == 0) db[i] += sb;
}

__global__ void extract_zero_kernel(float* __restrict__ p, int count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) p[i] = 0.f;
}

// dpooled[z][h n + j][f] = sum_e do[z n + j][h hd + e] W_v[h hd + e][f]: e in index order, one thread per channel
__global__ void extract_unfold_bwd_dp_kernel(const float* __restrict__ dov, const float* __restrict__ Wv, int n, int D, float* __restrict__ dpooled) {
  const int row = blockIdx.x, z = blockIdx.y, f = threadIdx.x;
  const int hd = D / 2 / EX_HEADS, h = row / n, j = row % n;
  const float* gr = dov + ((size_t)z * n + j) * (D / 2) + h * hd;
  const float* wr = Wv + (size_t)h * hd * D + f;
  float s = 0.f;
  for (int e = 0; e < hd; ++e) s = fmaf(gr[e], wr[(size_t)e * D], s);
  dpooled[((size_t)z * EX_HEADS * n + row) * D + f] = s;
}

template <int D> static void launch_pool_bwd(const float* x, const float* qt, long qzs, const float* dout, const float* lse, const float* delta, int BC,
                                             int M, int C, int hw, int R, int RP, int ntk, float* dx, float* part, hipStream_t st) {
  constexpr int LDS = xb_lds_floats(D) * 4;
  static_assert(LDS <= 160 * 1024, "one workgroup per CU");
  static unsigned long long attr_mask = 0;
  ensure_dyn_lds(reinterpret_cast<const void*>(extract_pool_bwd_kernel<D>), LDS, attr_mask);
  hipLaunchKernelGGL((extract_pool_bwd_kernel<D>), dim3(ntk, BC), dim3(256), LDS, st, x, qt, qzs, dout, lse, delta, M, C, hw, R, RP, dx, part);
}

}  // namespace la

extern "C" int la_extract_pool_bwd_plan(int M, int hw, int D, int R, int* tile_rows, int* ntiles, long long* scratch_floats_per_pair) {
  LA_CHECK_ARG((R % la::EX_HEADS) == 0, "la_extract_pool_bwd_plan: R=%d must be 8 n", R);
  if (!extract_sizes_ok("la_extract_pool_bwd_plan", D, R / la::EX_HEADS)) return -1;
  LA_CHECK_ARG(M >= 1 && hw >= 1 && (long long)M * hw <= (1ll << 30), "la_extract_pool_bwd_plan: bad sizes M=%d hw=%d (M hw 1..2^30)", M, hw);
  const int RP = (R + 15) / 16 * 16;
  const int ntk = (M * hw + la::XB_TK - 1) / la::XB_TK;
  if (tile_rows) *tile_rows = la::XB_TK;
  if (ntiles) *ntiles = ntk;
  if (scratch_floats_per_pair) *scratch_floats_per_pair = (long long)ntk * RP * D + RP;      // the dqt partials and delta
  return 0;
}

extern "C" int la_extract_pool_bwd(const float* x, const float* qt, int qt_broadcast, const float* out, const float* lse, const float* dout, int B,
                                   int M, int C, int hw, int D, int n, float* scratch, float* dx, float* dqt, void* stream) {
  const char* who = "la_extract_pool_bwd";
  LA_CHECK_ARG(x && qt && out && lse && dout && scratch && dx && dqt, "%s: null pointer", who);
  if (!extract_sizes_ok(who, D, n)) return -1;
  LA_CHECK_ARG(B >= 1 && C >= 1 && M >= 1 && hw >= 1 && (long long)B * C <= 65535 && (long long)M * hw <= (1ll << 30) &&
                   (long long)B * M * C * hw <= (1ll << 31) - 1,
               "%s: bad sizes B=%d M=%d C=%d hw=%d (B C 1..65535, M hw up to 2^30, B M C hw below 2^31)", who, B, M, C, hw);
  LA_CHECK_ARG(ex_al16(x) && ex_al16(qt) && ex_al16(dout) && ex_al16(scratch) && ex_al16(dx), "%s: 16-byte aligned x / qt / dout / scratch / dx", who);
  const int R = la::EX_HEADS * n, BC = B * C;
  const int RP = (R + 15) / 16 * 16;
  const int ntk = (M * hw + la::XB_TK - 1) / la::XB_TK;
  float* part = scratch;                                           // [BC][ntk][RP][D]
  float* delta = scratch + (size_t)BC * ntk * RP * D;              // [BC][R]
  const long qzs = qt_broadcast ? 0 : (long)R * D;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(la::extract_delta_kernel, dim3(R, BC), dim3(64), 0, st, dout, out, D, delta);
  LA_CHECK_LAUNCH(who);
  if (D == 64)
    la::launch_pool_bwd<64>(x, qt, qzs, dout, lse, delta, BC, M, C, hw, R, RP, ntk, dx, part, st);
  else if (D == 128)
    la::launch_pool_bwd<128>(x, qt, qzs, dout, lse, delta, BC, M, C, hw, R, RP, ntk, dx, part, st);
  else
    la::launch_pool_bwd<256>(x, qt, qzs, dout, lse, delta, BC, M, C, hw, R, RP, ntk, dx, part, st);
  LA_CHECK_LAUNCH(who);
  if (qt_broadcast)
    hipLaunchKernelGGL(la::extract_dqt_sum_kernel, dim3(R, 1), dim3(D), 0, st, part, ntk, RP, D, R, BC, dqt);
  else
    hipLaunchKernelGGL(la::extract_dqt_sum_kernel, dim3(R, BC), dim3(D), 0, st, part, ntk, RP, D, R, 1, dqt);
  LA_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int la_extract_fold_bwd(const float* dqt, const float* q, const float* Wk, int BC, int n, int D, float* dq, float* dWk, float* dbk,
                                   void* stream) {
  const char* who = "la_extract_fold_bwd";
  LA_CHECK_ARG(dqt && q && Wk && dq && dWk && dbk, "%s: null pointer", who);
  if (!extract_sizes_ok(who, D, n)) return -1;
  LA_CHECK_ARG(BC >= 1 && BC <= 65535, "%s: BC=%d must be 1..65535", who, BC);
  const float scale = 1.0f / sqrtf((float)(D / 2 / la::EX_HEADS));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(la::extract_fold_bwd_dq_kernel, dim3(n, BC, 4), dim3(256), 0, st, dqt, Wk, n, D, scale, dq);
  LA_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(la::extract_wgrad_kernel, dim3(D / 2), dim3(D), 0, st, q, dqt, BC, n, D, scale, dWk, (float*)nullptr);
  LA_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(la::extract_zero_kernel, dim3(1), dim3(128), 0, st, dbk, D / 2);
  LA_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int la_extract_unfold_bwd(const float* dov, const float* pooled, const float* Wv, int BC, int n, int D, float* dpooled, float* dWv,
                                     float* dbv, void* stream) {
  const char* who = "la_extract_unfold_bwd";
  LA_CHECK_ARG(dov && pooled && Wv && dpooled && dWv && dbv, "%s: null pointer", who);
  if (!extract_sizes_ok(who, D, n)) return -1;
  LA_CHECK_ARG(BC >= 1 && BC <= 65535, "%s: BC=%d must be 1..65535", who, BC);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(la::extract_unfold_bwd_dp_kernel, dim3(la::EX_HEADS * n, BC), dim3(D), 0, st, dov, Wv, n, D, dpooled);
  LA_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(la::extract_wgrad_kernel, dim3(D / 2), dim3(D), 0, st, dov, pooled, BC, n, D, 1.0f, dWv, dbv);
  LA_CHECK_LAUNCH(who);
  return 0;
}
