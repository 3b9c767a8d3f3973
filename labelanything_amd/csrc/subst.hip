// Error-point sampling of query substitution (experiment/substitution.py:17-97 generate_points_from_errors, then
// data/transforms.py:176-191 PromptsProcessor.torch_apply_coords) without the one-hot tensors, torch.nonzero / torch.unique, the host
// set arithmetic and the per-class torch.randint launches of the reference: one streaming pass that counts the error pixels of every
// (image, class) per tile, and one wave per (image, class) that scans those counts, picks the tile of each draw by binary search and
// re-reads only that tile to find the rank-th error pixel in raster (y, x) order - torch.nonzero's order.
//
// Per pixel p = argmax over C (first maximal index, NaN wins - torch.argmax), g = ground truth with ignore_index (and any value
// outside [0, C)) read as 0.  A pixel with p != g is an error of class g with label +1 (false negative) and of class p with label -1
// (false positive).  Compiled with contraction off: the coordinate scale is evaluated as the reference's float32 tensor ops.
#include "la_common.h"
#include "../../include/la_hip.h"

#pragma clang fp contract(off)

namespace la {

constexpr int SUB_TILE = 4096;       // pixels per tile: 256 threads x 16 in la_error_count, 64 lanes x 64 in la_error_points
constexpr int SUB_CMAX = 64;         // classes per episode (LDS counters of la_error_count)
constexpr int SUB_TMAX = 4096;       // tiles per image (LDS scan of la_error_points): H * W <= 16.7 M pixels

__device__ __forceinline__ void sub_pixel(const float* __restrict__ lg, const int64_t* __restrict__ gt, int C, long HW, long i, int ignore,
                                          int& p, int& g) {
  float best = lg[i];
  p = 0;
  for (int c = 1; c < C; ++c) {
    const float v = lg[(long)c * HW + i];
    if (v > best || (v != v && best == best)) {
      best = v;
      p = c;
    }
  }
  const int64_t t = gt[i];
  g = (t == ignore || t < 0 || t >= C) ? 0 : (int)t;
}

// grid (tiles, B), 256 threads.  counts [B, C, tiles]; preds int64 [B, H*W] or null.
__global__ __launch_bounds__(256) void error_count_kernel(const float* __restrict__ logits, const int64_t* __restrict__ gt, int C, long HW,
                                                          int ignore, int T, unsigned* __restrict__ counts, int64_t* __restrict__ preds) {
  __shared__ unsigned s_cnt[4][SUB_CMAX];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tile = blockIdx.x, b = blockIdx.y;
  for (int k = tid; k < 4 * SUB_CMAX; k += 256) (&s_cnt[0][0])[k] = 0u;
  __syncthreads();
  const float* lg = logits + (long)b * C * HW;
  const int64_t* gb = gt + (long)b * HW;
  for (int k = 0; k < SUB_TILE / 256; ++k) {
    const long i = (long)tile * SUB_TILE + k * 256 + tid;
    int p = 0, g = 0;
    const bool valid = i < HW;
    if (valid) {
      sub_pixel(lg, gb, C, HW, i, ignore, p, g);
      if (preds) preds[(long)b * HW + i] = p;
    }
    const bool err = valid && p != g;
    if (__ballot(err) == 0ull) continue;               // wave-uniform
    for (int c = 0; c < C; ++c) {
      const unsigned n = (unsigned)__popcll(__ballot(err && (g == c || p == c)));
      if (lane == 0) s_cnt[wave][c] += n;               // one writer per (wave, class)
    }
  }
  __syncthreads();
  if (tid < C) counts[((long)b * C + tid) * T + tile] = s_cnt[0][tid] + s_cnt[1][tid] + s_cnt[2][tid] + s_cnt[3][tid];
}

// grid (C, B), one wave.  ranks int32 [B, C, n] or u fp32 [B, C, n]; dims int64 rows (h, w) at dims[b * dims_stride] or null (raw pixel
// coordinates); points fp32 [B, C, n, 2] = (x, y), labels fp32 [B, C, n].
__global__ __launch_bounds__(64) void error_points_kernel(const float* __restrict__ logits, const int64_t* __restrict__ gt, int C, int W,
                                                          long HW, int ignore, int T, const unsigned* __restrict__ counts, int n,
                                                          const int* __restrict__ ranks, const float* __restrict__ uni,
                                                          const int64_t* __restrict__ dims, long dims_stride, int long_side, int custom,
                                                          float* __restrict__ points, float* __restrict__ labels) {
  __shared__ unsigned s_inc[SUB_TMAX];
  const int lane = threadIdx.x;
  const int c = blockIdx.x, b = blockIdx.y;
  const unsigned* cnt = counts + ((long)b * C + c) * T;
  unsigned carry = 0;
  for (int t0 = 0; t0 < T; t0 += 64) {
    unsigned v = (t0 + lane < T) ? cnt[t0 + lane] : 0u;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned y = __shfl_up(v, o);
      if (lane >= o) v += y;
    }
    if (t0 + lane < T) s_inc[t0 + lane] = carry + v;
    carry += __shfl(v, 63);
  }
  __syncthreads();
  const unsigned total = carry;

  // torch_apply_coords on 0-d int64 tensors: every step a float32 tensor op (x / t is reciprocal(t) * x)
  float fx = 1.f, fy = 1.f;
  if (dims) {
    const int64_t oh = dims[(long)b * dims_stride], ow = dims[(long)b * dims_stride + 1];
    float nh = (float)long_side, nw = (float)long_side;
    if (custom) {
      const float sc = __fmul_rn(__fdiv_rn(1.f, (float)(oh > ow ? oh : ow)), (float)long_side);
      nh = (float)(int)__fadd_rn(__fmul_rn((float)oh, sc), 0.5f);
      nw = (float)(int)__fadd_rn(__fmul_rn((float)ow, sc), 0.5f);
    }
    fx = __fmul_rn(__fdiv_rn(1.f, (float)ow), nw);
    fy = __fmul_rn(__fdiv_rn(1.f, (float)oh), nh);
  }

  const float* lg = logits + (long)b * C * HW;
  const int64_t* gb = gt + (long)b * HW;
  for (int k = 0; k < n; ++k) {
    const long o = ((long)b * C + c) * n + k;
    if (total == 0u) {
      if (lane == 0) {
        points[2 * o] = 0.f;
        points[2 * o + 1] = 0.f;
        labels[o] = 0.f;
      }
      continue;
    }
    unsigned r;
    if (ranks) {
      const int rk = ranks[o];
      r = rk < 0 ? 0u : ((unsigned)rk >= total ? total - 1u : (unsigned)rk);
    } else {
      const double x = floor((double)uni[o] * (double)total);
      r = x < 0.0 ? 0u : (x >= (double)total ? total - 1u : (unsigned)x);
    }
    // first tile whose inclusive count exceeds r
    int lo = 0, hi = T - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_inc[mid] > r) hi = mid; else lo = mid + 1;
    }
    const unsigned rr = r - (lo ? s_inc[lo - 1] : 0u);
    // lane j keeps the error mask of the tile's j-th run of 64 pixels (raster order)
    const long base = (long)lo * SUB_TILE;
    unsigned long long mine = 0ull;
    for (int j0 = 0; j0 < 64; j0 += 8) {
      bool e[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const long i = base + (long)(j0 + q) * 64 + lane;
        int p = 0, g = 0;
        if (i < HW) sub_pixel(lg, gb, C, HW, i, ignore, p, g);
        e[q] = (i < HW) && p != g && (g == c || p == c);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const unsigned long long m = __ballot(e[q]);
        if (lane == j0 + q) mine = m;
      }
    }
    const unsigned pc = (unsigned)__popcll(mine);
    unsigned inc = pc;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned y = __shfl_up(inc, d);
      if (lane >= d) inc += y;
    }
    const unsigned exc = inc - pc;
    const bool owner = exc <= rr && rr < inc;
    if (owner) {
      unsigned long long m = mine;
      for (unsigned s = rr - exc; s > 0u; --s) m &= m - 1ull;
      const long i = base + (long)lane * 64 + (__ffsll((long long)m) - 1);
      int p = 0, g = 0;
      sub_pixel(lg, gb, C, HW, i, ignore, p, g);
      const int y = (int)(i / W), x = (int)(i - (long)y * W);
      points[2 * o] = __fmul_rn((float)x, fx);
      points[2 * o + 1] = __fmul_rn((float)y, fy);
      labels[o] = (c == 0) ? 0.f : (g == c ? 1.f : -1.f);
    }
  }
}

}  // namespace la

extern "C" int la_error_count(const float* logits, const long long* gt, int B, int C, int H, int W, int ignore_index, unsigned* counts,
                              long long* preds, void* stream) {
  LA_CHECK_ARG(logits && gt && counts && B > 0 && C > 0 && C <= la::SUB_CMAX && H > 0 && W > 0, "la_error_count: bad arguments (C <= %d)",
               la::SUB_CMAX);
  const long HW = (long)H * W;
  const long T = (HW + la::SUB_TILE - 1) / la::SUB_TILE;
  LA_CHECK_ARG(T <= la::SUB_TMAX && B <= 65535, "la_error_count: image too large (%ld tiles > %d) or B > 65535", T, la::SUB_TMAX);
  hipLaunchKernelGGL(la::error_count_kernel, dim3((unsigned)T, B), dim3(256), 0, (hipStream_t)stream, logits,
                     reinterpret_cast<const int64_t*>(gt), C, HW, ignore_index, (int)T, counts, reinterpret_cast<int64_t*>(preds));
  LA_CHECK_LAUNCH("la_error_count");
  return 0;
}

extern "C" int la_error_points(const float* logits, const long long* gt, int B, int C, int H, int W, int ignore_index, const unsigned* counts,
                               int num_points, const int* ranks, const float* u, const long long* dims, long dims_stride, int long_side,
                               int custom_preprocess, float* points, float* labels, void* stream) {
  LA_CHECK_ARG(logits && gt && counts && points && labels && (ranks || u) && B > 0 && C > 0 && C <= la::SUB_CMAX && H > 0 && W > 0 &&
                   num_points > 0 && B <= 65535 && long_side > 0,
               "la_error_points: bad arguments");
  const long HW = (long)H * W;
  const long T = (HW + la::SUB_TILE - 1) / la::SUB_TILE;
  LA_CHECK_ARG(T <= la::SUB_TMAX, "la_error_points: image too large (%ld tiles > %d)", T, la::SUB_TMAX);
  hipLaunchKernelGGL(la::error_points_kernel, dim3(C, B), dim3(64), 0, (hipStream_t)stream, logits, reinterpret_cast<const int64_t*>(gt), C, W,
                     HW, ignore_index, (int)T, counts, num_points, ranks, u, reinterpret_cast<const int64_t*>(dims), dims_stride, long_side,
                     custom_preprocess, points, labels);
  LA_CHECK_LAUNCH("la_error_points");
  return 0;
}
