// The two-level classification head (classification_levels = 2, mask_decoder.py:204,345-346,358-362).
//
//   la_classify_wide / _bwd    coarse level: seg[b, c, pix] = tok[b, c, :] . img[b, pix, :] over the full transformer width D
//   la_level_reduce / _bwd     level_reducer = Conv2d(2, 1, 3x3, padding "same") over [fine logits, x4 bilinear enlargement of the coarse
//                              logits]; the enlargement is evaluated per tile in LDS and never reaches memory
//
// Everything is fp32 multiply-add in a fixed order per output (the coarse logits are of order 30).  The only atomics are the sums that
// the headers call ACCUMULATED (dtok, dw, dbias).
#include "la_common.h"
#include "../../include/la_hip.h"

namespace la {

// ---------------------------------------------------------------------------------------------------------------------------
// coarse classify: one pixel per lane, the image row is walked 16 channels at a time and held against up to 8 tokens (the token
// addresses are wave-uniform: scalar loads).  More than 8 classes re-read the row (L2) once per group of 8.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void classify_wide_kernel(const float* __restrict__ tok, const float* __restrict__ img, int Npix, int C, int D,
                                                           float* __restrict__ seg) {
  const int b = blockIdx.y;
  const int pix = blockIdx.x * 64 + threadIdx.x;
  const bool live = pix < Npix;
  const int pc = live ? pix : Npix - 1;
  const float4* row = reinterpret_cast<const float4*>(img + ((size_t)b * Npix + pc) * D);
  for (int c0 = 0; c0 < C; c0 += 8) {
    const int nc = min(8, C - c0);
    const float* tk = tok + ((size_t)b * C + c0) * D;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int d0 = 0; d0 < D; d0 += 16) {
      float f[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 t = row[(d0 >> 2) + q];
        f[4 * q] = t.x; f[4 * q + 1] = t.y; f[4 * q + 2] = t.z; f[4 * q + 3] = t.w;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < nc) {
          const float* t = tk + (size_t)j * D + d0;
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[j] = fmaf(f[e], t[e], acc[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nc && live) seg[((size_t)b * C + c0 + j) * Npix + pix] = acc[j];
  }
}

// dimg[b, pix, d] = sum_c dseg[b, c, pix] tok[b, c, d] (written), dtok[b, c, d] += sum_pix dseg[b, c, pix] img[b, pix, d].  One workgroup per
// (image, 64 pixels): its dseg columns sit in LDS, a thread owns channels d = tid, tid + 256, ... and folds the 64 pixels in index order;
// one atomic per (workgroup, c, d).
__global__ __launch_bounds__(256) void classify_wide_bwd_kernel(const float* __restrict__ dseg, const float* __restrict__ tok,
                                                                const float* __restrict__ img, int Npix, int C, int D, float* __restrict__ dimg,
                                                                float* __restrict__ dtok) {
  __shared__ float sg[32 * 64];
  const int b = blockIdx.y;
  const int p0 = blockIdx.x * 64;
  const int np = min(64, Npix - p0);
  for (int i = threadIdx.x; i < C * 64; i += 256) {
    const int c = i >> 6, p = i & 63;
    sg[i] = p < np ? dseg[((size_t)b * C + c) * Npix + p0 + p] : 0.f;
  }
  __syncthreads();
  for (int d = threadIdx.x; d < D; d += 256) {
    for (int c0 = 0; c0 < C; c0 += 8) {
      const int nc = min(8, C - c0);
      float tk[8], acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        tk[j] = j < nc ? tok[((size_t)b * C + c0 + j) * D + d] : 0.f;
        acc[j] = 0.f;
      }
      for (int p = 0; p < np; ++p) {
        const size_t at = ((size_t)b * Npix + p0 + p) * D + d;
        const float x = img[at];
        float s = c0 ? dimg[at] : 0.f;          // (this thread's own earlier store)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (j < nc) {
            const float g = sg[(c0 + j) * 64 + p];
            s = fmaf(g, tk[j], s);
            acc[j] = fmaf(g, x, acc[j]);
          }
        }
        dimg[at] = s;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (j < nc) atomicAdd(&dtok[((size_t)b * C + c0 + j) * D + d], acc[j]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The head.  A workgroup owns a 32 x 32 tile of one (b, c) plane at the fine resolution = 8 x 8 coarse pixels.
//
// x4 bilinear enlargement, align_corners = False: fine index y = 4 q + p reads the coarse pair (lo, lo + 1) with lo = q - 1 for p < 2 and q
// otherwise; the weight of lo + 1 is 5/8, 7/8, 1/8, 3/8 for p = 0 .. 3.  Rule 1 (source indices clamp to the plane): where lo < 0 or
// lo + 1 > n - 1 the surviving neighbour takes the whole weight - what clamping the index gives, without the rounding of 3/8 v + 5/8 v.
// Rule 2 (zero padding of the 3 x 3 at the fine resolution): a tap outside the 4 gh x 4 gw plane contributes zero for BOTH levels: the
// staged tiles hold zeros there, also for the enlarged level.  Nothing is ever read outside the workgroup's own plane.
//
// A thread owns column cx of four consecutive tile rows, so each half-wave (the lane group of a ds_read_b32) reads 32 consecutive words
// of one LDS row: conflict-free whatever the row stride.  Rows are 40 words apart (16-byte aligned rows).
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int LR_T = 32;                 // fine tile side
constexpr int LR_S = 40;                 // LDS row stride (words)
constexpr int LR_C = LR_T / 4 + 2;       // coarse tile side with its halo

__device__ __forceinline__ void lr_taps(int y, int n, int& lo, float& wlo, float& whi) {
  const int q = y >> 2, p = y & 3;
  lo = p < 2 ? q - 1 : q;
  whi = p == 0 ? 0.625f : p == 1 ? 0.875f : p == 2 ? 0.125f : 0.375f;
  wlo = 1.f - whi;
  if (lo < 0) { wlo = 0.f; whi = 1.f; }
  else if (lo + 1 > n - 1) { wlo = 1.f; whi = 0.f; }
}

// weight with which coarse index Y enters fine index y (0 <= y < 4 n)
__device__ __forceinline__ float lr_weight(int y, int n, int Y) {
  int lo;
  float wlo, whi;
  lr_taps(y, n, lo, wlo, whi);
  return (lo == Y ? wlo : 0.f) + (lo + 1 == Y ? whi : 0.f);
}

struct LrTile {
  int y0, x0, cy0, cx0;
  long plane;
};
__device__ __forceinline__ LrTile lr_tile(long t, int nty, int ntx) {
  LrTile r;
  const int tx = (int)(t % ntx);
  t /= ntx;
  const int ty = (int)(t % nty);
  r.plane = t / nty;
  r.y0 = ty * LR_T; r.x0 = tx * LR_T;
  r.cy0 = ty * (LR_T / 4) - 1; r.cx0 = tx * (LR_T / 4) - 1;
  return r;
}

// s0: the fine tile with a one-pixel halo (34 x 34), s1: the coarse tile with its halo (10 x 10, indices clamped to the plane), both of
// plane `tl.plane` only; zeros outside the fine plane.
__device__ __forceinline__ void lr_stage(const LrTile& tl, const float* __restrict__ p0, const float* __restrict__ p1, int gh, int gw, float* s0,
                                         float* s1) {
  const int H = 4 * gh, W = 4 * gw;
  if (threadIdx.x < LR_C * LR_C) {
    const int k = threadIdx.x / LR_C, l = threadIdx.x % LR_C;
    const int cy = min(max(tl.cy0 + k, 0), gh - 1), cx = min(max(tl.cx0 + l, 0), gw - 1);
    s1[threadIdx.x] = p1[(size_t)cy * gw + cx];
  }
  for (int i = threadIdx.x; i < (LR_T + 2) * (LR_T + 2); i += 256) {
    const int r = i / (LR_T + 2), c = i % (LR_T + 2);
    const int y = tl.y0 - 1 + r, x = tl.x0 - 1 + c;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    s0[r * LR_S + c] = in ? p0[(size_t)y * W + x] : 0.f;
  }
}

// su: the enlarged coarse level on the same 34 x 34 window, zero outside the fine plane (needs s1, i.e. a barrier after lr_stage)
__device__ __forceinline__ void lr_enlarge(const LrTile& tl, int gh, int gw, const float* s1, float* su) {
  const int H = 4 * gh, W = 4 * gw;
  for (int i = threadIdx.x; i < (LR_T + 2) * (LR_T + 2); i += 256) {
    const int r = i / (LR_T + 2), c = i % (LR_T + 2);
    const int y = tl.y0 - 1 + r, x = tl.x0 - 1 + c;
    float v = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      int ly, lx;
      float ay, by, ax, bx;
      lr_taps(y, gh, ly, ay, by);
      lr_taps(x, gw, lx, ax, bx);
      const int ya = max(ly, 0) - tl.cy0, yb = min(ly + 1, gh - 1) - tl.cy0;
      const int xa = max(lx, 0) - tl.cx0, xb = min(lx + 1, gw - 1) - tl.cx0;
      v = (by * bx) * s1[yb * LR_C + xb];
      v = fmaf(by * ax, s1[yb * LR_C + xa], v);
      v = fmaf(ay * bx, s1[ya * LR_C + xb], v);
      v = fmaf(ay * ax, s1[ya * LR_C + xa], v);
    }
    su[r * LR_S + c] = v;
  }
}

// Per output: bias, then the nine fine taps in (ky, kx) order, then the nine taps of the enlarged level - one fmaf each.
__global__ __launch_bounds__(256) void level_reduce_kernel(const float* __restrict__ cls0, const float* __restrict__ cls1,
                                                           const float* __restrict__ w, const float* __restrict__ bias, int gh, int gw, int nty,
                                                           int ntx, float* __restrict__ seg) {
  __shared__ float s0[(LR_T + 2) * LR_S], su[(LR_T + 2) * LR_S], s1[LR_C * LR_C], sw[19];
  const int H = 4 * gh, W = 4 * gw;
  const LrTile tl = lr_tile(blockIdx.x, nty, ntx);
  if (threadIdx.x < 18) sw[threadIdx.x] = w[threadIdx.x];
  if (threadIdx.x == 18) sw[18] = bias[0];
  lr_stage(tl, cls0 + (size_t)tl.plane * H * W, cls1 + (size_t)tl.plane * gh * gw, gh, gw, s0, s1);
  __syncthreads();
  lr_enlarge(tl, gh, gw, s1, su);
  __syncthreads();
  const int cx = threadIdx.x & 31, rg = threadIdx.x >> 5;
  const int x = tl.x0 + cx;
  if (x >= W) return;
  float* out = seg + (size_t)tl.plane * H * W;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = rg * 4 + k;
    const int y = tl.y0 + r;
    if (y >= H) break;
    float acc = sw[18];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) acc = fmaf(sw[ky * 3 + kx], s0[(r + ky) * LR_S + cx + kx], acc);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) acc = fmaf(sw[9 + ky * 3 + kx], su[(r + ky) * LR_S + cx + kx], acc);
    out[(size_t)y * W + x] = acc;
  }
}

// Adjoint.  One round of resident workgroups walks the tiles with a grid stride; each keeps their share of dw / dbias in registers: 19 atomics per workgroup.
//   sd   dseg on the tile with a 3-pixel halo (38 x 38), zero outside the plane
//   dcls0[y, x] = sum_k w[0][ky][kx] dseg[y - ky + 1, x - kx + 1]                                (written)
//   sg   the same with w[1] = d / d(enlarged level) on the tile with a 2-pixel halo (36 x 36), zero outside the plane (rule 2)
//   dcls1[Y, X] = sum over the <= 8 x 8 fine pixels that read (Y, X) of weight_y weight_x sg   (written: along x into sx, then along y)
//   dw[l][ky][kx] += sum dseg[y, x] level_l[y + ky - 1, x + kx - 1], dbias += sum dseg         (accumulated)
__global__ __launch_bounds__(256) void level_reduce_bwd_kernel(const float* __restrict__ dseg, const float* __restrict__ cls0,
                                                               const float* __restrict__ cls1, const float* __restrict__ w, int gh, int gw, int nty,
                                                               int ntx, long ntiles, float* __restrict__ dcls0, float* __restrict__ dcls1,
                                                               float* __restrict__ dw, float* __restrict__ dbias) {
  constexpr int SD = LR_T + 6, SG = LR_T + 4, NC = LR_T / 4;
  __shared__ float sd[SD * LR_S], sg[SG * LR_S], s0[(LR_T + 2) * LR_S], su[(LR_T + 2) * LR_S], s1[LR_C * LR_C], sx[SG * NC], sw[18], red[4 * 19];
  const int H = 4 * gh, W = 4 * gw;
  if (threadIdx.x < 18) sw[threadIdx.x] = w[threadIdx.x];
  float acc[19];
#pragma unroll
  for (int i = 0; i < 19; ++i) acc[i] = 0.f;
  const int cx = threadIdx.x & 31, rg = threadIdx.x >> 5;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const LrTile tl = lr_tile(t, nty, ntx);
    const float* dp = dseg + (size_t)tl.plane * H * W;
    __syncthreads();                                     // the previous tile's readers are done
    lr_stage(tl, cls0 + (size_t)tl.plane * H * W, cls1 + (size_t)tl.plane * gh * gw, gh, gw, s0, s1);
    for (int i = threadIdx.x; i < SD * SD; i += 256) {
      const int r = i / SD, c = i % SD;
      const int y = tl.y0 - 3 + r, x = tl.x0 - 3 + c;
      const bool in = y >= 0 && y < H && x >= 0 && x < W;
      sd[r * LR_S + c] = in ? dp[(size_t)y * W + x] : 0.f;
    }
    __syncthreads();
    lr_enlarge(tl, gh, gw, s1, su);
    for (int i = threadIdx.x; i < SG * SG; i += 256) {
      const int r = i / SG, c = i % SG;
      const int y = tl.y0 - 2 + r, x = tl.x0 - 2 + c;
      float v = 0.f;
      if (y >= 0 && y < H && x >= 0 && x < W) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) v = fmaf(sw[9 + ky * 3 + kx], sd[(r + 2 - ky) * LR_S + c + 2 - kx], v);
      }
      sg[r * LR_S + c] = v;
    }
    __syncthreads();
    // fine level + the weight gradients: a thread owns column cx of rows 4 rg .. 4 rg + 3
    {
      const int x = tl.x0 + cx;
      float* out = dcls0 + (size_t)tl.plane * H * W;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int r = rg * 4 + k;
        const int y = tl.y0 + r;
        if (x < W && y < H) {
          float v = 0.f;
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) v = fmaf(sw[ky * 3 + kx], sd[(r + 4 - ky) * LR_S + cx + 4 - kx], v);
          out[(size_t)y * W + x] = v;
          const float g = sd[(r + 3) * LR_S + cx + 3];
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
              acc[ky * 3 + kx] = fmaf(g, s0[(r + ky) * LR_S + cx + kx], acc[ky * 3 + kx]);
              acc[9 + ky * 3 + kx] = fmaf(g, su[(r + ky) * LR_S + cx + kx], acc[9 + ky * 3 + kx]);
            }
          acc[18] += g;
        }
      }
    }
    // coarse level, along x: sx[r][X] = sum over the fine columns that read coarse column X
    for (int i = threadIdx.x; i < SG * NC; i += 256) {
      const int r = i / NC, X = i % NC;
      const int gx = tl.cx0 + 1 + X;
      float v = 0.f;
      if (gx < gw) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int x = 4 * gx - 2 + j;
          if (x >= 0 && x < W) v = fmaf(lr_weight(x, gw, gx), sg[r * LR_S + 4 * X + j], v);
        }
      }
      sx[i] = v;
    }
    __syncthreads();
    if (threadIdx.x < NC * NC) {
      const int Y = threadIdx.x / NC, X = threadIdx.x % NC;
      const int gy = tl.cy0 + 1 + Y, gx = tl.cx0 + 1 + X;
      if (gy < gh && gx < gw) {
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int y = 4 * gy - 2 + j;
          if (y >= 0 && y < H) v = fmaf(lr_weight(y, gh, gy), sx[(4 * Y + j) * NC + X], v);
        }
        dcls1[(size_t)tl.plane * gh * gw + (size_t)gy * gw + gx] = v;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 19; ++i) {
    const float s = wave_sum_dpp(acc[i]);
    if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 19 + i] = s;
  }
  __syncthreads();
  if (threadIdx.x < 19) {
    const float s = (red[threadIdx.x] + red[19 + threadIdx.x]) + (red[38 + threadIdx.x] + red[57 + threadIdx.x]);
    atomicAdd(threadIdx.x < 18 ? dw + threadIdx.x : dbias, s);
  }
}

}  // namespace la

static bool wide_ok(const char* who, int B, int Npix, int C, int D) {
  if (B <= 0 || B > 65535 || Npix <= 0 || C <= 0) {
    la_set_error("%s: bad sizes B=%d Npix=%d C=%d (B <= 65535)", who, B, Npix, C);
    return false;
  }
  if (C > 32) {
    la_set_error("%s: C=%d classes (at most 32)", who, C);
    return false;
  }
  if (D <= 0 || D % 64 != 0 || D > 1024) {
    la_set_error("%s: width D=%d (a multiple of 64, at most 1024)", who, D);
    return false;
  }
  return true;
}

extern "C" int la_classify_wide(const float* tok, const float* img, int B, int Npix, int C, int D, float* seg, void* stream) {
  LA_CHECK_ARG(tok && img && seg, "la_classify_wide: null pointer");
  if (!wide_ok("la_classify_wide", B, Npix, C, D)) return -1;
  hipLaunchKernelGGL(la::classify_wide_kernel, dim3((Npix + 63) / 64, B), dim3(64), 0, (hipStream_t)stream, tok, img, Npix, C, D, seg);
  LA_CHECK_LAUNCH("la_classify_wide");
  return 0;
}

extern "C" int la_classify_wide_bwd(const float* dseg, const float* tok, const float* img, int B, int Npix, int C, int D, float* dimg,
                                    float* dtok, void* stream) {
  LA_CHECK_ARG(dseg && tok && img && dimg && dtok, "la_classify_wide_bwd: null pointer");
  if (!wide_ok("la_classify_wide_bwd", B, Npix, C, D)) return -1;
  hipLaunchKernelGGL(la::classify_wide_bwd_kernel, dim3((Npix + 63) / 64, B), dim3(256), 0, (hipStream_t)stream, dseg, tok, img, Npix, C, D,
                     dimg, dtok);
  LA_CHECK_LAUNCH("la_classify_wide_bwd");
  return 0;
}

static bool reduce_ok(const char* who, int B, int C, int gh, int gw, long& ntiles, int& nty, int& ntx) {
  if (B <= 0 || C <= 0 || gh <= 0 || gw <= 0 || gh > 4096 || gw > 4096) {
    la_set_error("%s: bad sizes B=%d C=%d grid %d x %d (sides 1..4096)", who, B, C, gh, gw);
    return false;
  }
  nty = (4 * gh + la::LR_T - 1) / la::LR_T;
  ntx = (4 * gw + la::LR_T - 1) / la::LR_T;
  ntiles = (long)B * C * nty * ntx;
  if (ntiles > 0x7fffffffL) {
    la_set_error("%s: %ld tiles (B=%d C=%d grid %d x %d) exceed one launch", who, ntiles, B, C, gh, gw);
    return false;
  }
  return true;
}

extern "C" int la_level_reduce(const float* cls0, const float* cls1, const float* w, const float* bias, int B, int C, int gh, int gw, float* seg,
                               void* stream) {
  LA_CHECK_ARG(cls0 && cls1 && w && bias && seg, "la_level_reduce: null pointer");
  long ntiles;
  int nty, ntx;
  if (!reduce_ok("la_level_reduce", B, C, gh, gw, ntiles, nty, ntx)) return -1;
  hipLaunchKernelGGL(la::level_reduce_kernel, dim3((unsigned)ntiles), dim3(256), 0, (hipStream_t)stream, cls0, cls1, w, bias, gh, gw, nty, ntx,
                     seg);
  LA_CHECK_LAUNCH("la_level_reduce");
  return 0;
}

extern "C" int la_level_reduce_bwd(const float* dseg, const float* cls0, const float* cls1, const float* w, int B, int C, int gh, int gw,
                                   float* dcls0, float* dcls1, float* dw, float* dbias, void* stream) {
  LA_CHECK_ARG(dseg && cls0 && cls1 && w && dcls0 && dcls1 && dw && dbias, "la_level_reduce_bwd: null pointer");
  long ntiles;
  int nty, ntx;
  if (!reduce_ok("la_level_reduce_bwd", B, C, gh, gw, ntiles, nty, ntx)) return -1;
  // one round of resident workgroups (what the occupancy query says of this kernel's registers and LDS), each striding over the tiles
  static int resident[64];
  int dev = 0;
  (void)hipGetDevice(&dev);
  int cap = dev >= 0 && dev < 64 ? resident[dev] : 0;
  if (cap == 0) {
    int ncu = 0, per_cu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, la::level_reduce_bwd_kernel, 256, 0) != hipSuccess || per_cu <= 0) per_cu = 4;
    cap = ncu * per_cu;
    if (dev >= 0 && dev < 64) resident[dev] = cap;
  }
  const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
  hipLaunchKernelGGL(la::level_reduce_bwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, dseg, cls0, cls1, w, gh, gw, nty, ntx, ntiles,
                     dcls0, dcls1, dw, dbias);
  LA_CHECK_LAUNCH("la_level_reduce_bwd");
  return 0;
}
