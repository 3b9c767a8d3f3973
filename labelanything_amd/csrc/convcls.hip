// conv_classification (mask_decoder.py:257-271, 299-307): every class prototype becomes a cf x 5 x 5 kernel through two bias-free
// ConvTranspose2d(cf, cf, 3) and the logits are a per-episode 5 x 5 cross-correlation, zero padding 2, of the cf-channel feature map.
//
//   la_proto_kernels / _bwd    protos [BC, cf] -> k1 [BC, cf, 3, 3] -> K [BC, 25, cf] (tap-major, channel-minor = the NHWC feature rows)
//   la_classify_conv           seg[b, c, y, x] = sum_d sum_uv feat[b, y+u-2, x+v-2, d] K[b, c, uv, d]
//   la_classify_conv_bwd       dfeat (the correlation with flipped taps summed over the classes) and dK (a sum over the pixels)
//
// Everything is fp32: the three products over the channels run on the exact-fp32 MFMA 16x16x4, the rest is fmaf.  Every sum has a fixed
// order and there is no atomic anywhere, so two runs give the same bits.
//
// MFMA 16x16x4 f32 operand layout (lane l, q = l / 16, n = l % 16): A[row n][k q], B[k q][col n], D register r = [row 4 q + r][col n].
#include "la_common.h"
#include "../../include/la_hip.h"

#include <cstdint>

namespace la {

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float comp(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// ---------------------------------------------------------------------------------------------------------------------------
// Forward.  The correlation is taken apart as  T[p][c, uv] = feat[p][:] . K[c, uv][:]  for the pixels p of a tile WITH its halo, followed by
// seg[y][x] = sum_uv T[(y+u-2, x+v-2)][c, uv]: a GEMM with M = pixels, N = 25 x classes, K = cf that reads every feature row once per
// workgroup, and 25 additions per output.  A workgroup owns 12 x 12 outputs = 16 x 16 halo pixels = 16 MFMA row tiles (one halo row each),
// four per wave, and NT column tiles: one class (NT = 2) or two (NT = 4).  Both operands come straight from memory as float4 (a lane's
// four consecutive channels feed four MFMAs, A and B agreeing on which channel is k = q of which), so the channel dimension is walked
// 16 at a time and nothing is staged; only T goes through LDS.  Halo pixels outside the map are zero rows of A: absent taps.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int CC_T = 12;
constexpr int CC_H = CC_T + 4;

template <int NT>
__global__ __launch_bounds__(256) void classify_conv_kernel(const float* __restrict__ feat, const float* __restrict__ K, int C, int H, int W, int cf,
                                                            int ntx, int cbase, float* __restrict__ seg) {
  constexpr int CPC = NT / 2;                 // classes per workgroup
  constexpr int S = NT * 16;                  // LDS row stride; columns are rotated by hx + 12 hy so that the 64 lanes of the tap sum, which
                                              // walk tx + 12 ty, read 64 different banks (S = 64) for every tap
  __shared__ float T[CC_H * CC_H * S];
  const int b = blockIdx.z;
  const int c0 = cbase + blockIdx.y * CPC;      // (the host launches whole class groups only)
  const int nc = min(CPC, C - c0);
  const int y0 = (blockIdx.x / ntx) * CC_T, x0 = (blockIdx.x % ntx) * CC_T;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;

  const float* arow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = y0 - 2 + 4 * wv + i, x = x0 - 2 + n;
    arow[i] = (y >= 0 && y < H && x >= 0 && x < W) ? feat + (((size_t)b * H + y) * W + x) * cf + 4 * q : nullptr;
  }
  const float* brow[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = t * 16 + n;
    brow[t] = col < 25 * nc ? K + (((size_t)b * C + c0) * 25 + col) * cf + 4 * q : nullptr;
  }
  f32x4 acc[4][NT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    for (int t = 0; t < NT; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int k0 = 0; k0 < cf; k0 += 16) {
    float4 a[4], bv[NT];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = arow[i] ? *reinterpret_cast<const float4*>(arow[i] + k0) : zero;
#pragma unroll
    for (int t = 0; t < NT; ++t) bv[t] = brow[t] ? *reinterpret_cast<const float4*>(brow[t] + k0) : zero;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[i][t] = mfma4(comp(a[i], j), comp(bv[t], j), acc[i][t]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int hy = 4 * wv + i, hx = 4 * q + r;
        T[(hy * CC_H + hx) * S + ((t * 16 + n + hx + 12 * hy) & (S - 1))] = acc[i][t][r];
      }
  __syncthreads();
  for (int o = threadIdx.x; o < nc * CC_T * CC_T; o += 256) {
    const int cc = o / (CC_T * CC_T), rem = o % (CC_T * CC_T);
    const int ty = rem / CC_T, tx = rem % CC_T;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 5; ++u)
#pragma unroll
      for (int v = 0; v < 5; ++v) {
        const int hy = ty + u, hx = tx + v;
        s += T[(hy * CC_H + hx) * S + ((cc * 25 + u * 5 + v + hx + 12 * hy) & (S - 1))];
      }
    seg[(((size_t)b * C + c0 + cc) * H + y) * W + x] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// dfeat[b, y, x, d] = sum over c, uv of dseg[b, c, y-u+2, x-v+2] K[b, c, uv, d]: M = pixels, N = channels, K = 25 C (zero-filled up to
// a multiple of 4).  A workgroup owns 128 consecutive pixels of one episode and 32 channels; a wave 32 pixels.  A is gathered from dseg
// (absent where the shifted pixel falls outside the map), B are rows of K.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void classify_conv_dfeat_kernel(const float* __restrict__ dseg, const float* __restrict__ K, int C, int H, int W,
                                                                  int cf, float* __restrict__ dfeat) {
  const int b = blockIdx.z, d0 = blockIdx.y * 32;
  const int HW = H * W, KK = 25 * C;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  const int pbase = blockIdx.x * 128 + wv * 32;
  int py[2], px[2];
  bool live[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int p = pbase + i * 16 + n;
    live[i] = p < HW;
    py[i] = live[i] ? p / W : 0;
    px[i] = live[i] ? p % W : 0;
  }
  const float* dsb = dseg + (size_t)b * C * HW;
  const float* kb = K + (size_t)b * KK * cf + d0 + n;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
    for (int t = 0; t < 2; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < KK; k0 += 4) {
    const int kk = k0 + q;
    const bool kin = kk < KK;
    const int c = kk / 25, tap = kk % 25, u = tap / 5, v = tap % 5;
    float a[2], bv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int yy = py[i] - u + 2, xx = px[i] - v + 2;
      a[i] = (kin && live[i] && yy >= 0 && yy < H && xx >= 0 && xx < W) ? dsb[((size_t)c * H + yy) * W + xx] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) bv[t] = kin ? kb[(size_t)kk * cf + t * 16] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[i][t] = mfma4(a[i], bv[t], acc[i][t]);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = pbase + i * 16 + 4 * q + r;
      if (p < HW) {
#pragma unroll
        for (int t = 0; t < 2; ++t) dfeat[((size_t)b * HW + p) * cf + d0 + t * 16 + n] = acc[i][t][r];
      }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// dK[b, c, uv, d] = sum over the pixels (y, x) of feat[b, y, x, d] dseg[b, c, y-u+2, x-v+2]: M = (class, tap) rows of up to two classes,
// N = 32 channels, K = ALL pixels of the episode.  One workgroup of eight waves per (episode, class pair, channel chunk): wave w takes the
// pixel quads w, w + 8, ... in index order, the eight partial tiles are added in wave order through LDS.  Nothing is accumulated across
// workgroups, so the reduction order is a function of the shape alone.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512) void classify_conv_dk_kernel(const float* __restrict__ dseg, const float* __restrict__ feat, int C, int H, int W,
                                                               int cf, float* __restrict__ dK) {
  __shared__ float red[8 * 64 * 32];
  const int b = blockIdx.z, c0 = blockIdx.y * 2, d0 = blockIdx.x * 32;
  const int nc = min(2, C - c0);
  const int HW = H * W;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4, n = lane & 15;
  int ac[4], au[4], av[4];
  bool arow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = i * 16 + n;
    arow[i] = m < 25 * nc;
    const int tap = m % 25;
    ac[i] = arow[i] ? m / 25 : 0;
    au[i] = tap / 5;
    av[i] = tap % 5;
  }
  const float* dsb = dseg + ((size_t)b * C + c0) * HW;
  const float* fb = feat + (size_t)b * HW * cf + d0 + n;
  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    for (int t = 0; t < 2; ++t) acc[i][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int p0 = 4 * wv; p0 < HW; p0 += 32) {
    const int p = p0 + q;
    const bool pin = p < HW;
    const int y = pin ? p / W : 0, x = pin ? p % W : 0;
    float a[4], bv[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int yy = y - au[i] + 2, xx = x - av[i] + 2;
      a[i] = (pin && arow[i] && yy >= 0 && yy < H && xx >= 0 && xx < W) ? dsb[((size_t)ac[i] * H + yy) * W + xx] : 0.f;
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) bv[t] = pin ? fb[(size_t)p * cf + t * 16] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[i][t] = mfma4(a[i], bv[t], acc[i][t]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[(wv * 64 + i * 16 + 4 * q + r) * 32 + t * 16 + n] = acc[i][t][r];
  __syncthreads();
  for (int e = threadIdx.x; e < 25 * nc * 32; e += 512) {
    const int m = e >> 5, col = e & 31;
    float s = red[m * 32 + col];
#pragma unroll
    for (int w = 1; w < 8; ++w) s += red[(w * 64 + m) * 32 + col];
    dK[(((size_t)b * C + c0) * 25 + m) * cf + d0 + col] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// prototype_tconv: k1[bc][m][ij] = sum_in e[bc][in] W1[in][m][ij];  K[bc][(a+i, b+j)][o] = sum_m sum_ab sum_ij k1[bc][m][ab] W2[m][o][ij].
// Small (10.6 MMAC per prototype at cf = 256) and weight-bound; plain fmaf in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void proto_k1_kernel(const float* __restrict__ e, const float* __restrict__ W1, long total, int cf,
                                                       float* __restrict__ k1) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int per = cf * 9;
  const long bc = gid / per;
  const int r = (int)(gid % per);
  const float* ev = e + bc * cf;
  float s = 0.f;
  for (int in = 0; in < cf; ++in) s = fmaf(ev[in], W1[(size_t)in * per + r], s);
  k1[gid] = s;
}

// a workgroup = one prototype x 64 output channels x four slices of m; the slices are added in slice order through LDS
__global__ __launch_bounds__(256) void proto_k2_kernel(const float* __restrict__ k1, const float* __restrict__ W2, int cf, float* __restrict__ K) {
  __shared__ float red[4 * 25 * 64];
  const int bc = blockIdx.y, o0 = blockIdx.x * 64;
  const int ms = threadIdx.x >> 6, ol = threadIdx.x & 63, o = o0 + ol;
  float acc[25];
#pragma unroll
  for (int t = 0; t < 25; ++t) acc[t] = 0.f;
  if (o < cf) {
    const int mq = cf / 4;
    for (int m = ms * mq; m < (ms + 1) * mq; ++m) {
      const float* kp = k1 + ((size_t)bc * cf + m) * 9;
      const float* wp = W2 + ((size_t)m * cf + o) * 9;
      float kv[9], wv[9];
#pragma unroll
      for (int t = 0; t < 9; ++t) { kv[t] = kp[t]; wv[t] = wp[t]; }
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int bb = 0; bb < 3; ++bb)
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[(a + i) * 5 + bb + j] = fmaf(kv[a * 3 + bb], wv[i * 3 + j], acc[(a + i) * 5 + bb + j]);
    }
  }
#pragma unroll
  for (int t = 0; t < 25; ++t) red[(ms * 25 + t) * 64 + ol] = acc[t];
  __syncthreads();
  for (int e = threadIdx.x; e < 25 * 64; e += 256) {
    const int tap = e >> 6, l = e & 63;
    if (o0 + l < cf)
      K[((size_t)bc * 25 + tap) * cf + o0 + l] = ((red[tap * 64 + l] + red[(25 + tap) * 64 + l]) + red[(50 + tap) * 64 + l]) + red[(75 + tap) * 64 + l];
  }
}

// dk1[bc][m][ab] = sum_o sum_ij dK[bc][(a+i, b+j)][o] W2[m][o][ij]; one thread per (bc, m)
__global__ __launch_bounds__(64) void proto_dk1_kernel(const float* __restrict__ dK, const float* __restrict__ W2, int cf, float* __restrict__ dk1) {
  const int bc = blockIdx.y, m = blockIdx.x * 64 + threadIdx.x;
  if (m >= cf) return;
  float acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.f;
  for (int o = 0; o < cf; ++o) {
    const float* wp = W2 + ((size_t)m * cf + o) * 9;
    float g[25], wv[9];
#pragma unroll
    for (int t = 0; t < 25; ++t) g[t] = dK[((size_t)bc * 25 + t) * cf + o];
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[t] = wp[t];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int bb = 0; bb < 3; ++bb)
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) acc[a * 3 + bb] = fmaf(g[(a + i) * 5 + bb + j], wv[i * 3 + j], acc[a * 3 + bb]);
  }
#pragma unroll
  for (int t = 0; t < 9; ++t) dk1[((size_t)bc * cf + m) * 9 + t] = acc[t];
}

// dW2[m][o][ij] += sum_bc sum_ab k1[bc][m][ab] dK[bc][(a+i, b+j)][o]; one thread per (m, o), prototypes in index order
__global__ __launch_bounds__(64) void proto_dw2_kernel(const float* __restrict__ dK, const float* __restrict__ k1, int BC, int cf,
                                                       float* __restrict__ dW2) {
  const int m = blockIdx.y, o = blockIdx.x * 64 + threadIdx.x;
  if (o >= cf) return;
  float acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = 0.f;
  for (int bc = 0; bc < BC; ++bc) {
    const float* kp = k1 + ((size_t)bc * cf + m) * 9;
    float g[25], kv[9];
#pragma unroll
    for (int t = 0; t < 25; ++t) g[t] = dK[((size_t)bc * 25 + t) * cf + o];
#pragma unroll
    for (int t = 0; t < 9; ++t) kv[t] = kp[t];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int bb = 0; bb < 3; ++bb) acc[i * 3 + j] = fmaf(kv[a * 3 + bb], g[(a + i) * 5 + bb + j], acc[i * 3 + j]);
  }
  float* out = dW2 + ((size_t)m * cf + o) * 9;
#pragma unroll
  for (int t = 0; t < 9; ++t) out[t] += acc[t];
}

// dprotos[bc][in] = sum_r dk1[bc][r] W1[in][r] over r < 9 cf: one wave per output, lanes stride r, fixed butterfly
__global__ __launch_bounds__(64) void proto_de_kernel(const float* __restrict__ dk1, const float* __restrict__ W1, int cf, float* __restrict__ de) {
  const int bc = blockIdx.y, in = blockIdx.x;
  const int per = cf * 9;
  const float* g = dk1 + (size_t)bc * per;
  const float* wp = W1 + (size_t)in * per;
  float s = 0.f;
  for (int r = threadIdx.x; r < per; r += 64) s = fmaf(g[r], wp[r], s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (threadIdx.x == 0) de[(size_t)bc * cf + in] = s;
}

// dW1[in][r] += sum_bc e[bc][in] dk1[bc][r]
__global__ __launch_bounds__(256) void proto_dw1_kernel(const float* __restrict__ e, const float* __restrict__ dk1, int BC, int cf,
                                                        float* __restrict__ dW1) {
  const int per = cf * 9;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (long)cf * per) return;
  const int in = (int)(gid / per), r = (int)(gid % per);
  float s = 0.f;
  for (int bc = 0; bc < BC; ++bc) s = fmaf(e[(size_t)bc * cf + in], dk1[(size_t)bc * per + r], s);
  dW1[gid] += s;
}

}  // namespace la

static bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static bool convcls_ok(const char* who, int B, int C, int H, int W, int cf) {
  if (B <= 0 || B > 65535 || C <= 0 || C > 65535 || H <= 0 || W <= 0 || H > 16384 || W > 16384) {
    la_set_error("%s: bad sizes B=%d C=%d map %d x %d (B, C 1..65535, sides 1..16384)", who, B, C, H, W);
    return false;
  }
  if (cf < 32 || cf > 256 || (cf % 32) != 0) {
    la_set_error("%s: cf=%d must be a multiple of 32 up to 256", who, cf);
    return false;
  }
  return true;
}

extern "C" int la_classify_conv(const float* feat, const float* K, int B, int C, int H, int W, int cf, float* seg, void* stream) {
  LA_CHECK_ARG(feat && K && seg, "la_classify_conv: null pointer");
  if (!convcls_ok("la_classify_conv", B, C, H, W, cf)) return -1;
  LA_CHECK_ARG(al16(feat) && al16(K), "la_classify_conv: 16-byte aligned feat / K");
  const int ntx = (W + la::CC_T - 1) / la::CC_T, nty = (H + la::CC_T - 1) / la::CC_T;
  hipStream_t st = (hipStream_t)stream;
  // class pairs on the 64-column kernel; an odd last class on the 32-column one, which issues half the MFMA work for it
  if (C >= 2) {
    hipLaunchKernelGGL(la::classify_conv_kernel<4>, dim3(ntx * nty, C / 2, B), dim3(256), 0, st, feat, K, C, H, W, cf, ntx, 0, seg);
    LA_CHECK_LAUNCH("la_classify_conv (class pairs)");
  }
  if (C & 1) hipLaunchKernelGGL(la::classify_conv_kernel<2>, dim3(ntx * nty, 1, B), dim3(256), 0, st, feat, K, C, H, W, cf, ntx, C - 1, seg);
  LA_CHECK_LAUNCH("la_classify_conv");
  return 0;
}

extern "C" int la_classify_conv_bwd(const float* dseg, const float* feat, const float* K, int B, int C, int H, int W, int cf, float* dfeat,
                                    float* dK, void* stream) {
  LA_CHECK_ARG(dseg && feat && K && dfeat && dK, "la_classify_conv_bwd: null pointer");
  if (!convcls_ok("la_classify_conv_bwd", B, C, H, W, cf)) return -1;
  LA_CHECK_ARG(al16(feat) && al16(K), "la_classify_conv_bwd: 16-byte aligned feat / K");
  hipLaunchKernelGGL(la::classify_conv_dfeat_kernel, dim3((H * W + 127) / 128, cf / 32, B), dim3(256), 0, (hipStream_t)stream, dseg, K, C, H, W, cf,
                     dfeat);
  LA_CHECK_LAUNCH("la_classify_conv_bwd (dfeat)");
  hipLaunchKernelGGL(la::classify_conv_dk_kernel, dim3(cf / 32, (C + 1) / 2, B), dim3(512), 0, (hipStream_t)stream, dseg, feat, C, H, W, cf, dK);
  LA_CHECK_LAUNCH("la_classify_conv_bwd (dK)");
  return 0;
}

static bool proto_ok(const char* who, int BC, int cf) {
  if (BC <= 0 || BC > 65535 || cf < 32 || cf > 256 || (cf % 32) != 0) {
    la_set_error("%s: BC=%d (1..65535), cf=%d (a multiple of 32 up to 256)", who, BC, cf);
    return false;
  }
  return true;
}

extern "C" int la_proto_kernels(const float* protos, const float* W1, const float* W2, int BC, int cf, float* k1, float* K, void* stream) {
  LA_CHECK_ARG(protos && W1 && W2 && k1 && K, "la_proto_kernels: null pointer");
  if (!proto_ok("la_proto_kernels", BC, cf)) return -1;
  const long total = (long)BC * cf * 9;
  hipLaunchKernelGGL(la::proto_k1_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, protos, W1, total, cf, k1);
  LA_CHECK_LAUNCH("la_proto_kernels (k1)");
  hipLaunchKernelGGL(la::proto_k2_kernel, dim3((cf + 63) / 64, BC), dim3(256), 0, (hipStream_t)stream, k1, W2, cf, K);
  LA_CHECK_LAUNCH("la_proto_kernels (K)");
  return 0;
}

extern "C" int la_proto_kernels_bwd(const float* dK, const float* protos, const float* k1, const float* W1, const float* W2, int BC, int cf,
                                    float* dk1, float* dprotos, float* dW1, float* dW2, void* stream) {
  LA_CHECK_ARG(dK && protos && k1 && W1 && W2 && dk1 && dprotos && dW1 && dW2, "la_proto_kernels_bwd: null pointer");
  if (!proto_ok("la_proto_kernels_bwd", BC, cf)) return -1;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(la::proto_dk1_kernel, dim3((cf + 63) / 64, BC), dim3(64), 0, s, dK, W2, cf, dk1);
  LA_CHECK_LAUNCH("la_proto_kernels_bwd (dk1)");
  hipLaunchKernelGGL(la::proto_dw2_kernel, dim3((cf + 63) / 64, cf), dim3(64), 0, s, dK, k1, BC, cf, dW2);
  LA_CHECK_LAUNCH("la_proto_kernels_bwd (dW2)");
  hipLaunchKernelGGL(la::proto_de_kernel, dim3(cf, BC), dim3(64), 0, s, dk1, W1, cf, dprotos);
  LA_CHECK_LAUNCH("la_proto_kernels_bwd (dprotos)");
  hipLaunchKernelGGL(la::proto_dw1_kernel, dim3((unsigned)(((long)cf * cf * 9 + 255) / 256)), dim3(256), 0, s, protos, dk1, BC, cf, dW1);
  LA_CHECK_LAUNCH("la_proto_kernels_bwd (dW1)");
  return 0;
}
