// Loss components of LabelAnythingLoss beyond the focal term: the logits objective (focal + dice + false positive, any subset, fused
// with its gradient) and the prompt-contrastive term over the class-example embeddings.
//
// Reference (loss/__init__.py:67-89, loss/focal.py:17-26, loss/dice.py, loss/fp.py, loss/prompt.py:10-48, loss/utils.py:17-43):
//   focal  mean over ALL B*HW pixels of (1 - pt)^gamma * w[t] * ce (w: class weighting of the whole batch, 0 at ignored pixels)
//   dice   p = softmax; per (b, c): I = sum p * [t == c], U = sum p + sum [t == c], over every pixel (ignored ones add their p);
//          L = mean_b mean_c w_c * (1 - (2 I + eps) / (U + eps)), eps 1e-6, w_c = 1 without class weighting
//   fp     a[b][c] = class c absent from image b once ignored targets read as 0; per non-ignored pixel sum_c p_c a / (A_b + 1e-6)
//          with A_b = sum_c a[b][c]; L = sum over pixels / number of non-ignored pixels
// Four launches for the logits objective: per-image label histogram -> (dice only) per-(image, class) sums of p and of p at the
// target from per-workgroup fp64 partials -> per-image coefficients -> one workgroup pass per tile that writes dlogits once -> fold.
// A pixel's C logits are re-read per pass over the planes (max, sum of exp, then p = exp(x - max) / sum recomputed where needed):
// lo_dice_sums makes three passes, lo_fused four; the re-reads of a tile are meant to hit the caches (not measured separately).
// Every workgroup covers one tile of ONE image; every sum runs in a fixed order (no float atomics).
#include <algorithm>

#include "la_common.h"
#include "../../include/la_hip.h"

#pragma clang fp contract(off)

namespace la {

constexpr int LO_MAXC = 64;          // classes per episode (== wave size: lane c owns class c in the dice sums)
constexpr int LO_BLOCKS = 2048;      // workgroups over all images
constexpr int LO_FOCAL = 1, LO_DICE = 2, LO_FP = 4;
constexpr int PC_MAXN = 1024, PC_MAXD = 1024;

struct LoLayout {
  int tiles;
  long tile_len;
  long counts, wcls, coef, dterm, dpart, vpart, bytes;
};

static inline long lo_align(long v) { return (v + 255) / 256 * 256; }

static LoLayout lo_layout(int B, int C, long HW) {
  LoLayout l;
  const long per = (LO_BLOCKS + B - 1) / B;
  const long max_tiles = std::max(1L, (HW + 1023) / 1024);
  long tiles = std::max(1L, std::min(per, max_tiles));
  l.tile_len = ((HW + tiles - 1) / tiles + 3) / 4 * 4;                  // a multiple of 4: the float4 path never straddles a tile
  l.tiles = (int)((HW + l.tile_len - 1) / l.tile_len);
  long off = 0;
  l.counts = off; off = lo_align(off + (long)B * (C + 2) * 8);         // uint64 [B, C + 2]: 0 ignore, 1 + c class c, C + 1 out of range
  l.wcls = off;   off = lo_align(off + (long)C * 4);                    // fp32 [C] class weights
  l.coef = off;   off = lo_align(off + (long)B * C * 4 * 4);            // fp32 [B, C, 4]: dice alpha, beta, fp gradient, fp value
  l.dterm = off;  off = lo_align(off + (long)B * C * 8);                // fp64 [B, C] weighted dice terms
  l.dpart = off;  off = lo_align(off + (long)B * l.tiles * C * 2 * 8);  // fp64 [B, tiles, C, 2] sum p, sum p at target
  l.vpart = off;  off = lo_align(off + (long)B * l.tiles * 2 * 8);      // fp64 [B, tiles, 2] focal, fp value partials
  l.bytes = off;
  return l;
}

template <int V> __device__ __forceinline__ void lo_load(const float* __restrict__ p, float (&x)[V]) {
  if constexpr (V == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
  } else {
    x[0] = p[0];
  }
}
template <int V> __device__ __forceinline__ void lo_store(float* __restrict__ p, const float (&x)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  else p[0] = x[0];
}

// max and sum of exp over the classes of V pixels (two passes over the planes: exactly the softmax the reference evaluates)
template <int V>
__device__ __forceinline__ void lo_softmax_stats(const float* __restrict__ xp, int C, long HW, float (&mx)[V], float (&se)[V]) {
  float x[V];
#pragma unroll
  for (int v = 0; v < V; ++v) mx[v] = -INFINITY, se[v] = 0.f;
  for (int c = 0; c < C; ++c) {
    lo_load<V>(xp + (long)c * HW, x);
#pragma unroll
    for (int v = 0; v < V; ++v) mx[v] = fmaxf(mx[v], x[v]);
  }
  for (int c = 0; c < C; ++c) {
    lo_load<V>(xp + (long)c * HW, x);
#pragma unroll
    for (int v = 0; v < V; ++v) se[v] += expf(x[v] - mx[v]);
  }
}

// grid (tiles, B), 256 threads: per-image label histogram, integer atomics only
__global__ __launch_bounds__(256) void lo_hist_kernel(const long long* __restrict__ target, long HW, long tile_len, int C, long long ignore,
                                                      unsigned long long* __restrict__ counts) {
  __shared__ unsigned h[LO_MAXC + 2];
  const int b = blockIdx.y;
  for (int i = threadIdx.x; i <= C + 1; i += 256) h[i] = 0;
  __syncthreads();
  const long p0 = (long)blockIdx.x * tile_len, p1 = p0 + tile_len < HW ? p0 + tile_len : HW;
  const long long* tb = target + (long)b * HW;
  for (long i = p0 + threadIdx.x; i < p1; i += 256) {
    const long long t = tb[i];
    if (t == ignore) atomicAdd(&h[0], 1u);
    else if (t >= 0 && t < C) atomicAdd(&h[1 + (int)t], 1u);
    else atomicAdd(&h[C + 1], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= C + 1; i += 256)
    if (h[i]) atomicAdd(&counts[(long)b * (C + 2) + i], (unsigned long long)h[i]);
}

// grid (tiles, B), 256 threads: dpart[b, tile, c] = (sum p_c, sum p_c [t == c]) over the tile.  Each wave reduces one class at a time
// with an xor butterfly (every lane ends with the same bits); lane c keeps class c's running fp64 sum.
template <int V>
__global__ __launch_bounds__(256) void lo_dice_sums_kernel(const float* __restrict__ x, const long long* __restrict__ target, int C, long HW,
                                                           long tile_len, long long ignore, double* __restrict__ dpart) {
  __shared__ double red[4][LO_MAXC][2];
  const int b = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const float* xb = x + (long)b * C * HW;
  const long long* tb = target + (long)b * HW;
  const long p0 = (long)tile * tile_len, p1 = p0 + tile_len < HW ? p0 + tile_len : HW;
  double accp = 0.0, acci = 0.0;
  for (long base = p0; base < p1; base += 256L * V) {
    const long i = base + (long)tid * V;
    const bool ok = i < p1;
    float mx[V], se[V], xv[V];
    int tc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) mx[v] = 0.f, se[v] = 1.f, tc[v] = -1;
    if (ok) {
      lo_softmax_stats<V>(xb + i, C, HW, mx, se);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const long long t = tb[i + v];
        tc[v] = (t != ignore && t >= 0 && t < C) ? (int)t : -1;
      }
    }
    for (int c = 0; c < C; ++c) {
      float sp = 0.f, si = 0.f;
      if (ok) {
        lo_load<V>(xb + (long)c * HW + i, xv);
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float p = expf(xv[v] - mx[v]) / se[v];
          sp += p;
          if (tc[v] == c) si += p;
        }
      }
      sp = wave_sum(sp);
      si = wave_sum(si);
      if (lane == c) {
        accp += (double)sp;
        acci += (double)si;
      }
    }
  }
  if (lane < C) {
    red[wave][lane][0] = accp;
    red[wave][lane][1] = acci;
  }
  __syncthreads();
  if (tid < C) {
    double sp = 0.0, si = 0.0;
    for (int w = 0; w < 4; ++w) sp += red[w][tid][0], si += red[w][tid][1];
    double* o = dpart + (((long)b * tiles + tile) * C + tid) * 2;
    o[0] = sp;
    o[1] = si;
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);    // xor butterfly: every lane ends with the same bits
  return v;
}

// grid (C, B), one wave per (image, class): class weights of the batch, dice terms and gradient coefficients, fp coefficients.  The
// lanes fold the per-tile dice partials (lane-strided, then a butterfly); lane 0 does the rest.
__global__ __launch_bounds__(64) void lo_coef_kernel(const unsigned long long* __restrict__ counts, const double* __restrict__ dpart, int B,
                                                     int C, long HW, int tiles, int mask, int class_weighting, float w_dice, float w_fp,
                                                     float* __restrict__ wcls, float* __restrict__ coef,
                                                     double* __restrict__ dterm, float* __restrict__ class_weights) {
  const int b = blockIdx.y, c = blockIdx.x, lane = threadIdx.x;
  double sp = 0.0, si = 0.0;
  if (mask & LO_DICE) {
    for (int t = lane; t < tiles; t += 64) {
      const double* o = dpart + (((long)b * tiles + t) * C + c) * 2;
      sp += o[0];
      si += o[1];
    }
    sp = wave_sum_f64(sp);
    si = wave_sum_f64(si);
  }
  if (lane != 0) return;
  const long n = (long)B * HW;
  unsigned long long cnt = 0, ign_all = 0;
  for (int j = 0; j < B; ++j) {
    cnt += counts[(long)j * (C + 2) + 1 + c];
    ign_all += counts[(long)j * (C + 2)];
  }
  // get_weight_matrix_from_labels: 1 / log(1.1 + count / (B * HW)) for the classes present, 1 for the others (focal and dice)
  float w = 1.0f;
  if (class_weighting && cnt > 0) w = 1.0f / logf(1.1f + (float)cnt / (float)n);
  if (b == 0) {
    wcls[c] = w;
    if (class_weights) class_weights[c] = w;
  }
  const unsigned long long* cb = counts + (long)b * (C + 2);
  float* cf = coef + ((long)b * C + c) * 4;
  // dice (loss/dice.py:96-113): the macro mean of the weighted per-(b, c) terms
  double al = 0.0, be = 0.0, term = 0.0;
  if (mask & LO_DICE) {
    const double eps = 1e-6, u = sp + (double)cb[1 + c] + eps, num = 2.0 * si + eps;
    term = (double)w * (1.0 - num / u);
    const double k = (double)w_dice * (double)w_dice * (double)w / ((double)B * (double)C);
    al = k * num / (u * u);                  // d/dp of -(2I + eps) / (U + eps) = (2I + eps) / (U + eps)^2 - 2 [t == c] / (U + eps)
    be = k * 2.0 / u;
  }
  dterm[(long)b * C + c] = term;
  // false positive (loss/fp.py): presence after ignored targets read as class 0
  int absent = 0;
  for (int j = 0; j < C; ++j) absent += (cb[1 + j] == 0 && !(j == 0 && cb[0] > 0)) ? 1 : 0;
  const int a = (cb[1 + c] == 0 && !(c == 0 && cb[0] > 0)) ? 1 : 0;
  const float r = 1.0f / ((float)absent + 1e-6f);
  const unsigned long long valid = (unsigned long long)n - ign_all;
  float fg = 0.f, fv = 0.f;
  if (mask & LO_FP) {
    fv = a ? r : 0.f;
    if (valid > 0) fg = (float)((double)w_fp * (double)w_fp * (double)fv / (double)valid);
  }
  cf[0] = (float)al;
  cf[1] = (float)be;
  cf[2] = fg;
  cf[3] = fv;
}

// grid (tiles, B), 256 threads: per pixel the softmax statistics, focal value and gradient, dice and fp gradients through the softmax
// (dz_j = p_j (g_j - sum_k p_k g_k)), dlogits written once; per-workgroup fp64 partials of the focal and fp values
template <int V>
__global__ __launch_bounds__(256) void lo_fused_kernel(const float* __restrict__ x, const long long* __restrict__ target, int B, int C,
                                                       long HW, long tile_len, long long ignore, int mask, float gamma, float w_focal,
                                                       const float* __restrict__ wcls, const float* __restrict__ coef,
                                                       float* __restrict__ dx, double* __restrict__ vpart) {
  __shared__ float s_w[LO_MAXC], s_al[LO_MAXC], s_be[LO_MAXC], s_fg[LO_MAXC], s_fv[LO_MAXC];
  __shared__ double red[2][256];
  const int b = blockIdx.y, tile = blockIdx.x, tiles = gridDim.x, tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) {
    const float* cf = coef + ((long)b * C + c) * 4;
    s_w[c] = wcls[c];
    s_al[c] = cf[0];
    s_be[c] = cf[1];
    s_fg[c] = cf[2];
    s_fv[c] = cf[3];
  }
  __syncthreads();
  const bool focal = mask & LO_FOCAL, smooth = mask & (LO_DICE | LO_FP);
  const float inv_n = w_focal * w_focal / (float)((long)B * HW);
  const float* xb = x + (long)b * C * HW;
  const long long* tb = target + (long)b * HW;
  float* db = dx ? dx + (long)b * C * HW : nullptr;
  const long p0 = (long)tile * tile_len, p1 = p0 + tile_len < HW ? p0 + tile_len : HW;
  double accf = 0.0, accp = 0.0;
  for (long i = p0 + (long)tid * V; i < p1; i += 256L * V) {
    float mx[V], se[V], xv[V], S[V], xt[V], fk[V], fpm[V], fps[V];
    int tc[V];
    lo_softmax_stats<V>(xb + i, C, HW, mx, se);
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const long long t = tb[i + v];
      tc[v] = (t >= 0 && t < C && t != ignore) ? (int)t : -1;
      fpm[v] = t != ignore ? 1.f : 0.f;          // fp.py: mask = target != ignore_index
      S[v] = 0.f, xt[v] = 0.f, fk[v] = 0.f, fps[v] = 0.f;
    }
    for (int c = 0; c < C; ++c) {
      lo_load<V>(xb + (long)c * HW + i, xv);
#pragma unroll
      for (int v = 0; v < V; ++v) {
        if (tc[v] == c) xt[v] = xv[v];
        if (smooth) {
          const float p = expf(xv[v] - mx[v]) / se[v];
          const float g = s_al[c] + s_fg[c] * fpm[v] - (tc[v] == c ? s_be[c] : 0.f);
          S[v] += p * g;
          fps[v] += p * s_fv[c];
        }
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      if (focal && tc[v] >= 0) {
        const float ce = logf(se[v]) - (xt[v] - mx[v]);      // shift-stable: mx + logf(se) - x_t loses ulp(mx) to a common offset
        const float pt = expf(-ce);
        const float om = 1.0f - pt;
        const float wt = s_w[tc[v]];
        accf += (double)(powf(om, gamma) * wt * ce);
        const float g = powf(om, gamma) + (om > 0.f ? gamma * ce * pt * powf(om, gamma - 1.0f) : 0.f);
        fk[v] = inv_n * wt * g;
      }
      if (mask & LO_FP) accp += (double)(fps[v] * fpm[v]);
    }
    if (db) {
      for (int c = 0; c < C; ++c) {
        lo_load<V>(xb + (long)c * HW + i, xv);
        float d[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const float p = expf(xv[v] - mx[v]) / se[v];
          float dv = fk[v] * (p - (c == tc[v] ? 1.0f : 0.0f));
          if (smooth) dv += p * ((s_al[c] + s_fg[c] * fpm[v] - (tc[v] == c ? s_be[c] : 0.f)) - S[v]);
          d[v] = dv;
        }
        lo_store<V>(db + (long)c * HW + i, d);
      }
    }
  }
  red[0][tid] = accf;
  red[1][tid] = accp;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* o = vpart + ((long)b * tiles + tile) * 2;
    o[0] = red[0][0];
    o[1] = red[1][0];
  }
}

// one wave: the components and the total in a fixed order (lane-strided partial sums, then a butterfly)
__global__ __launch_bounds__(64) void lo_fold_kernel(const unsigned long long* __restrict__ counts, const double* __restrict__ dterm, const double* __restrict__ vpart,
                               int B, int C, long HW, int tiles, int mask, float w_focal, float w_dice, float w_fp, float* __restrict__ value,
                               float* __restrict__ components) {
  const int lane = threadIdx.x;
  double focal = 0.0, fp = 0.0, dice = 0.0;
  for (long r = lane; r < (long)B * tiles; r += 64) {
    focal += vpart[r * 2];
    fp += vpart[r * 2 + 1];
  }
  focal = wave_sum_f64(focal);
  fp = wave_sum_f64(fp);
  if (lane != 0) return;
  unsigned long long ign = 0;
  for (int b = 0; b < B; ++b) {
    ign += counts[(long)b * (C + 2)];
    double row = 0.0;
    for (int c = 0; c < C; ++c) row += dterm[(long)b * C + c];
    dice += row / (double)C;
  }
  const long n = (long)B * HW;
  focal /= (double)n;
  dice /= (double)B;
  fp /= (double)(n - (long)ign);                     // no valid pixel: 0 / 0, as the reference
  const double lf = (mask & LO_FOCAL) ? focal : 0.0, ld = (mask & LO_DICE) ? dice : 0.0, lp = (mask & LO_FP) ? fp : 0.0;
  // logits components enter the total with their weight squared and are reported with it once (loss/__init__.py:78,87)
  components[0] = (float)((double)w_focal * lf);
  components[1] = (float)((double)w_dice * ld);
  components[2] = (float)((double)w_fp * lp);
  value[0] = (float)((double)w_focal * w_focal * lf + (double)w_dice * w_dice * ld + (double)w_fp * w_fp * lp);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Prompt contrastive (loss/prompt.py:10-48): rows e_i = class_examples_embeddings[b] in (m, c) order, L2-normalised (F.normalize, eps
// 1e-12); z_ij = (e_i . e_j) exp(t') + bias; y_ij = +1 for the same class index (i % C == j % C), -1 otherwise; each pair i < j of
// flagged rows adds softplus(-y z) / (valid_b * B).
// ---------------------------------------------------------------------------------------------------------------------------------
struct PcLayout {
  long ehat, den, part, bytes;
};
static PcLayout pc_layout(int B, int n, int D) {
  PcLayout l;
  long off = 0;
  l.ehat = off; off = lo_align(off + (long)B * n * D * 4);
  l.den = off;  off = lo_align(off + (long)B * n * 4 * 2);           // fp32 [B, n, 2]: clamped norm, raw norm
  l.part = off; off = lo_align(off + (long)B * n * 3 * 8);           // fp64 [B, n, 3]: loss, d t', d bias of the pairs (i, j > i)
  l.bytes = off;
  return l;
}

__device__ __forceinline__ float pc_block_sum(float v, float* red4) {
  v = wave_sum(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red4[wave] = v;
  __syncthreads();
  return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// grid (n, B), 256 threads: ehat = e / max(||e||, 1e-12)
__global__ __launch_bounds__(256) void pc_normalize_kernel(const float* __restrict__ emb, int n, int D, float* __restrict__ ehat,
                                                           float* __restrict__ den) {
  __shared__ float red4[4];
  const long row = (long)blockIdx.y * n + blockIdx.x;
  const float* e = emb + row * D;
  float ss = 0.f;
  for (int d = threadIdx.x; d < D; d += 256) ss += e[d] * e[d];
  const float nrm = sqrtf(pc_block_sum(ss, red4));
  const float dd = fmaxf(nrm, 1e-12f);
  for (int d = threadIdx.x; d < D; d += 256) ehat[row * D + d] = e[d] / dd;
  if (threadIdx.x == 0) {
    den[row * 2] = dd;
    den[row * 2 + 1] = nrm;
  }
}

__device__ __forceinline__ float pc_softplus(float u) { return fmaxf(u, 0.f) + log1pf(expf(-fabsf(u))); }
__device__ __forceinline__ float pc_sigmoid(float u) {
  if (u >= 0.f) return 1.0f / (1.0f + expf(-u));
  const float e = expf(u);
  return e / (1.0f + e);
}

// grid (n, B), 256 threads: block (i, b) computes s_ij for every j (one wave per j), the pair gradients G_ij = dL/ds_ij, row i's
// gradient through F.normalize, and the partial sums of the pairs (i, j > i)
__global__ __launch_bounds__(256) void pc_pairs_kernel(const float* __restrict__ ehat, const float* __restrict__ den,
                                                       const unsigned char* __restrict__ flags, int B, int n, int C, int D,
                                                       const float* __restrict__ t_prime, const float* __restrict__ bias,
                                                       float* __restrict__ demb, double* __restrict__ part) {
  __shared__ float s_ei[PC_MAXD], s_g[PC_MAXN], red4[4];
  __shared__ double s_red[4][3];
  __shared__ int s_valid;
  const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long row = (long)b * n + i;
  const float* eb = ehat + (long)b * n * D;
  const unsigned char* fb = flags + (long)b * n;
  if (tid == 0) s_valid = 0;
  for (int d = tid; d < D; d += 256) s_ei[d] = eb[(long)i * D + d];
  __syncthreads();
  int cnt = 0;
  for (int j = tid; j < n; j += 256) cnt += fb[j] ? 1 : 0;
  if (cnt) atomicAdd(&s_valid, cnt);
  __syncthreads();
  const bool fi = fb[i] != 0;
  const float et = expf(t_prime[0]), bs = bias[0];
  const float inv = fi ? 1.0f / ((float)s_valid * (float)B) : 0.f;
  double al = 0.0, at = 0.0, ab = 0.0;                  // lane 0 of each wave: its pairs (i, j > i) in increasing j
  for (int j = wave; j < n; j += 4) {
    float g = 0.f;
    if (fi && j != i && fb[j]) {                        // wave-uniform branch
      const float* ej = eb + (long)j * D;
      float s = 0.f;
      for (int d = lane; d < D; d += 64) s += s_ei[d] * ej[d];
      s = wave_sum(s);
      const float y = (j % C == i % C) ? 1.0f : -1.0f;
      const float z = s * et + bs;
      const float u = -y * z;
      const float dz = -y * pc_sigmoid(u) * inv;        // d softplus(-y z) / dz, divided by valid_b * B
      g = dz * et;
      if (lane == 0 && j > i) {
        al += (double)(pc_softplus(u) * inv);
        at += (double)(dz * s * et);
        ab += (double)dz;
      }
    }
    if (lane == 0) s_g[j] = g;
  }
  if (lane == 0) {
    s_red[wave][0] = al;
    s_red[wave][1] = at;
    s_red[wave][2] = ab;
  }
  __syncthreads();
  if (tid < 3) part[row * 3 + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
  // dL/dehat_i = sum_j G_ij ehat_j; back through x / max(||x||, eps)
  float gi[PC_MAXD / 256];
#pragma unroll
  for (int k = 0; k < PC_MAXD / 256; ++k) gi[k] = 0.f;
  if (fi) {
    for (int j = 0; j < n; ++j) {
      const float g = s_g[j];
      if (g == 0.f) continue;                           // block-uniform (LDS)
      const float* ej = eb + (long)j * D;
#pragma unroll
      for (int k = 0; k < PC_MAXD / 256; ++k) {
        const int d = tid + 256 * k;
        if (d < D) gi[k] += g * ej[d];
      }
    }
  }
  float dot = 0.f;
#pragma unroll
  for (int k = 0; k < PC_MAXD / 256; ++k) {
    const int d = tid + 256 * k;
    if (d < D) dot += s_ei[d] * gi[k];
  }
  dot = pc_block_sum(dot, red4);
  const float dd = den[row * 2], nrm = den[row * 2 + 1];
  const bool through = nrm >= 1e-12f;                   // clamp_min passes the gradient where norm >= eps
#pragma unroll
  for (int k = 0; k < PC_MAXD / 256; ++k) {
    const int d = tid + 256 * k;
    if (d < D) demb[row * D + d] = through ? (gi[k] - s_ei[d] * dot) / nrm : gi[k] / dd;
  }
}

// one wave: lane-strided partial sums in a fixed order, then a butterfly (deterministic, as lo_fold_kernel)
__global__ __launch_bounds__(64) void pc_fold_kernel(const double* __restrict__ part, long rows, float* __restrict__ loss,
                                                     float* __restrict__ dt, float* __restrict__ db) {
  double l = 0.0, t = 0.0, b = 0.0;
  for (long r = threadIdx.x; r < rows; r += 64) {
    l += part[r * 3];
    t += part[r * 3 + 1];
    b += part[r * 3 + 2];
  }
  l = wave_sum_f64(l);
  t = wave_sum_f64(t);
  b = wave_sum_f64(b);
  if (threadIdx.x != 0) return;
  loss[0] = (float)l;
  if (dt) dt[0] = (float)t;
  if (db) db[0] = (float)b;
}

}  // namespace la

extern "C" int la_logits_objective_workspace_bytes(int B, int C, long HW, long* bytes) {
  LA_CHECK_ARG(bytes && B > 0 && HW > 0 && C >= 2 && C <= la::LO_MAXC, "la_logits_objective_workspace_bytes: bad shape B=%d C=%d HW=%ld (C <= %d)",
               B, C, HW, la::LO_MAXC);
  *bytes = la::lo_layout(B, C, HW).bytes;
  return 0;
}

extern "C" int la_logits_objective(const float* logits, const long long* target, int B, int C, long HW, long long ignore_index, int mask,
                                   float w_focal, float gamma, float w_dice, float w_fp, int class_weighting, float* value, float* components,
                                   float* dlogits, float* class_weights, void* workspace, long workspace_bytes, void* stream) {
  LA_CHECK_ARG(logits && target && value && components && workspace, "la_logits_objective: null pointer");
  LA_CHECK_ARG(B > 0 && HW > 0 && C >= 2 && C <= la::LO_MAXC, "la_logits_objective: bad shape B=%d C=%d HW=%ld (C <= %d)", B, C, HW,
               la::LO_MAXC);
  LA_CHECK_ARG(mask > 0 && mask < 8, "la_logits_objective: component mask %d (1 focal | 2 dice | 4 fp)", mask);
  LA_CHECK_ARG(B <= 65535, "la_logits_objective: B=%d > 65535", B);
  const la::LoLayout l = la::lo_layout(B, C, HW);
  LA_CHECK_ARG(workspace_bytes >= l.bytes, "la_logits_objective: workspace needs %ld bytes", l.bytes);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  auto* counts = (unsigned long long*)(ws + l.counts);
  auto* wcls = (float*)(ws + l.wcls);
  auto* coef = (float*)(ws + l.coef);
  auto* dterm = (double*)(ws + l.dterm);
  auto* dpart = (double*)(ws + l.dpart);
  auto* vpart = (double*)(ws + l.vpart);
  if (hipMemsetAsync(counts, 0, (size_t)B * (C + 2) * 8, st) != hipSuccess) {
    la_set_error("la_logits_objective: memset failed");
    return -2;
  }
  const dim3 grid(l.tiles, B);
  const bool vec = HW % 4 == 0 && ((uintptr_t)logits & 15) == 0 && (!dlogits || ((uintptr_t)dlogits & 15) == 0);
  hipLaunchKernelGGL(la::lo_hist_kernel, grid, dim3(256), 0, st, target, HW, l.tile_len, C, ignore_index, counts);
  if (mask & la::LO_DICE) {
    if (vec) hipLaunchKernelGGL(la::lo_dice_sums_kernel<4>, grid, dim3(256), 0, st, logits, target, C, HW, l.tile_len, ignore_index, dpart);
    else hipLaunchKernelGGL(la::lo_dice_sums_kernel<1>, grid, dim3(256), 0, st, logits, target, C, HW, l.tile_len, ignore_index, dpart);
  }
  hipLaunchKernelGGL(la::lo_coef_kernel, dim3(C, B), dim3(64), 0, st, counts, dpart, B, C, HW, l.tiles, mask, class_weighting, w_dice, w_fp,
                     wcls, coef, dterm, class_weights);
  if (vec)
    hipLaunchKernelGGL(la::lo_fused_kernel<4>, grid, dim3(256), 0, st, logits, target, B, C, HW, l.tile_len, ignore_index, mask, gamma, w_focal,
                       wcls, coef, dlogits, vpart);
  else
    hipLaunchKernelGGL(la::lo_fused_kernel<1>, grid, dim3(256), 0, st, logits, target, B, C, HW, l.tile_len, ignore_index, mask, gamma, w_focal,
                       wcls, coef, dlogits, vpart);
  hipLaunchKernelGGL(la::lo_fold_kernel, dim3(1), dim3(64), 0, st, counts, dterm, vpart, B, C, HW, l.tiles, mask, w_focal, w_dice, w_fp, value,
                     components);
  LA_CHECK_LAUNCH("la_logits_objective");
  return 0;
}

extern "C" int la_prompt_contrastive_workspace_bytes(int B, int n, int D, long* bytes) {
  LA_CHECK_ARG(bytes && B > 0 && n > 0 && D > 0, "la_prompt_contrastive_workspace_bytes: bad shape B=%d n=%d D=%d", B, n, D);
  *bytes = la::pc_layout(B, n, D).bytes;
  return 0;
}

extern "C" int la_prompt_contrastive(const float* emb, const unsigned char* flags, int B, int n, int C, int D, const float* t_prime,
                                     const float* bias, float* loss, float* demb, float* dt_prime, float* dbias, void* workspace,
                                     long workspace_bytes, void* stream) {
  LA_CHECK_ARG(emb && flags && t_prime && bias && loss && demb && workspace, "la_prompt_contrastive: null pointer");
  LA_CHECK_ARG(B > 0 && B <= 65535 && C > 0 && n > 0 && n % C == 0 && D > 0, "la_prompt_contrastive: bad shape B=%d n=%d C=%d D=%d", B, n, C,
               D);
  LA_CHECK_ARG(n <= la::PC_MAXN && D <= la::PC_MAXD, "la_prompt_contrastive: n = M*C = %d rows and D = %d must be <= %d and <= %d", n, D,
               la::PC_MAXN, la::PC_MAXD);
  const la::PcLayout l = la::pc_layout(B, n, D);
  LA_CHECK_ARG(workspace_bytes >= l.bytes, "la_prompt_contrastive: workspace needs %ld bytes", l.bytes);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  auto* ehat = (float*)(ws + l.ehat);
  auto* den = (float*)(ws + l.den);
  auto* part = (double*)(ws + l.part);
  hipLaunchKernelGGL(la::pc_normalize_kernel, dim3(n, B), dim3(256), 0, st, emb, n, D, ehat, den);
  hipLaunchKernelGGL(la::pc_pairs_kernel, dim3(n, B), dim3(256), 0, st, ehat, den, flags, B, n, C, D, t_prime, bias, demb, part);
  hipLaunchKernelGGL(la::pc_fold_kernel, dim3(1), dim3(64), 0, st, part, (long)B * n, loss, dt_prime, dbias);
  LA_CHECK_LAUNCH("la_prompt_contrastive");
  return 0;
}
