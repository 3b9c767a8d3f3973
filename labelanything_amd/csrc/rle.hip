// Episode prompts and ground truths straight from COCO run-length annotations (reference data/coco.py:397-477,514-544,
// data/transforms.py:123-157,203-224): the reference decodes every annotation into a dense H x W array on the host and derives the
// per-class mask prompt, the point prompts and the label map from it.  Here the runs themselves are the device-side representation.
//   An annotation is `n` column-major runs that alternate 0 / 1 and start with a 0-run; la_rle_scan turns the counts into inclusive
//   run ends, so that pixel (x, y) of an h x w image - position p = x * h + y - lies in run r = #{ends <= p} and is set when r is odd.
//   la_rle_scan          counts -> ends + area, one wave per annotation
//   la_rle_decode        dense u8 masks of chosen annotations (building block / debugging aid; nothing below calls it)
//   la_rle_prompt_masks  apply_masks + annotations_to_tensor("mask") for every (image, class slot) of an episode in one launch
//   la_rle_ground_truth  compute_ground_truths + collate_gts: the last covering annotation in file order wins
//   la_rle_points        sample_point + apply_coords: the rank-th set pixel in np.argwhere (row-major) order
// Everything is integer work on a few hundred run ends per annotation (L1 / L2 resident); results are exact and deterministic (no
// floating-point or global atomics, fixed orders).  Annotation records are RLE_META ints: run offset, run count, h, w, image,
// class slot, order within the image, reserved.
#include "la_common.h"
#include "../../include/la_hip.h"

namespace la {

constexpr int RLE_META = 8;

__device__ __forceinline__ int wave_sum_i32(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// index of the run that holds position p = number of inclusive ends <= p (zero-length runs are stepped over); its parity is the pixel
__device__ __forceinline__ int rle_run_of(const int* __restrict__ ends, int n, int p) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ends[mid] <= p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void rle_scan_kernel(const int* __restrict__ runs, const int* __restrict__ meta, int K,
                                                       int* __restrict__ ends, int* __restrict__ area) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= K) return;
  const int off = meta[k * RLE_META], n = meta[k * RLE_META + 1];
  int carry = 0, ones = 0;
  for (int base = 0; base < n; base += 64) {                 // wave-inclusive scan of a 64-run chunk, carried into the next one
    const int i = base + lane;
    const int c = i < n ? runs[off + i] : 0;
    int v = c;
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o, 64);
      if (lane >= o) v += t;
    }
    if (i < n) ends[off + i] = carry + v;
    if (i & 1) ones += c;
    carry += __shfl(v, 63, 64);
  }
  ones = wave_sum_i32(ones);
  if (lane == 0) area[k] = ones;
}

// One 64 x 64 tile of a row-major output.  The lanes of a wave walk DOWN a column: neighbouring rows of one column are neighbouring
// positions of the column-major runs, so the 64 binary searches of a wave read the same few cache lines (along a row they would be h
// positions apart).  Values are parked in LDS (row stride 68 bytes = 17 banks: conflict-free both ways) and leave row-major, 64
// consecutive elements per wave.  value(row, col) -> u8 is only called inside [0, rows) x [0, cols); store(row, col, v) likewise.
// COLS == false is the plain mapping (lanes along a row, no LDS), kept for the measurement library's A/B (tools/rle_prompts_bench.py).
template <bool COLS, typename V, typename S>
__device__ __forceinline__ void rle_tile64(unsigned char (*tile)[68], int rows, int cols, int ty, int tx, V value, S store) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (!COLS) {
    for (int pass = 0; pass < 16; ++pass) {
      const int r2 = ty * 64 + pass * 4 + wave, c2 = tx * 64 + lane;
      if (r2 < rows && c2 < cols) store(r2, c2, value(r2, c2));
    }
    return;
  }
  const int r = ty * 64 + lane;
  for (int j = 0; j < 16; ++j) {
    const int c = tx * 64 + wave * 16 + j;
    tile[lane][wave * 16 + j] = (r < rows && c < cols) ? value(r, c) : (unsigned char)0;
  }
  __syncthreads();
  for (int pass = 0; pass < 16; ++pass) {
    const int lr = pass * 4 + wave;
    const int r2 = ty * 64 + lr, c2 = tx * 64 + lane;
    if (r2 < rows && c2 < cols) store(r2, c2, tile[lr][lane]);
  }
}

// grid (tiles of H x W, k): out u8 [k, H, W] of annotations sel[0..k) (all of size H x W - checked by the caller)
template <bool COLS>
__global__ __launch_bounds__(256) void rle_decode_kernel(const int* __restrict__ ends, const int* __restrict__ meta, const int* __restrict__ sel,
                                                         int H, int W, unsigned char* __restrict__ out) {
  __shared__ unsigned char tile[64][68];
  const int* m = meta + (size_t)sel[blockIdx.y] * RLE_META;
  const int* e = ends + m[0];
  const int n = m[1];
  const int tw = (W + 63) >> 6;
  unsigned char* o = out + (size_t)blockIdx.y * H * W;
  rle_tile64<COLS>(tile, H, W, blockIdx.x / tw, blockIdx.x % tw,
             [&](int y, int x) { return (unsigned char)(rle_run_of(e, n, x * H + y) & 1); },
             [&](int y, int x, unsigned char v) { o[(size_t)y * W + x] = v; });
}

// PromptsProcessor.apply_masks (data/transforms.py:203-224) for every (image, class slot) p = blockIdx.y of the episode: OR of the
// slot's annotations index[first[p] .. + count[p]), nearest resize (h, w) -> new_hw, zero pad to S x S, nearest resize to Mo x Mo,
// composed per output pixel exactly like prompt_mask_kernel (prep.hip) - but the source pixel is looked up in the runs, so no H x W
// buffer exists anywhere.  custom == 0: one resize (h, w) -> (Mo, Mo).  flags as in prompt_mask_kernel.
template <bool COLS>
__global__ __launch_bounds__(256) void rle_prompt_mask_kernel(const int* __restrict__ ends, const int* __restrict__ meta,
                                                              const int* __restrict__ first, const int* __restrict__ count,
                                                              const int* __restrict__ index, const int* __restrict__ img_hw,
                                                              const int* __restrict__ new_hw, int C, int custom, int S, int Mo,
                                                              float* __restrict__ out, unsigned char* __restrict__ flags) {
  __shared__ unsigned char tile[64][68];
  __shared__ int any_set;
  const int p = blockIdx.y, img = p / C;
  const int f = first[p], cnt = count[p];
  const int H = img_hw[2 * img], W = img_hw[2 * img + 1], nh = new_hw[2 * img], nw = new_hw[2 * img + 1];
  if (threadIdx.x == 0) any_set = 0;
  __syncthreads();
  const int tw = (Mo + 63) >> 6;
  float* o = out + (size_t)p * Mo * Mo;
  int mine = 0;
  rle_tile64<COLS>(tile, Mo, Mo, blockIdx.x / tw, blockIdx.x % tw,
             [&](int oy, int ox) {
               int sy, sx;
               if (custom) {
                 const int py = nearest_src(oy, S, Mo), px = nearest_src(ox, S, Mo);      // position on the padded S x S canvas
                 if (py >= nh || px >= nw) return (unsigned char)0;
                 sy = nearest_src(py, H, nh);
                 sx = nearest_src(px, W, nw);
               } else {
                 sy = nearest_src(oy, H, Mo);
                 sx = nearest_src(ox, W, Mo);
               }
               const int pos = sx * H + sy;
               int v = 0;
               for (int k = 0; k < cnt && !v; ++k) {
                 const int* m = meta + (size_t)index[f + k] * RLE_META;
                 v = rle_run_of(ends + m[0], m[1], pos) & 1;
               }
               mine |= v;
               return (unsigned char)v;
             },
             [&](int oy, int ox, unsigned char v) { o[(size_t)oy * Mo + ox] = (float)v; });
  if (mine) atomicOr(&any_set, 1);
  __syncthreads();
  if (threadIdx.x == 0 && any_set) flags[p] = 1;        // flags are zeroed by the caller; several blocks may set the same 1
}

// compute_ground_truths + collate_gts (data/coco.py:514-544, data/utils.py:388-393): grid (tiles of Hmax x Wmax, N).  The image's
// annotations index[first[img] .. + count[img]) are listed in file order; painting them in that order leaves the class slot of the
// LAST one that covers a pixel, so walk backwards and stop at the first hit.  0 where nothing covers and outside the image's (h, w).
template <bool COLS>
__global__ __launch_bounds__(256) void rle_ground_truth_kernel(const int* __restrict__ ends, const int* __restrict__ meta,
                                                               const int* __restrict__ first, const int* __restrict__ count,
                                                               const int* __restrict__ index, const int* __restrict__ img_hw, int Hmax,
                                                               int Wmax, long long* __restrict__ out) {
  __shared__ unsigned char tile[64][68];
  const int img = blockIdx.y;
  const int f = first[img], cnt = count[img];
  const int H = img_hw[2 * img], W = img_hw[2 * img + 1];
  const int tw = (Wmax + 63) >> 6;
  long long* o = out + (size_t)img * Hmax * Wmax;
  rle_tile64<COLS>(tile, Hmax, Wmax, blockIdx.x / tw, blockIdx.x % tw,
             [&](int y, int x) {
               if (y >= H || x >= W) return (unsigned char)0;
               const int pos = x * H + y;
               for (int k = cnt - 1; k >= 0; --k) {
                 const int* m = meta + (size_t)index[f + k] * RLE_META;
                 if (rle_run_of(ends + m[0], m[1], pos) & 1) return (unsigned char)m[5];
               }
               return (unsigned char)0;
             },
             [&](int y, int x, unsigned char v) { o[(size_t)y * Wmax + x] = (long long)v; });
}

// PromptsProcessor.sample_point + apply_coords (data/transforms.py:152-174): one wave per draw (annotation, rank, destination).
// The rank-th set pixel in row-major order, from column-major runs, without a dense mask: a 1-run [s, e) holds
//   R(e) - R(s) pixels in rows < y,            R(p) = (p / h) * y + min(p % h, y)
//   Q(e) - Q(s) pixels of row y in columns < x, Q(p) = min(x, p > y ? (p - y + h - 1) / h : 0)
// so both the row (smallest y with more than `rank` set pixels in rows <= y) and then the column are found by bisection, every probe
// one strided pass of the wave over the annotation's 1-runs and an integer wave sum.  All counts are < h * w < 2^31.
// points fp32 [.., 2] = (x * (new_w / w), y * (new_h / h)), ratio and product in fp64, rounded to fp32 once; flags u8 = 1.
__global__ __launch_bounds__(256) void rle_points_kernel(const int* __restrict__ ends, const int* __restrict__ meta, const int* __restrict__ area,
                                                         const int* __restrict__ new_hw, const int* __restrict__ draws, int D,
                                                         float* __restrict__ points, unsigned char* __restrict__ flags) {
  const int d = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (d >= D) return;
  const int* m = meta + (size_t)draws[3 * d] * RLE_META;
  const int* e = ends + m[0];
  const int n = m[1], h = m[2], w = m[3], img = m[4];
  const int rank = min(max(draws[3 * d + 1], 0), area[draws[3 * d]] - 1);      // the host never packs an annotation without a set pixel
  const int dst = draws[3 * d + 2];
  auto rows_below = [&](int y) {
    int s = 0;
    for (int i = 1 + 2 * lane; i < n; i += 128) {
      const int a = e[i - 1], b = e[i];
      s += (b / h) * y + min(b % h, y) - (a / h) * y - min(a % h, y);
    }
    return wave_sum_i32(s);
  };
  int lo = 0, hi = h - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rows_below(mid + 1) > rank) hi = mid;
    else lo = mid + 1;
  }
  const int y = lo;
  const int rem = rank - rows_below(y);
  auto cols_before = [&](int x) {
    int s = 0;
    for (int i = 1 + 2 * lane; i < n; i += 128) {
      const int a = e[i - 1], b = e[i];
      s += min(x, b > y ? (b - y + h - 1) / h : 0) - min(x, a > y ? (a - y + h - 1) / h : 0);
    }
    return wave_sum_i32(s);
  };
  lo = 0, hi = w - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cols_before(mid + 1) > rem) hi = mid;
    else lo = mid + 1;
  }
  if (lane == 0) {
    points[2 * (size_t)dst] = (float)((double)lo * ((double)new_hw[2 * img + 1] / (double)w));
    points[2 * (size_t)dst + 1] = (float)((double)y * ((double)new_hw[2 * img] / (double)h));
    flags[dst] = 1;
  }
}

// measurement library only: LA_RLE_ROW_LANES=1 selects the plain thread mapping of the tiled kernels (same results)
#ifdef LA_DEBUG
#define LA_RLE_LAUNCH(kernel, grid, ...)                                                                                   \
  do {                                                                                                                     \
    const char* _e = la_dbg_env("LA_RLE_ROW_LANES");                                                                       \
    if (_e && _e[0] == '1') hipLaunchKernelGGL(kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);       \
    else hipLaunchKernelGGL(kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__);                           \
  } while (0)
#else
#define LA_RLE_LAUNCH(kernel, grid, ...) hipLaunchKernelGGL(kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, __VA_ARGS__)
#endif

}  // namespace la

extern "C" int la_rle_scan(const int* runs, const int* meta, int K, int* ends, int* area, void* stream) {
  LA_CHECK_ARG(runs && meta && ends && area, "la_rle_scan: null pointer");
  LA_CHECK_ARG(K > 0, "la_rle_scan: no annotations");
  hipLaunchKernelGGL(la::rle_scan_kernel, dim3((K + 3) / 4), dim3(256), 0, (hipStream_t)stream, runs, meta, K, ends, area);
  LA_CHECK_LAUNCH("la_rle_scan");
  return 0;
}

extern "C" int la_rle_decode(const int* ends, const int* meta, const int* sel, int k, int H, int W, unsigned char* out, void* stream) {
  LA_CHECK_ARG(ends && meta && sel && out, "la_rle_decode: null pointer");
  LA_CHECK_ARG(k > 0 && k <= 65535 && H > 0 && W > 0 && (long)H * W < (1L << 31), "la_rle_decode: bad shape (k %d, %d x %d)", k, H, W);
  const int tiles = ((H + 63) / 64) * ((W + 63) / 64);
  LA_RLE_LAUNCH(la::rle_decode_kernel, dim3(tiles, k), ends, meta, sel, H, W, out);
  LA_CHECK_LAUNCH("la_rle_decode");
  return 0;
}

extern "C" int la_rle_prompt_masks(const int* ends, const int* meta, const int* first, const int* count, const int* index, const int* img_hw,
                                   const int* new_hw, int N, int C, int custom, int S, int Mo, float* out, unsigned char* flags,
                                   void* stream) {
  LA_CHECK_ARG(ends && meta && first && count && index && img_hw && new_hw && out && flags, "la_rle_prompt_masks: null pointer");
  LA_CHECK_ARG(N > 0 && C > 0 && (long)N * C <= 65535 && S > 0 && Mo > 0 && Mo <= 4096, "la_rle_prompt_masks: bad geometry (N %d, C %d, S %d, Mo %d)",
               N, C, S, Mo);
  const int t = (Mo + 63) / 64;
  LA_RLE_LAUNCH(la::rle_prompt_mask_kernel, dim3(t * t, N * C), ends, meta, first, count, index, img_hw,
                     new_hw, C, custom, S, Mo, out, flags);
  LA_CHECK_LAUNCH("la_rle_prompt_masks");
  return 0;
}

extern "C" int la_rle_ground_truth(const int* ends, const int* meta, const int* first, const int* count, const int* index, const int* img_hw,
                                   int N, int Hmax, int Wmax, long long* out, void* stream) {
  LA_CHECK_ARG(ends && meta && first && count && index && img_hw && out, "la_rle_ground_truth: null pointer");
  LA_CHECK_ARG(N > 0 && N <= 65535 && Hmax > 0 && Wmax > 0 && (long)Hmax * Wmax < (1L << 31), "la_rle_ground_truth: bad shape (N %d, %d x %d)", N,
               Hmax, Wmax);
  const int tiles = ((Hmax + 63) / 64) * ((Wmax + 63) / 64);
  LA_RLE_LAUNCH(la::rle_ground_truth_kernel, dim3(tiles, N), ends, meta, first, count, index, img_hw,
                     Hmax, Wmax, out);
  LA_CHECK_LAUNCH("la_rle_ground_truth");
  return 0;
}

extern "C" int la_rle_points(const int* ends, const int* meta, const int* area, const int* new_hw, const int* draws, int D, float* points,
                             unsigned char* flags, void* stream) {
  LA_CHECK_ARG(ends && meta && area && new_hw && draws && points && flags, "la_rle_points: null pointer");
  LA_CHECK_ARG(D > 0, "la_rle_points: no draws");
  hipLaunchKernelGGL(la::rle_points_kernel, dim3((D + 3) / 4), dim3(256), 0, (hipStream_t)stream, ends, meta, area, new_hw, draws, D, points, flags);
  LA_CHECK_LAUNCH("la_rle_points");
  return 0;
}
