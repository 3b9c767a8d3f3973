// Rotary position embedding of the q and k columns of a packed q | k | v buffer (DINOv3 ViT: transformers DINOv3ViTAttention /
// apply_rotary_pos_emb), in place.  One pass over the q | k columns of the patch rows: rows x 2 ea x 2 bytes read and written, nothing
// else touched - prefix rows (CLS + registers), the padded columns of a head and the v block keep their bits because no thread
// addresses them.  A thread owns 8 consecutive columns of the first half of a head and the 8 that pair with them in the second half:
// two 16-byte loads, four 32-byte table reads (L2 resident: the table is [hw, hd] fp32 twice), fp32 arithmetic, two 16-byte stores.
#include "la_common.h"
#include "../../include/la_hip.h"

namespace la {

template <typename T>
__global__ __launch_bounds__(256) void rope_qk_kernel(T* __restrict__ qkv, long total, int ld, int tokens, int prefix, int heads, int hd,
                                                      int hdp, const float* __restrict__ cosw, const float* __restrict__ sinw) {
  const int half = hd >> 1, chunks = hd >> 4;
  const int items = 2 * heads * chunks;          // 8-column pairs per row: (q | k) x heads x chunks
  const int hw = tokens - prefix;
  const long ea = (long)heads * hdp;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int item = (int)(i % items);
    const long pr = i / items;                   // patch row, prefix rows not counted
    const long img = pr / hw;
    const int pos = (int)(pr - img * hw);
    const int c = item % chunks, hh = item / chunks;
    const int blk = hh / heads, h = hh - blk * heads;
    T* p = qkv + (img * tokens + prefix + pos) * (long)ld + blk * ea + (long)h * hdp + c * 8;
    const uint4 a = *reinterpret_cast<const uint4*>(p);
    const uint4 b = *reinterpret_cast<const uint4*>(p + half);
    const long tb = (long)pos * hd + c * 8;
    const float4* c1 = reinterpret_cast<const float4*>(cosw + tb);
    const float4* s1 = reinterpret_cast<const float4*>(sinw + tb);
    const float4* c2 = reinterpret_cast<const float4*>(cosw + tb + half);
    const float4* s2 = reinterpret_cast<const float4*>(sinw + tb + half);
    const float4 cv1[2] = {c1[0], c1[1]}, sv1[2] = {s1[0], s1[1]}, cv2[2] = {c2[0], c2[1]}, sv2[2] = {s2[0], s2[1]};
    const float* fc1 = reinterpret_cast<const float*>(cv1);
    const float* fs1 = reinterpret_cast<const float*>(sv1);
    const float* fc2 = reinterpret_cast<const float*>(cv2);
    const float* fs2 = reinterpret_cast<const float*>(sv2);
    const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
    uint32_t oa[4], ob[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x1l = unpack_lo<T>(aw[j]), x1h = unpack_hi<T>(aw[j]);
      const float x2l = unpack_lo<T>(bw[j]), x2h = unpack_hi<T>(bw[j]);
      // x cos + (-x2 | x1) sin
      oa[j] = pack2<T>(x1l * fc1[2 * j] - x2l * fs1[2 * j], x1h * fc1[2 * j + 1] - x2h * fs1[2 * j + 1]);
      ob[j] = pack2<T>(x2l * fc2[2 * j] + x1l * fs2[2 * j], x2h * fc2[2 * j + 1] + x1h * fs2[2 * j + 1]);
    }
    *reinterpret_cast<uint4*>(p) = make_uint4(oa[0], oa[1], oa[2], oa[3]);
    *reinterpret_cast<uint4*>(p + half) = make_uint4(ob[0], ob[1], ob[2], ob[3]);
  }
}

}  // namespace la

extern "C" int la_rope_qk(void* qkv, long rows, int ld, int tokens, int prefix, int heads, int hd, int hdp, const float* cosw,
                          const float* sinw, int dt, void* stream) {
  LA_CHECK_ARG(qkv && cosw && sinw, "la_rope_qk: null pointer");
  LA_CHECK_ARG(dt == LA_F16 || dt == LA_BF16, "la_rope_qk: bad dtype %d", dt);
  LA_CHECK_ARG(rows > 0 && tokens > 0 && prefix >= 0 && prefix < tokens && rows % tokens == 0,
               "la_rope_qk: rows=%ld must be whole images of tokens=%d, prefix=%d of them not rotated", rows, tokens, prefix);
  LA_CHECK_ARG(heads > 0 && hd > 0 && (hd % 16) == 0 && hdp >= hd && (hdp % 8) == 0,
               "la_rope_qk: head width %d (padded %d) must be a multiple of 16 inside a multiple of 8", hd, hdp);
  LA_CHECK_ARG((long)ld >= 3l * heads * hdp && (ld % 8) == 0, "la_rope_qk: ld=%d must cover 3 x %d x %d columns and be a multiple of 8", ld,
               heads, hdp);
  LA_CHECK_ARG(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)cosw & 15) == 0 && ((uintptr_t)sinw & 15) == 0,
               "la_rope_qk: qkv and the tables must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const long total = rows / tokens * (tokens - prefix) * (2l * heads * (hd / 16));
  const long nb = (total + 255) / 256;
  const dim3 grid((unsigned)(nb > 65536 ? 65536 : nb)), blk(256);
  if (dt == LA_F16)
    hipLaunchKernelGGL(la::rope_qk_kernel<la::f16_t>, grid, blk, 0, st, (la::f16_t*)qkv, total, ld, tokens, prefix, heads, hd, hdp, cosw, sinw);
  else
    hipLaunchKernelGGL(la::rope_qk_kernel<la::bf16_t>, grid, blk, 0, st, (la::bf16_t*)qkv, total, ld, tokens, prefix, heads, hd, hdp, cosw, sinw);
  LA_CHECK_LAUNCH("la_rope_qk");
  return 0;
}
