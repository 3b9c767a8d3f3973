// What extract.hip (forward, folding) and extract_bwd.hip (their backward) share: the exact-fp32 MFMA step, the head count and the
// argument checks common to every entry point of the embedding extraction.
#pragma once
#include "la_common.h"

#include <cstdint>

namespace la {

// MFMA 16x16x4 f32 operand layout (lane l, q = l / 16, n = l % 16): A[row n][k q], B[k q][col n], D register r = [row 4 q + r][col n].
__device__ __forceinline__ f32x4 ex_mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float ex_comp(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

constexpr int EX_HEADS = 8;

}  // namespace la

static inline bool ex_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static inline bool extract_sizes_ok(const char* who, int D, int n) {
  if (D != 64 && D != 128 && D != 256) {
    la_set_error("%s: D=%d must be 64, 128 or 256", who, D);
    return false;
  }
  if (n < 1 || n > 16) {
    la_set_error("%s: n=%d queries per pair must be 1..16", who, n);
    return false;
  }
  return true;
}
