// The same 32 x 32 x K product on the two 16-bit MFMA shapes of gfx950, K ascending in 64-deep tiles as the GEMM main loops walk it:
//   shape 0: v_mfma_f32_32x32x16 - one accumulator block, four k-steps of 16 per tile (what every la_gemm kernel issues)
//   shape 1: v_mfma_f32_16x16x32 - 2 x 2 accumulator blocks, two k-steps of 32 per tile
// One wave, operands straight from global memory: the only question is whether the two shapes ROUND alike
// (tests/test_mfma_shape_gpu.py), which decides whether a main loop may change shape without moving results.
#include "la_common.h"
#include "../../include/la_hip.h"

namespace la {

template <typename T> struct Mfma16;
template <> struct Mfma16<f16_t> {
  static __device__ __forceinline__ f32x4 go(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8_t, a), __builtin_bit_cast(h8_t, b), c, 0, 0, 0);
  }
};
template <> struct Mfma16<bf16_t> {
  static __device__ __forceinline__ f32x4 go(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(b8_t, a), __builtin_bit_cast(b8_t, b), c, 0, 0, 0);
  }
};

template <typename T, int SHAPE>
__global__ __launch_bounds__(64) void mfma_shape_kernel(const T* __restrict__ A, const T* __restrict__ W, float* __restrict__ out, int K) {
  const int lane = threadIdx.x;
  if constexpr (SHAPE == 0) {
    const int fr = lane & 31, fh = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += 64)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const size_t o = (size_t)fr * K + k0 + ks * 16 + fh * 8;
        acc = Half16<T>::mfma32(*reinterpret_cast<const uint4*>(A + o), *reinterpret_cast<const uint4*>(W + o), acc);
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) out[((r & 3) + 8 * (r >> 2) + 4 * fh) * 32 + fr] = acc[r];
  } else {
    const int r16 = lane & 15, q = lane >> 4;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 64)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        uint4 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const size_t o = (size_t)(16 * i + r16) * K + k0 + ks * 32 + q * 8;
          a[i] = *reinterpret_cast<const uint4*>(A + o);
          b[i] = *reinterpret_cast<const uint4*>(W + o);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = Mfma16<T>::go(a[i], b[j], acc[i][j]);
      }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(16 * i + 4 * q + r) * 32 + 16 * j + r16] = acc[i][j][r];
  }
}

}  // namespace la

extern "C" int la_mfma_shape_probe(const void* A, const void* W, float* out, int K, int dt, int shape, void* stream) {
  LA_CHECK_ARG(A && W && out, "la_mfma_shape_probe: null pointer");
  LA_CHECK_ARG(K > 0 && (K % 64) == 0, "la_mfma_shape_probe: K=%d must be a positive multiple of 64", K);
  LA_CHECK_ARG((dt == LA_F16 || dt == LA_BF16) && (shape == 0 || shape == 1), "la_mfma_shape_probe: dt=%d must be 16-bit, shape=%d 0 or 1", dt, shape);
  LA_CHECK_ARG((((uintptr_t)A | (uintptr_t)W) & 15) == 0, "la_mfma_shape_probe: operands must be 16-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  using namespace la;
  if (dt == LA_F16) {
    if (shape == 0) mfma_shape_kernel<f16_t, 0><<<1, 64, 0, s>>>((const f16_t*)A, (const f16_t*)W, out, K);
    else mfma_shape_kernel<f16_t, 1><<<1, 64, 0, s>>>((const f16_t*)A, (const f16_t*)W, out, K);
  } else {
    if (shape == 0) mfma_shape_kernel<bf16_t, 0><<<1, 64, 0, s>>>((const bf16_t*)A, (const bf16_t*)W, out, K);
    else mfma_shape_kernel<bf16_t, 1><<<1, 64, 0, s>>>((const bf16_t*)A, (const bf16_t*)W, out, K);
  }
  LA_CHECK_LAUNCH("la_mfma_shape_probe");
  return 0;
}
