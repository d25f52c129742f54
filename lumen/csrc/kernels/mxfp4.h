// In-register MXFP4 -> 16-bit conversion shared by kernels/w4a8_gemm.hip (w4_dequant) and
// kernels/w4a16_gemm.hip: an E8M0 block-scale byte as f32, and v_cvt_scalef32_pk_{bf16,f16}_fp4,
// which turns one code byte (two e2m1 codes, the low nibble first) times that scale into one
// packed 16-bit pair, rounded once (exact in bf16).
#pragma once
#include "common.h"

namespace lumen {
namespace mx {

// 2^(e - 127) as f32: the byte is the exponent field (byte 0: the subnormal 2^-127)
__device__ __forceinline__ float e8m0_f32(unsigned e) {
  return __builtin_bit_cast(float, e ? e << 23 : 0x00400000u);
}

// the two e2m1 codes of byte B of v times s -> one packed 16-bit pair, exact
template <typename T, int B> __device__ __forceinline__ unsigned cvt2(unsigned v, float s);
#define LUMEN_W4_CVT(B)                                                                         \
  template <> __device__ __forceinline__ unsigned cvt2<bf16, B>(unsigned v, float s) {          \
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, s, B));    \
  }                                                                                             \
  template <> __device__ __forceinline__ unsigned cvt2<fp16, B>(unsigned v, float s) {          \
    return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(v, s, B));     \
  }
LUMEN_W4_CVT(0) LUMEN_W4_CVT(1) LUMEN_W4_CVT(2) LUMEN_W4_CVT(3)
#undef LUMEN_W4_CVT

// one code word (8 consecutive k) times s -> 8 16-bit elements in k order
template <typename T>
__device__ __forceinline__ uint4 cvt8(unsigned v, float s) {
  return make_uint4(cvt2<T, 0>(v, s), cvt2<T, 1>(v, s), cvt2<T, 2>(v, s), cvt2<T, 3>(v, s));
}

// one code word (8 consecutive elements) times s -> 8 f32, exact (v_cvt_scalef32_pk_f32_fp4)
__device__ __forceinline__ void cvt8f(unsigned v, float s, float (&o)[8]) {
  const auto a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, s, 0);
  const auto b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, s, 1);
  const auto c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, s, 2);
  const auto d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, s, 3);
  o[0] = a[0]; o[1] = a[1]; o[2] = b[0]; o[3] = b[1];
  o[4] = c[0]; o[5] = c[1]; o[6] = d[0]; o[7] = d[1];
}

// ---- the quantizer (ops/quant.py quantize_mxfp4_rows, bit for bit) -----------------------------
// Biased E8M0 byte of a block whose largest magnitude is amax (finite, >= 0): e = floor(log2
// amax) - 2 from the f32 exponent field, clamped below at -127; 127 for an all-zero block.
__device__ __forceinline__ unsigned scale_byte(float amax) {
  const int E = static_cast<int>(__builtin_bit_cast(unsigned, amax) >> 23) - 2;
  return amax > 0.f ? static_cast<unsigned>(E < 0 ? 0 : E) : 127u;
}

// e2m1 code of x under the block byte e: |x| 2^-(e-127) clamped at 6, rounded to the nearest grid
// point with ties to the even code (the grid's step is 0.5 below 2, 1 below 4, 2 above, and
// round-half-even in each range lands on the even code); no negative zero.  Every step is exact
// in f32: the multiplier 2^(127-e) has exponent field 254 - e in [2, 254].
__device__ __forceinline__ unsigned encode1(float x, unsigned e) {
  const float inv = __builtin_bit_cast(float, (254u - e) << 23);
  const float a = fminf(fabsf(x) * inv, 6.f);
  const float v = a < 2.f ? rintf(a * 2.f) * 0.5f : (a < 4.f ? rintf(a) : rintf(a * 0.5f) * 2.f);
  const unsigned c = static_cast<unsigned>(v < 2.f ? v * 2.f : (v < 4.f ? v + 2.f : v * 0.5f + 4.f));
  return c | ((x < 0.f && c != 0u) ? 8u : 0u);
}

// 8 consecutive elements -> one code word, the even element in the low nibble of each byte
__device__ __forceinline__ unsigned encode8(const float (&v)[8], unsigned e) {
  unsigned w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) w |= encode1(v[j], e) << (4 * j);
  return w;
}

}  // namespace mx
}  // namespace lumen
