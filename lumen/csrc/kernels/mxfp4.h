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

}  // namespace mx
}  // namespace lumen
