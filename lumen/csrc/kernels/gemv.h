// VALU pieces of the rows-per-lane GEMVs (kernels/skinny_gemm.hip, w8_gemm.hip, w8a8_gemm.hip,
// w4a16_gemm.hip): the packed 16-bit dot product, the DPP row sum, and the exact in-register
// e4m3fn -> 16-bit conversion of the fp8 weights (the MXFP4 one is kernels/mxfp4.h's).
#pragma once
#include "common.h"

namespace lumen {
namespace gemv {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// c + a.lo * b.lo + a.hi * b.hi on packed 16-bit pairs, f32 accumulation
template <typename T> __device__ __forceinline__ float dot2(unsigned a, unsigned b, float c);
template <> __device__ __forceinline__ float dot2<bf16>(unsigned a, unsigned b, float c) {
  return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a),
                                         __builtin_bit_cast(bf16x2, b), c, false);
}
template <> __device__ __forceinline__ float dot2<fp16>(unsigned a, unsigned b, float c) {
  return __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, b), c,
                                false);
}

template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL,
                                                               0xF, 0xF, false));
}
__device__ __forceinline__ float sum16(float v) {  // over the 16 lanes of a DPP row
  v += dppf<0xB1>(v);
  v += dppf<0x4E>(v);
  v += dppf<0x141>(v);
  v += dppf<0x140>(v);
  return v;
}

// two e4m3fn bytes of v (HI: bytes 2, 3; else bytes 0, 1) -> one packed 16-bit pair, exact
template <typename T, bool HI> __device__ __forceinline__ unsigned cvt2(unsigned v);
template <> __device__ __forceinline__ unsigned cvt2<bf16, false>(unsigned v) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, false));
}
template <> __device__ __forceinline__ unsigned cvt2<bf16, true>(unsigned v) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.0f, true));
}
template <> __device__ __forceinline__ unsigned cvt2<fp16, false>(unsigned v) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, 1.0f, false));
}
template <> __device__ __forceinline__ unsigned cvt2<fp16, true>(unsigned v) {
  return __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(v, 1.0f, true));
}

// 8 e4m3fn bytes (a: elements 0..3, b: 4..7) -> 8 16-bit elements
template <typename T>
__device__ __forceinline__ uint4 cvt8(unsigned a, unsigned b) {
  return make_uint4(cvt2<T, false>(a), cvt2<T, true>(a), cvt2<T, false>(b), cvt2<T, true>(b));
}

}  // namespace gemv
}  // namespace lumen
