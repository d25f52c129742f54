// Dequantisers of a quantized frozen base for training (--base_quantization fp8 | mxfp4).
//
// The frozen projections are stored once, as ops/quant.py's QuantWeight (e4m3fn + one f32 scale
// per output row) or Mxfp4Weight (two e2m1 codes per byte + one E8M0 scale per 32 k), and turned
// into the 16-bit operand of the (unchanged) hipBLASLt GEMMs right before each use:
//
//  * qbase_dequant    [N, K] codes -> 16-bit rows at row stride ld >= K; columns K..ld are never
//                     written.  The forward's weight and the NN backward's.
//  * qbase_dequant_t  [N, K] codes -> contiguous 16-bit [K, N] = dequant()^T: the TN input-gradient
//                     GEMM's operand straight from the quantized storage (no resident W^T, no
//                     separate transpose pass).
//
// Both are bit-identical to the holders' dequant(): fp8 is f32(q) * scale in f32 and ONE rounding
// to the output type (w8_gemm.hip's w8_dequant arithmetic; v_cvt_scalef32_pk_*_fp8 is exact only
// for the unscaled conversion, which is not what dequant() computes), MXFP4 is mxfp4.h's
// v_cvt_scalef32_pk_*_fp4.  K % 16 == 0 and N % 8 == 0; every load and store is bounded by N and K.
#include "api.h"
#include "common.h"
#include "mxfp4.h"

namespace lumen {
namespace qbase {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// 4 e4m3fn bytes times s -> two packed 16-bit pairs (elements 0, 1 and 2, 3)
template <typename T>
__device__ __forceinline__ void fp8x4(unsigned w, float s, unsigned& o0, unsigned& o1) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  o0 = pk2<T>(lo[0] * s, lo[1] * s);
  o1 = pk2<T>(hi[0] * s, hi[1] * s);
}

// ---- row-major ----------------------------------------------------------------------------------
// fp8: thread = one 16-byte chunk (16 k) of one row: one 16-byte load, two 16-byte stores
template <typename T>
__global__ void __launch_bounds__(256)
dequant_fp8_kernel(const unsigned char* __restrict__ q, const float* __restrict__ scale,
                   T* __restrict__ out, long long chunks, int kchunks, long long ld) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  const long long n = c / kchunks;
  const int kc = (int)(c - n * kchunks);
  const float s = scale[n];
  const uint4 w = *reinterpret_cast<const uint4*>(q + c * 16);
  unsigned o[8];
  fp8x4<T>(w.x, s, o[0], o[1]);
  fp8x4<T>(w.y, s, o[2], o[3]);
  fp8x4<T>(w.z, s, o[4], o[5]);
  fp8x4<T>(w.w, s, o[6], o[7]);
  uint4* op = reinterpret_cast<uint4*>(out + n * ld + 16 * kc);
  op[0] = make_uint4(o[0], o[1], o[2], o[3]);
  op[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

// MXFP4: thread = one code word (8 k) of one row: a wave stores 1 KiB contiguous.  Only words
// below K are touched, so the padded half of a last block (K % 32 == 16) is neither read nor
// written.
template <typename T>
__global__ void __launch_bounds__(256)
dequant_mx_kernel(const unsigned char* __restrict__ q, const unsigned char* __restrict__ scale,
                  T* __restrict__ out, long long N, int K, long long ld) {
  const int c8 = K >> 3, KB = (K + 31) >> 5;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * c8) return;
  const long long n = idx / c8;
  const int c = (int)(idx - n * c8);
  const unsigned v = *reinterpret_cast<const unsigned*>(q + n * (16LL * KB) + 4 * c);
  const float s = mx::e8m0_f32(scale[n * KB + (c >> 2)]);
  *reinterpret_cast<uint4*>(out + n * ld + 8 * c) = mx::cvt8<T>(v, s);
}

// ---- transposed ---------------------------------------------------------------------------------
// Workgroup = a tile of TN = 128 rows (n) x TK = 128 columns (k) of the weight.  A thread loads
// one 16-byte chunk of q from each of the two rows of an n pair (the chunks of a row are read by
// adjacent lanes: 128 bytes of fp8, 64 bytes of MXFP4 codes per row and tile), converts, and
// interleaves the two rows in registers, so that what goes to LDS is one dword {w[n][k],
// w[n + 1][k]} per k: the LDS image is already [k][n] (32 KiB, 64 dwords per k row), written with
// ds_write_b32 and read back with ds_read_b128 for the 16-byte stores along n (a k row of the
// tile = 256 contiguous bytes of out, written by 16 adjacent lanes).
//
// Banks.  A store instruction's 32-lane group holds every chunk c of a row and a few adjacent n
// pairs; its dwords are 16 (fp8) or 32 (MXFP4) k rows apart, i.e. on the same bank in a plain
// image.  The image is therefore swizzled: dword column P of k row k lives at P ^ (((k >> 4) &
// 7) << 2).  In a group the low bits of P are the pair, the bits above them fixed, and the XOR
// puts the chunk there: 32 distinct banks.  The XOR moves whole aligned groups of 4 dwords, so
// the 16-byte reads stay aligned and contiguous, and 16 adjacent lanes read one whole k row.
constexpr int TN = 128, TK = 128, TD = TN / 2;  // TD: dwords per k row of the image

__device__ __forceinline__ int swz(int k, int P) { return k * TD + (P ^ (((k >> 4) & 7) << 2)); }

// a, b: packed 16-bit pairs (k, k + 1) of rows n and n + 1 -> the image's dwords of k and k + 1
__device__ __forceinline__ void put2(unsigned* tile, int k, int P, unsigned a, unsigned b) {
  tile[swz(k, P)] = (a & 0xffffu) | (b << 16);
  tile[swz(k + 1, P)] = (a >> 16) | (b & 0xffff0000u);
}

// image -> out[k0 + k][n0 ...]: 16 chunks of 8 n per k row, 16 k rows per pass
template <typename T>
__device__ __forceinline__ void store_tile(const unsigned* tile, T* __restrict__ out, long long N,
                                           int K, long long n0, int k0) {
  const int g = threadIdx.x & 15, kr = threadIdx.x >> 4;
  const long long n = n0 + 8 * g;
#pragma unroll
  for (int i = 0; i < TK / 16; ++i) {
    const int k = 16 * i + kr;
    // N % 8 == 0: a chunk of 8 n is inside or outside as a whole
    if (k0 + k < K && n < N)
      *reinterpret_cast<uint4*>(out + (long long)(k0 + k) * N + n) =
          *reinterpret_cast<const uint4*>(tile + swz(k, 4 * g));
  }
}

template <typename T>
__global__ void __launch_bounds__(256)
dequant_t_fp8_kernel(const unsigned char* __restrict__ q, const float* __restrict__ scale,
                     T* __restrict__ out, long long N, int K) {
  __shared__ __attribute__((aligned(16))) unsigned tile[TK * TD];
  const long long n0 = (long long)blockIdx.x * TN;
  const int k0 = blockIdx.y * TK;
  const int c = threadIdx.x & 7;  // 16-byte chunk = 16 k
  const int kq = k0 + 16 * c;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int P = 32 * i + (threadIdx.x >> 3);
    const long long n = n0 + 2 * P;
    uint4 wa = make_uint4(0, 0, 0, 0), wb = wa;
    float sa = 0.f, sb = 0.f;
    if (n < N && kq < K) {  // N % 8 == 0: the pair's second row exists; K % 16 == 0: whole chunks
      wa = *reinterpret_cast<const uint4*>(q + n * K + kq);
      wb = *reinterpret_cast<const uint4*>(q + (n + 1) * K + kq);
      sa = scale[n];
      sb = scale[n + 1];
    }
    const unsigned va[4] = {wa.x, wa.y, wa.z, wa.w}, vb[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      unsigned a0, a1, b0, b1;
      fp8x4<T>(va[j], sa, a0, a1);
      fp8x4<T>(vb[j], sb, b0, b1);
      put2(tile, 16 * c + 4 * j, P, a0, b0);
      put2(tile, 16 * c + 4 * j + 2, P, a1, b1);
    }
  }
  __syncthreads();
  store_tile<T>(tile, out, N, K, n0, k0);
}

// a 16-byte chunk of codes is one MX block (32 k) with one scale byte; rows are padded to whole
// blocks in storage, so a block below KB is read whole, and the k rows of its padded half
// (K % 32 == 16) are left out by store_tile's k < K
template <typename T>
__global__ void __launch_bounds__(256)
dequant_t_mx_kernel(const unsigned char* __restrict__ q, const unsigned char* __restrict__ scale,
                    T* __restrict__ out, long long N, int K) {
  __shared__ __attribute__((aligned(16))) unsigned tile[TK * TD];
  const int KB = (K + 31) >> 5;
  const long long n0 = (long long)blockIdx.x * TN;
  const int k0 = blockIdx.y * TK;
  const int c = threadIdx.x & 3;  // 16-byte chunk = 32 k
  const int kb = (k0 >> 5) + c;
  const int P = threadIdx.x >> 2;
  const long long n = n0 + 2 * P;
  uint4 wa = make_uint4(0, 0, 0, 0), wb = wa;
  float sa = 0.f, sb = 0.f;
  if (n < N && kb < KB) {
    wa = *reinterpret_cast<const uint4*>(q + (n * KB + kb) * 16);
    wb = *reinterpret_cast<const uint4*>(q + ((n + 1) * KB + kb) * 16);
    sa = mx::e8m0_f32(scale[n * KB + kb]);
    sb = mx::e8m0_f32(scale[(n + 1) * KB + kb]);
  }
  const unsigned va[4] = {wa.x, wa.y, wa.z, wa.w}, vb[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint4 a = mx::cvt8<T>(va[j], sa), b = mx::cvt8<T>(vb[j], sb);
    const int k = 32 * c + 8 * j;
    put2(tile, k, P, a.x, b.x);
    put2(tile, k + 2, P, a.y, b.y);
    put2(tile, k + 4, P, a.z, b.z);
    put2(tile, k + 6, P, a.w, b.w);
  }
  __syncthreads();
  store_tile<T>(tile, out, N, K, n0, k0);
}

}  // namespace qbase
}  // namespace lumen

namespace {
inline bool qb_misaligned16(const void* a, const void* b) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) != 0;
}
// fmt 0: fp8 (scale f32 [N]), 1: MXFP4 (scale uint8 [N, ceil(K / 32)])
inline bool qb_bad(int fmt, const void* q, const void* scale, const void* out, long long N,
                   long long K) {
  return (fmt != 0 && fmt != 1) || N < 8 || N % 8 != 0 || K < 16 || K % 16 != 0 ||
         K > 0x7fffffffLL || N > 0x7fffffffLL || scale == nullptr || qb_misaligned16(q, out) ||
         (fmt == 0 && (reinterpret_cast<uintptr_t>(scale) & 3) != 0);
}
}  // namespace

// out[n * ld + k] (16-bit) = dequant(q, scale)[n, k] for k < K; N % 8 == 0, K % 16 == 0,
// ld >= K, ld % 8 == 0, 16-byte aligned q and out
extern "C" hipError_t lumen_qbase_dequant(int fmt, int dtype, const void* q, const void* scale,
                                          void* out, long long N, long long K, long long ld,
                                          hipStream_t st) {
  using namespace lumen;
  if (qb_bad(fmt, q, scale, out, N, K) || ld < K || ld % 8 != 0) return hipErrorInvalidValue;
  if (dtype != kBF16 && dtype != kF16) return hipErrorInvalidValue;
  const long long items = N * (fmt == 0 ? K / 16 : K / 8);
  const long long blocks = (items + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  dim3 grid((unsigned)blocks), block(256);
  const unsigned char* qp = (const unsigned char*)q;
  if (fmt == 0) {
    if (dtype == kBF16)
      hipLaunchKernelGGL(qbase::dequant_fp8_kernel<bf16>, grid, block, 0, st, qp,
                         (const float*)scale, (bf16*)out, items, (int)(K / 16), ld);
    else
      hipLaunchKernelGGL(qbase::dequant_fp8_kernel<fp16>, grid, block, 0, st, qp,
                         (const float*)scale, (fp16*)out, items, (int)(K / 16), ld);
  } else {
    if (dtype == kBF16)
      hipLaunchKernelGGL(qbase::dequant_mx_kernel<bf16>, grid, block, 0, st, qp,
                         (const unsigned char*)scale, (bf16*)out, N, (int)K, ld);
    else
      hipLaunchKernelGGL(qbase::dequant_mx_kernel<fp16>, grid, block, 0, st, qp,
                         (const unsigned char*)scale, (fp16*)out, N, (int)K, ld);
  }
  return hipGetLastError();
}

// out [K, N] (16-bit, contiguous) = dequant(q, scale)^T; same constraints
extern "C" hipError_t lumen_qbase_dequant_t(int fmt, int dtype, const void* q, const void* scale,
                                            void* out, long long N, long long K, hipStream_t st) {
  using namespace lumen;
  if (qb_bad(fmt, q, scale, out, N, K)) return hipErrorInvalidValue;
  if (dtype != kBF16 && dtype != kF16) return hipErrorInvalidValue;
  const long long gx = (N + qbase::TN - 1) / qbase::TN, gy = (K + qbase::TK - 1) / qbase::TK;
  if (gy > 65535) return hipErrorInvalidValue;
  dim3 grid((unsigned)gx, (unsigned)gy), block(256);
  const unsigned char* qp = (const unsigned char*)q;
  if (fmt == 0) {
    if (dtype == kBF16)
      hipLaunchKernelGGL(qbase::dequant_t_fp8_kernel<bf16>, grid, block, 0, st, qp,
                         (const float*)scale, (bf16*)out, N, (int)K);
    else
      hipLaunchKernelGGL(qbase::dequant_t_fp8_kernel<fp16>, grid, block, 0, st, qp,
                         (const float*)scale, (fp16*)out, N, (int)K);
  } else {
    if (dtype == kBF16)
      hipLaunchKernelGGL(qbase::dequant_t_mx_kernel<bf16>, grid, block, 0, st, qp,
                         (const unsigned char*)scale, (bf16*)out, N, (int)K);
    else
      hipLaunchKernelGGL(qbase::dequant_t_mx_kernel<fp16>, grid, block, 0, st, qp,
                         (const unsigned char*)scale, (fp16*)out, N, (int)K);
  }
  return hipGetLastError();
}
