// fp8 activations x MXFP4 weights (W4A8, `--quantization mxfp4`) projections for serving:
//
//   weights  blocks of 32 consecutive k: one E8M0 scale byte e (2^(e - 127)) and 32 e2m1 codes
//            (two per byte, the low nibble the even k), ops/quant.py quantize_mxfp4_rows
//   (xq, sx) kernels/w8a8_gemm.hip's per-token e4m3 activations
//   y[m, n]  = round((sum_k f32(xq[m, k]) f32(code[n, k]) 2^e[n, k / 32]) * sx[m])   (f32 accum.)
//
// v_mfma_scale_f32_16x16x128_f8f6f4 takes the codes and the block scales as they are stored: the
// matrix core dequantises, no conversion instruction is issued.
//
//  * w4a8_dgemm_kernel  1 <= M <= 256: kernels/w8a8_gemm.hip's decode kernel (W rows as the A
//                       operand straight from non-temporal loads, xq staged in LDS, XCD remap,
//                       in-launch split-K), BM = 16 for M <= 16 with its own x staging;
//  * w4_dequant_kernel  q, scale -> 16-bit [N, K] for the fallback (v_cvt_scalef32_pk_*_fp4),
//                       bit-identical to ops/quant.py Mxfp4Weight.dequant().
//
// MFMA operands.  A (format 4 = e2m1): lane l holds the 16 bytes = 32 codes k0 + 32 (l >> 4) ..
// + 31 of W row (l & 15) in the first four registers of the operand, and as its scale operand the
// E8M0 byte of exactly that block.  B (format 0 = e4m3) is laid out differently, as two K = 64
// halves: the first four registers of lane l hold the 16 bytes k0 + 16 (l >> 4) .. + 15 of xq row
// (l & 15), the last four the 16 bytes k0 + 64 + 16 (l >> 4) .. + 15; unit scale.  (With equal
// formats on both sides the difference cancels, which is why kernels/w8a8_gemm.hip may load both
// operands by one rule; here the maps must agree element for element.  Found by measurement on
// the hardware and pinned by the exact integer data of tests/test_mxfp4_gpu.py.)  K % 16 == 0:
// 16-byte x chunks past K are zero-filled in registers; W rows are stored padded to whole blocks
// with zero nibbles (+0.0), whole 16-byte W chunks past that are zero-filled in registers with
// scale 2^0.
#include "api.h"
#include "common.h"
#include "dgemm.h"
#include "mxfp4.h"

namespace lumen {
namespace w4a8 {

typedef int i32x8 __attribute__((ext_vector_type(8)));
using dgemm::f32x4;
using dgemm::ld16z;
using dgemm::ntld16z;
using dgemm::swz;

// a block's E8M0 byte where ``ok``, 2^0 elsewhere (0xff would be NaN)
__device__ __forceinline__ int ntld1s(const unsigned char* p, bool ok) {
  int r = 0x7f;
  if (ok) r = __builtin_nontemporal_load(p);
  return r;
}

// one K = 128 step: a = the lane's 32 e2m1 codes with block scale sa, b0 / b1 = its 16 e4m3
// bytes of the first / second K = 64 half
__device__ __forceinline__ f32x4 mma128(uint4 a, int sa, uint4 b0, uint4 b1, f32x4 c) {
  const i32x8 av = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, 0, 0, 0, 0};
  const i32x8 bv = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w,
                    (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
  // formats 4 / 0 = e2m1 / e4m3; scale bytes 0 of sa and of 0x7f (2^0)
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, bv, c, 4, 0, 0, sa, 0, 0x7f);
}

constexpr int BK = 128;    // k elements per step: 128 bytes of an xq row, 64 of a W row
constexpr int ROWB = 128;
constexpr int NT = 256;
constexpr int XP = 16;     // BM = 16: k128 steps of x per LDS panel

// Block tile = BM rows (the padded decode batch) x BN output columns x a K range (split-K S), 4
// waves; y^T = W xq^T, so a lane's four accumulators are four consecutive output columns.
//  * wave w owns columns [w BN / 4, (w + 1) BN / 4); per k128 step a lane loads the 16 bytes
//    W[row 16 i + (lane & 15)][k0 + 32 (lane >> 4) ..] and that block's scale byte, PD steps
//    ahead; they feed all BM / 16 row blocks of the wave.
//  * BM >= 64: xq goes global -> registers -> LDS in k128 stages, double buffered, one barrier
//    per step.  BM = 16: a stage is only 2 KiB, so XP = 16 steps are staged at once into a single
//    32-KiB panel and the steps of a panel run without barriers (two barriers per panel), with
//    PD = 4 steps of W in flight.  (Measured and dropped: a 16-slot register ring of W with a
//    32-step panel -- 16 KiB in flight per wave -- was 1-7 us slower at every 7B projection and
//    twice as slow with split-K: the per-workgroup start-up, not the depth of the stream, is
//    what costs.)
//  * split-K: see dgemm.h; whoever stores the tile -- with split-K the last arriver -- applies
//    sx[m].
template <typename T, int BM, int BN>
__global__ void __launch_bounds__(NT, 1)
w4a8_dgemm_kernel(const unsigned char* __restrict__ xq, const float* __restrict__ sx,
                  const unsigned char* __restrict__ W, const unsigned char* __restrict__ scale,
                  T* __restrict__ y, float* __restrict__ ws, int* __restrict__ cnt, int M, int N,
                  int K, long long ldx, long long ldy, int S, int kt_total) {
  constexpr int NI = BN / 64, MJ = BM / 16;
  static_assert(NI * 64 == BN && MJ * 16 == BM, "wave tiling");
  constexpr bool PANEL = BM == 16;
  constexpr int PD = PANEL ? 4 : 2;  // k128 steps of W in flight per wave
  static_assert(XP % PD == 0, "panel steps");
  constexpr int STAGE_B = BM * ROWB;
  constexpr int LDS_B = PANEL ? XP * STAGE_B : 2 * STAGE_B;
  __shared__ __attribute__((aligned(16))) char lds[LDS_B + 16];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const dgemm::TileSlice ts = dgemm::tile_slice(blockIdx.x, gridDim.x, S);
  const int tile = ts.tile, slice = ts.slice;
  const int n0 = tile * BN;
  const int nvalid = min(BN, N - n0);
  const dgemm::KSlice ks = dgemm::k_slice(slice, S, kt_total);
  const int kb = ks.kb, nk = ks.nk;
  const int nrow0 = wid * (BN / 4);
  const int KB = (K + 31) >> 5;  // blocks per W row: 16 code bytes and one scale byte each

  // rows past N / M re-read the last valid row (finite data; those outputs are never stored)
  const unsigned char* wp[NI];
  const unsigned char* sp[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const long long row = n0 + min(nrow0 + 16 * i + lr, nvalid - 1);
    wp[i] = W + row * (16LL * KB);
    sp[i] = scale + row * KB;
  }
  const int wblk = kb * 4 + lg;  // this lane's first block
  const auto wload = [&](int i, int t) {
    const int b = wblk + 4 * t;
    return ntld16z(wp[i] + 16 * b, t < nk && b < KB);
  };
  const auto sload = [&](int i, int t) {
    const int b = wblk + 4 * t;
    return ntld1s(sp[i] + b, t < nk && b < KB);
  };

  f32x4 acc[NI][MJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 wc[PD][NI], wn[PD][NI];
  int sc[PD][NI], sn[PD][NI];
#pragma unroll
  for (int u = 0; u < PD; ++u)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      wc[u][i] = wload(i, u);
      sc[u][i] = sload(i, u);
    }

  if constexpr (PANEL) {
    // thread -> chunk c0 of row r0 of steps p0 + 2 q + h: 128 chunks per step
    const int r0 = (threadIdx.x >> 3) & 15, c0 = threadIdx.x & 7, h = threadIdx.x >> 7;
    const unsigned char* xrow = xq + (long long)min(r0, M - 1) * ldx;
    const int xl = r0 * ROWB + ((c0 ^ swz(r0)) << 4);
    for (int p0 = 0; p0 < nk; p0 += XP) {
      if (p0) __syncthreads();  // every wave is done reading the previous panel
      uint4 xr[XP / 2];
#pragma unroll
      for (int q = 0; q < XP / 2; ++q) {
        const int t = p0 + 2 * q + h;
        const int k = (kb + t) * BK + 16 * c0;
        xr[q] = ld16z(xrow + k, t < nk && k < K);
      }
#pragma unroll
      for (int q = 0; q < XP / 2; ++q)
        *reinterpret_cast<uint4*>(lds + (2 * q + h) * STAGE_B + xl) = xr[q];
      __syncthreads();
      const int pend = min(nk, p0 + XP);
      for (int t0 = p0; t0 < pend; t0 += PD) {
#pragma unroll
        for (int u = 0; u < PD; ++u)
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            wn[u][i] = wload(i, t0 + PD + u);
            sn[u][i] = sload(i, t0 + PD + u);
          }
#pragma unroll
        for (int u = 0; u < PD; ++u) {
          const int t = t0 + u;
          if (t < pend) {  // block-uniform
            const char* img = lds + (t - p0) * STAGE_B;
            const uint4 b0 =
                *reinterpret_cast<const uint4*>(img + lr * ROWB + ((lg ^ swz(lr)) << 4));
            const uint4 b1 =
                *reinterpret_cast<const uint4*>(img + lr * ROWB + (((4 + lg) ^ swz(lr)) << 4));
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i][0] = mma128(wc[u][i], sc[u][i], b0, b1, acc[i][0]);
          }
        }
#pragma unroll
        for (int u = 0; u < PD; ++u)
#pragma unroll
          for (int i = 0; i < NI; ++i) {
            wc[u][i] = wn[u][i];
            sc[u][i] = sn[u][i];
          }
      }
    }
  } else {
    constexpr int XQ = BM * 8 / NT;  // 16-byte x chunks per thread per stage
    static_assert(XQ * NT == BM * 8, "x staging");
    // x staging: thread -> chunk c0 of rows r0 + 32 q (32 q leaves the swizzle unchanged)
    const int r0 = threadIdx.x >> 3, c0 = threadIdx.x & 7;
    const int xk = kb * BK + 16 * c0;
    const int xl = r0 * ROWB + ((c0 ^ swz(r0)) << 4);
    const auto xload = [&](int q, int t) {
      const int k = xk + t * BK;
      return ld16z(xq + (long long)min(r0 + 32 * q, M - 1) * ldx + k, t < nk && k < K);
    };
#pragma unroll
    for (int q = 0; q < XQ; ++q) *reinterpret_cast<uint4*>(lds + xl + q * 32 * ROWB) = xload(q, 0);
    __syncthreads();

    int buf = 0;
    for (int t0 = 0; t0 < nk; t0 += PD) {
#pragma unroll
      for (int u = 0; u < PD; ++u)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          wn[u][i] = wload(i, t0 + PD + u);
          sn[u][i] = sload(i, t0 + PD + u);
        }
#pragma unroll
      for (int u = 0; u < PD; ++u) {
        const int t = t0 + u;
        if (t < nk) {  // block-uniform
          uint4 xr[XQ];
#pragma unroll
          for (int q = 0; q < XQ; ++q) xr[q] = xload(q, t + 1);  // zero past the slice's last step
          const char* img = lds + buf * STAGE_B;
#pragma unroll
          for (int j = 0; j < MJ; ++j) {
            const int r = 16 * j + lr;
            const uint4 b0 =
                *reinterpret_cast<const uint4*>(img + r * ROWB + ((lg ^ swz(r)) << 4));
            const uint4 b1 =
                *reinterpret_cast<const uint4*>(img + r * ROWB + (((4 + lg) ^ swz(r)) << 4));
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i][j] = mma128(wc[u][i], sc[u][i], b0, b1, acc[i][j]);
          }
          if (t + 1 < nk) {
            char* nxt = lds + (buf ^ 1) * STAGE_B;
#pragma unroll
            for (int q = 0; q < XQ; ++q)
              *reinterpret_cast<uint4*>(nxt + xl + q * 32 * ROWB) = xr[q];
          }
          // stage t + 1 is written for every wave; every wave is done reading stage t
          __syncthreads();
          buf ^= 1;
        }
      }
#pragma unroll
      for (int u = 0; u < PD; ++u)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          wc[u][i] = wn[u][i];
          sc[u][i] = sn[u][i];
        }
    }
  }

  LUMEN_DGEMM_SPLITK_REDUCE_OR_RETURN(NT, NI, MJ, acc, ws, cnt, tile, slice, S,
                                      reinterpret_cast<int*>(lds + LDS_B));

  // lane holds y^T[n = n0 + nrow0 + 16 i + 4 (lane >> 4) + 0..3][m = 16 j + (lane & 15)]
#pragma unroll
  for (int j = 0; j < MJ; ++j) {
    const int m = 16 * j + lr;
    if (m >= M) continue;
    const float sm = sx[m];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int n = nrow0 + 16 * i + 4 * lg;
      if (n >= nvalid) continue;  // N % 4 == 0: the four columns are valid together
      const uint2 val = make_uint2(pk2<T>(acc[i][j][0] * sm, acc[i][j][1] * sm),
                                   pk2<T>(acc[i][j][2] * sm, acc[i][j][3] * sm));
      *reinterpret_cast<uint2*>(y + (long long)m * ldy + n0 + n) = val;
    }
  }
}

// one launch per compiled (BM, BN) variant, 4 waves each: the list LUMEN_W4A8_VARIANTS in api.h
template <typename T>
hipError_t launch_dgemm(const void* xq, const float* sx, const void* W, const void* scale,
                        void* y, float* ws, int* cnt, int M, int N, int K, long long ldx,
                        long long ldy, int BM, int BN, int S, hipStream_t st) {
  const int tiles_n = (N + BN - 1) / BN;
  dim3 grid(tiles_n * S), block(NT);
#define LUMEN_W4A8_CASE(bm, bn)                                                                 \
  if (BM == bm && BN == bn) {                                                                   \
    hipLaunchKernelGGL((w4a8_dgemm_kernel<T, bm, bn>), grid, block, 0, st,                      \
                       (const unsigned char*)xq, sx, (const unsigned char*)W,                   \
                       (const unsigned char*)scale, (T*)y, ws, cnt, M, N, K, ldx, ldy, S,       \
                       (K + BK - 1) / BK);                                                      \
    return hipGetLastError();                                                                   \
  }
  LUMEN_W4A8_VARIANTS(LUMEN_W4A8_CASE)
#undef LUMEN_W4A8_CASE
  return hipErrorInvalidValue;
}

// ---- dequantisation for the fallback -------------------------------------------------------------
// (e8m0_f32 and cvt2, the block scale and the code-byte conversion, are kernels/mxfp4.h's)
using mx::cvt2;
using mx::e8m0_f32;

// thread = 8 consecutive k of one row: one code word in, one 16-byte store out (K % 8 == 0)
template <typename T>
__global__ void __launch_bounds__(256)
w4_dequant_kernel(const unsigned char* __restrict__ q, const unsigned char* __restrict__ scale,
                  T* __restrict__ out, long long N, int K) {
  const int c8 = K >> 3, KB = (K + 31) >> 5;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * c8) return;
  const long long n = idx / c8;
  const int c = (int)(idx - n * c8);
  const unsigned v = *reinterpret_cast<const unsigned*>(q + n * (16LL * KB) + 4 * c);
  const float s = e8m0_f32(scale[n * KB + (c >> 2)]);
  *reinterpret_cast<uint4*>(out + n * K + 8 * c) =
      make_uint4(cvt2<T, 0>(v, s), cvt2<T, 1>(v, s), cvt2<T, 2>(v, s), cvt2<T, 3>(v, s));
}

}  // namespace w4a8
}  // namespace lumen

namespace {
inline bool misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
           reinterpret_cast<uintptr_t>(c)) & 15) != 0;
}
}  // namespace

// y[M, N] = (xq[M, K] @ wdq[N, K]^T) * sx[M] on the decode MFMA kernel, M <= BM <= 256.  W: [N,
// 16 ceil(K / 32)] code bytes, scale: [N, ceil(K / 32)] E8M0 bytes, both contiguous.  K % 16 == 0;
// N % 4 == 0; xq rows at stride ldx bytes (% 16), y rows at stride ldy (% 4), 16-byte aligned
// bases.  1 <= S <= ceil(K / 128) (every slice has a k128 step).  S > 1: ``ws`` holds ceil(N / BN)
// * S * BM * BN floats and ``cnt`` ceil(N / BN) zeroed ints (left zero by every launch).
extern "C" hipError_t lumen_w4a8_decode_gemm(int dtype, const void* xq, const float* sx,
                                             const void* W, const void* scale, void* y, float* ws,
                                             int* cnt, int M, int N, int K, long long ldx,
                                             long long ldy, int BM, int BN, int S,
                                             hipStream_t st) {
  if (M < 1 || M > BM || BM > 256 || N < 4 || N % 4 != 0 || K < 16 || K % 16 != 0 ||
      ldx % 16 != 0 || ldy % 4 != 0 || ldx < K || ldy < N || S < 1 || S > (K + 127) / 128 ||
      sx == nullptr || scale == nullptr || misaligned16(xq, W, y))
    return hipErrorInvalidValue;
  if (S > 1 && (ws == nullptr || cnt == nullptr)) return hipErrorInvalidValue;
  if (dtype == lumen::kBF16)
    return lumen::w4a8::launch_dgemm<lumen::bf16>(xq, sx, W, scale, y, ws, cnt, M, N, K, ldx, ldy,
                                                  BM, BN, S, st);
  if (dtype == lumen::kF16)
    return lumen::w4a8::launch_dgemm<lumen::fp16>(xq, sx, W, scale, y, ws, cnt, M, N, K, ldx, ldy,
                                                  BM, BN, S, st);
  return hipErrorInvalidValue;
}

// out[N, K] (16-bit, contiguous) = e2m1 code * 2^(scale - 127); K % 8 == 0
extern "C" hipError_t lumen_w4_dequant(int dtype, const void* q, const void* scale, void* out,
                                       long long N, long long K, hipStream_t st) {
  if (N < 1 || K < 8 || K % 8 != 0 || K > 0x7fffffffLL || scale == nullptr ||
      misaligned16(q, out))
    return hipErrorInvalidValue;
  const long long blocks = (N * (K / 8) + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  dim3 grid((unsigned)blocks), block(256);
  if (dtype == lumen::kBF16)
    hipLaunchKernelGGL(lumen::w4a8::w4_dequant_kernel<lumen::bf16>, grid, block, 0, st,
                       (const unsigned char*)q, (const unsigned char*)scale, (lumen::bf16*)out, N,
                       (int)K);
  else if (dtype == lumen::kF16)
    hipLaunchKernelGGL(lumen::w4a8::w4_dequant_kernel<lumen::fp16>, grid, block, 0, st,
                       (const unsigned char*)q, (const unsigned char*)scale, (lumen::fp16*)out, N,
                       (int)K);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
