// fp8 activations x fp8 weights (W8A8, `--quantization ptpc_fp8`) projections for serving:
//
//   sx[m]    = max(amax_k |x[m, k]|, tiny) / 448                 (f32, per token row)
//   xq[m, k] = e4m3fn_rne(clamp(f32(x[m, k]) / sx[m], -448, 448))
//   y[m, n]  = round((sum_k f32(xq[m, k]) f32(wq[n, k])) * sx[m] * sw[n])   (f32 accumulation)
//
// Reference behaviour: vLLM's ptpc_fp8 on ROCm (per-token dynamic activation scales, per-channel
// weight scales).  wq / sw are kernels/w8_gemm.hip's weights (ops/quant.py quantize_fp8_rows); the
// fp8 weights go into the matrix cores as they are, with no conversion.
//
//  * act_quant_kernel   x [M, K] 16-bit -> xq [M, K] e4m3fn + sx [M], bit-identical to
//                       ops/quant.py quantize_fp8_tokens;
//  * w8a8_gemv_kernel   1 <= M <= 4: w8_gemm.hip's rows-per-lane GEMV with x read as fp8;
//  * w8a8_dgemm_kernel  5 <= M <= 256: w8_gemm.hip's tile / XCD-remap / in-launch split-K
//                       structure, W chunks straight from the non-temporal loads into the MFMA;
//  * w8a8_gemm_kernel   M > 256: 128 x 128 block tiles, both operands staged in LDS.
//
// MFMA operands.  Both A (W rows) and B (xq rows) are e4m3 bytes of k-contiguous rows, and both
// are loaded by ONE byte -> (lane, register) rule: lane l holds the 32 bytes k0 + 32 (l >> 4) ..
// of row (l & 15).  The scaled K = 128 form (v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 formats, unit
// block scales) takes the 32 bytes as they are; the non-scaled form (v_mfma_f32_16x16x32_fp8_fp8)
// takes them as four 8-byte operands.  Whatever k the hardware assigns to a (lane group, byte) it
// assigns to A and B alike, so the sum over k does not depend on it (tests/test_w8a8_gpu.py proves
// it with exact integer data).  K % 16 == 0: 16-byte chunks past K are zero-filled in registers /
// LDS (a zero byte is 0.0 in e4m3).
#include "api.h"
#include "common.h"
#include "dgemm.h"
#include "gemv.h"

namespace lumen {
namespace w8a8 {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
using dgemm::f32x4;
using dgemm::ld16z;
using dgemm::ntload16;
using dgemm::swz;
using gemv::cvt2;
using gemv::dot2;
using gemv::sum16;

// dgemm::ntld16z, kept here through ntload16 as this file always had it: with the header's form
// (the load written out) w8a8_gemv_kernel<*, 2, 8, 1> takes 83 VGPRs for 76, a wave per SIMD less
__device__ __forceinline__ uint4 ntld16z(const unsigned char* p, bool ok) {
  uint4 r = make_uint4(0, 0, 0, 0);
  if (ok) r = ntload16(p);
  return r;
}

constexpr float kFp8Max = 448.f;
constexpr float kTiny = 1e-12f;

// ---- per-token activation quantisation -----------------------------------------------------------
// One workgroup per row; a thread owns 16-element chunks (two 16-byte loads, one 16-byte store).
// The first QC chunks of a thread stay in registers between the amax pass and the conversion
// (K <= QC * 4096); longer rows re-read the rest (L2 hits).
constexpr int QC = 3;

template <typename T>
__device__ __forceinline__ void unpack16(const uint4& a, const uint4& b, float (&f)[16]) {
  const T* ea = reinterpret_cast<const T*>(&a);
  const T* eb = reinterpret_cast<const T*>(&b);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    f[j] = to_f32(ea[j]);
    f[8 + j] = to_f32(eb[j]);
  }
}

__device__ __forceinline__ float amax16(const float (&f)[16], float m) {
#pragma unroll
  for (int j = 0; j < 16; ++j) m = fmaxf(m, fabsf(f[j]));
  return m;
}

// 16 f32 -> 16 e4m3fn bytes: true f32 division, clamp, round to nearest even (v_cvt_pk_fp8_f32)
__device__ __forceinline__ uint4 quant16(const float (&f)[16], float s) {
  unsigned o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      q[j] = fminf(fmaxf(__fdiv_rn(f[4 * i + j], s), -kFp8Max), kFp8Max);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], w, true);
    o[i] = static_cast<unsigned>(w);
  }
  return make_uint4(o[0], o[1], o[2], o[3]);
}

template <typename T>
__global__ void __launch_bounds__(256)
act_quant_kernel(const T* __restrict__ x, unsigned char* __restrict__ xq, float* __restrict__ sx,
                 int K, long long ldx) {
  __shared__ float red[4];
  const int row = blockIdx.x;
  const int chunks = K >> 4;
  const T* xr = x + (long long)row * ldx;
  unsigned char* qr = xq + (long long)row * K;
  uint4 keep[QC][2];
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < QC; ++i) {
    const int c = threadIdx.x + 256 * i;
    keep[i][0] = keep[i][1] = make_uint4(0, 0, 0, 0);
    if (c < chunks) {
      keep[i][0] = *reinterpret_cast<const uint4*>(xr + 16 * c);
      keep[i][1] = *reinterpret_cast<const uint4*>(xr + 16 * c + 8);
    }
    float f[16];
    unpack16<T>(keep[i][0], keep[i][1], f);
    m = amax16(f, m);
  }
  for (int c = threadIdx.x + 256 * QC; c < chunks; c += 256) {
    float f[16];
    unpack16<T>(*reinterpret_cast<const uint4*>(xr + 16 * c),
                *reinterpret_cast<const uint4*>(xr + 16 * c + 8), f);
    m = amax16(f, m);
  }
  m = block_max<256>(m, red);
  const float s = __fdiv_rn(fmaxf(m, kTiny), kFp8Max);
  if (threadIdx.x == 0) sx[row] = s;
#pragma unroll
  for (int i = 0; i < QC; ++i) {
    const int c = threadIdx.x + 256 * i;
    if (c < chunks) {
      float f[16];
      unpack16<T>(keep[i][0], keep[i][1], f);
      *reinterpret_cast<uint4*>(qr + 16 * c) = quant16(f, s);
    }
  }
  for (int c = threadIdx.x + 256 * QC; c < chunks; c += 256) {
    float f[16];
    unpack16<T>(*reinterpret_cast<const uint4*>(xr + 16 * c),
                *reinterpret_cast<const uint4*>(xr + 16 * c + 8), f);
    *reinterpret_cast<uint4*>(qr + 16 * c) = quant16(f, s);
  }
}

// ---- 1 <= M <= 4: rows-per-lane GEMV -------------------------------------------------------------
// 4 fp8 weights . 4 fp8 activations (one word each)
template <typename T>
__device__ __forceinline__ float dot4(unsigned w, unsigned x, float c) {
  c = dot2<T>(cvt2<T, false>(w), cvt2<T, false>(x), c);
  return dot2<T>(cvt2<T, true>(w), cvt2<T, true>(x), c);
}

// lane = one 16-byte chunk (16 k elements) of each of R weight rows and of each x row; one
// workgroup = R rows, its 4 waves split K in 1024-element steps and meet in LDS.  The x rows are
// converted once per chunk and serve all R weight rows.
template <typename T, int MM, int R, int GS>
__global__ void __launch_bounds__(256)
w8a8_gemv_kernel(const unsigned char* __restrict__ xq, const float* __restrict__ sx,
                 const unsigned char* __restrict__ W, const float* __restrict__ scale,
                 T* __restrict__ y, int N, int K, int M, long long ldx, long long ldy) {
  __shared__ float red[4][MM][R];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n0 = blockIdx.x * R;
  const int S = (K + 1023) >> 10;  // 1024-element steps
  const int s0 = (wid * S) >> 2, s1 = ((wid + 1) * S) >> 2;
  const unsigned char* wp = W + (long long)n0 * K + 16 * lane;
  const unsigned char* xp = xq + 16 * lane;
  float acc[MM][R];
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
  for (int s = s0; s < s1; s += GS) {
    uint4 wv[GS][R], xv[GS][MM];
#pragma unroll
    for (int u = 0; u < GS; ++u) {
      const int k = (s + u) * 1024;
      const bool ok = (s + u < s1) && (k + 16 * lane < K);  // K % 16 == 0: whole chunks only
#pragma unroll
      for (int r = 0; r < R; ++r) wv[u][r] = ntld16z(wp + (long long)r * K + k, ok);
#pragma unroll
      for (int m = 0; m < MM; ++m) xv[u][m] = ld16z(xp + (long long)m * ldx + k, ok && m < M);
    }
#pragma unroll
    for (int u = 0; u < GS; ++u) {
      if (s + u < s1) {  // wave-uniform: no conversions for the steps past this wave's range
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int m = 0; m < MM; ++m) {
            acc[m][r] = dot4<T>(wv[u][r].x, xv[u][m].x, acc[m][r]);
            acc[m][r] = dot4<T>(wv[u][r].y, xv[u][m].y, acc[m][r]);
            acc[m][r] = dot4<T>(wv[u][r].z, xv[u][m].z, acc[m][r]);
            acc[m][r] = dot4<T>(wv[u][r].w, xv[u][m].w, acc[m][r]);
          }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float v = sum16(acc[m][r]);
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (lane == 0) red[wid][m][r] = v;
    }
  __syncthreads();
  if (threadIdx.x < R * MM) {
    const int m = threadIdx.x / R, r = threadIdx.x % R;
    if (m < M)
      y[(long long)m * ldy + n0 + r] = from_f32<T>(
          (red[0][m][r] + red[1][m][r] + red[2][m][r] + red[3][m][r]) * sx[m] * scale[n0 + r]);
  }
}

// ---- the MFMA step shared by the two GEMM kernels ------------------------------------------------
// a0 | a1: the lane's 32 bytes of its A row, b0 | b1: of its B row (see the header).  SC: the
// scaled K = 128 instruction (twice the bf16 rate); else four non-scaled K = 32 ones (bf16 rate).
template <bool SC>
__device__ __forceinline__ f32x4 mma128(uint4 a0, uint4 a1, uint4 b0, uint4 b1, f32x4 c) {
  if constexpr (SC) {
    const i32x8 a = {(int)a0.x, (int)a0.y, (int)a0.z, (int)a0.w,
                     (int)a1.x, (int)a1.y, (int)a1.z, (int)a1.w};
    const i32x8 b = {(int)b0.x, (int)b0.y, (int)b0.z, (int)b0.w,
                     (int)b1.x, (int)b1.y, (int)b1.z, (int)b1.w};
    // formats 0 / 0 = e4m3 / e4m3; block scales 0x7f = 2^0 for every 32-element block
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0x7f7f7f7f, 0,
                                                            0x7f7f7f7f);
  } else {
    const auto l = [](unsigned lo, unsigned hi) {
      return static_cast<long>(static_cast<unsigned long>(lo) |
                               (static_cast<unsigned long>(hi) << 32));
    };
    c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(l(a0.x, a0.y), l(b0.x, b0.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(l(a0.z, a0.w), l(b0.z, b0.w), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(l(a1.x, a1.y), l(b1.x, b1.y), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(l(a1.z, a1.w), l(b1.z, b1.w), c, 0, 0, 0);
    return c;
  }
}

constexpr int BK = 128;    // k elements = bytes per stage: one 128-byte LDS row per tile row
constexpr int ROWB = 128;
constexpr int PD = 2;      // k128 steps of W in flight per wave (decode kernel)
constexpr int NT = 256;

// ---- 5 <= M <= 256 -------------------------------------------------------------------------------
// Block tile = BM rows (the padded decode batch) x BN output columns x a K range (split-K S), 4
// waves; the product is formed transposed, y^T = W xq^T (W rows are the A operand), so a lane's
// four accumulators are four consecutive output columns.
//  * W goes global -> registers as fp8: wave w owns columns [w BN / 4, (w + 1) BN / 4); per k128
//    step a lane loads the 32 bytes W[row 16 i + (lane & 15)][k0 + 32 (lane >> 4) ..], PD steps
//    ahead; they are the A operand as loaded and feed all BM / 16 row blocks of the wave.
//  * xq (L2-resident, shared by every wave) goes global -> registers -> LDS in k128 stages of
//    128 bytes per row (half the bytes of the 16-bit kernel's stage per k), double buffered.
//  * split-K: see dgemm.h; whoever stores the tile -- with split-K the last arriver -- applies
//    sx[m] * sw[n].
template <typename T, int BM, int BN, bool SC>
__global__ void __launch_bounds__(NT, 1)
w8a8_dgemm_kernel(const unsigned char* __restrict__ xq, const float* __restrict__ sx,
                  const unsigned char* __restrict__ W, const float* __restrict__ scale,
                  T* __restrict__ y, float* __restrict__ ws, int* __restrict__ cnt, int M, int N,
                  int K, long long ldx, long long ldy, int S, int kt_total) {
  constexpr int NI = BN / 64, MJ = BM / 16;
  static_assert(NI * 64 == BN && MJ * 16 == BM, "wave tiling");
  constexpr int XQ = BM * 8 / NT;  // 16-byte x chunks per thread per stage
  static_assert(XQ * NT == BM * 8, "x staging");
  constexpr int STAGE_B = BM * ROWB;
  __shared__ __attribute__((aligned(16))) char lds[2 * STAGE_B + 16];
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

  // rows past N / M re-read the last valid row (finite data; those outputs are never stored);
  // chunks past K are zero
  const unsigned char* wp[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
    wp[i] = W + (long long)(n0 + min(nrow0 + 16 * i + lr, nvalid - 1)) * K;
  const int wk = kb * BK + 32 * lg;  // this lane's first k
  const auto wload = [&](int i, int t, int h) {
    const int k = wk + t * BK + 16 * h;
    return ntld16z(wp[i] + k, t < nk && k < K);
  };
  // x staging: thread -> chunk c0 of rows r0 + 32 q (32 q leaves the swizzle unchanged)
  const int r0 = threadIdx.x >> 3, c0 = threadIdx.x & 7;
  const int xk = kb * BK + 16 * c0;
  const int xl = r0 * ROWB + ((c0 ^ swz(r0)) << 4);
  const auto xload = [&](int q, int t) {
    const int k = xk + t * BK;
    return ld16z(xq + (long long)min(r0 + 32 * q, M - 1) * ldx + k, t < nk && k < K);
  };

  f32x4 acc[NI][MJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint4 wc[PD][NI][2], wn[PD][NI][2];
#pragma unroll
  for (int u = 0; u < PD; ++u)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      wc[u][i][0] = wload(i, u, 0);
      wc[u][i][1] = wload(i, u, 1);
    }
#pragma unroll
  for (int q = 0; q < XQ; ++q) *reinterpret_cast<uint4*>(lds + xl + q * 32 * ROWB) = xload(q, 0);
  __syncthreads();

  int buf = 0;
  for (int t0 = 0; t0 < nk; t0 += PD) {
#pragma unroll
    for (int u = 0; u < PD; ++u)
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        wn[u][i][0] = wload(i, t0 + PD + u, 0);
        wn[u][i][1] = wload(i, t0 + PD + u, 1);
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
              *reinterpret_cast<const uint4*>(img + r * ROWB + (((2 * lg) ^ swz(r)) << 4));
          const uint4 b1 =
              *reinterpret_cast<const uint4*>(img + r * ROWB + (((2 * lg + 1) ^ swz(r)) << 4));
#pragma unroll
          for (int i = 0; i < NI; ++i)
            acc[i][j] = mma128<SC>(wc[u][i][0], wc[u][i][1], b0, b1, acc[i][j]);
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
        wc[u][i][0] = wn[u][i][0];
        wc[u][i][1] = wn[u][i][1];
      }
  }

  LUMEN_DGEMM_SPLITK_REDUCE_OR_RETURN(NT, NI, MJ, acc, ws, cnt, tile, slice, S,
                                      reinterpret_cast<int*>(lds + 2 * STAGE_B));

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
      const float4 sc = *reinterpret_cast<const float4*>(scale + n0 + n);
      const uint2 val = make_uint2(pk2<T>(acc[i][j][0] * sm * sc.x, acc[i][j][1] * sm * sc.y),
                                   pk2<T>(acc[i][j][2] * sm * sc.z, acc[i][j][3] * sm * sc.w));
      *reinterpret_cast<uint2*>(y + (long long)m * ldy + n0 + n) = val;
    }
  }
}

// one launch per compiled (BM, BN) variant, 4 waves each: the list LUMEN_W8A8_VARIANTS in api.h
template <typename T, bool SC>
hipError_t launch_dgemm(const void* xq, const float* sx, const void* W, const float* scale,
                        void* y, float* ws, int* cnt, int M, int N, int K, long long ldx,
                        long long ldy, int BM, int BN, int S, hipStream_t st) {
  const int tiles_n = (N + BN - 1) / BN;
  dim3 grid(tiles_n * S), block(NT);
#define LUMEN_W8A8_CASE(bm, bn)                                                                 \
  if (BM == bm && BN == bn) {                                                                   \
    hipLaunchKernelGGL((w8a8_dgemm_kernel<T, bm, bn, SC>), grid, block, 0, st,                  \
                       (const unsigned char*)xq, sx, (const unsigned char*)W, scale, (T*)y, ws, \
                       cnt, M, N, K, ldx, ldy, S, (K + BK - 1) / BK);                           \
    return hipGetLastError();                                                                   \
  }
  LUMEN_W8A8_VARIANTS(LUMEN_W8A8_CASE)
#undef LUMEN_W8A8_CASE
  return hipErrorInvalidValue;
}

// ---- M > 256: block-tiled fp8 x fp8 GEMM on the scaled K = 128 MFMA -------------------------------
// Block tile = 128 rows of xq x 128 rows of W, 4 waves as 2 x 2, each 64 x 64 = 4 x 4 MFMA tiles
// (the product again transposed, y^T = W xq^T).  Both tiles are staged global -> registers -> LDS
// in k128 stages (16 KiB each, swizzled as above), double buffered with one barrier per stage.
// The XCD remap puts the M tiles of one W tile on one XCD.
constexpr int GT = 128;

template <typename T>
__global__ void __launch_bounds__(NT, 1)
w8a8_gemm_kernel(const unsigned char* __restrict__ xq, const float* __restrict__ sx,
                 const unsigned char* __restrict__ W, const float* __restrict__ scale,
                 T* __restrict__ y, int M, int N, int K, long long ldx, long long ldy,
                 int tiles_m) {
  constexpr int TILE_B = GT * ROWB;           // one operand tile of one stage
  constexpr int CQ = GT * 8 / NT;             // 16-byte chunks per thread per operand per stage
  __shared__ __attribute__((aligned(16))) char lds[4 * TILE_B];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lr = lane & 15, lg = lane >> 4;
  const int nb = gridDim.x, bid = blockIdx.x;
  const int xcd = bid & 7, q8 = nb >> 3, r8 = nb & 7;
  const int v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int tn = v / tiles_m, tm = v - tn * tiles_m;
  const int m0 = tm * GT, n0 = tn * GT;
  const int mvalid = min(GT, M - m0), nvalid = min(GT, N - n0);
  const int wn0 = (wid >> 1) * 64, wm0 = (wid & 1) * 64;
  const int nk = (K + BK - 1) / BK;

  const int r0 = threadIdx.x >> 3, c0 = threadIdx.x & 7;
  const int sl = r0 * ROWB + ((c0 ^ swz(r0)) << 4);
  // rows past M / N re-read the last valid row; chunks past K are zero
  const auto gload = [&](const unsigned char* base, long long ld, int row0, int valid, int q,
                         int t) {
    const int k = t * BK + 16 * c0;
    return ld16z(base + (long long)(row0 + min(r0 + 32 * q, valid - 1)) * ld + k,
                 t < nk && k < K);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int q = 0; q < CQ; ++q) {
    *reinterpret_cast<uint4*>(lds + sl + q * 32 * ROWB) = gload(W, K, n0, nvalid, q, 0);
    *reinterpret_cast<uint4*>(lds + TILE_B + sl + q * 32 * ROWB) = gload(xq, ldx, m0, mvalid, q, 0);
  }
  __syncthreads();

  int buf = 0;
  for (int t = 0; t < nk; ++t) {
    uint4 wr[CQ], xr[CQ];
#pragma unroll
    for (int q = 0; q < CQ; ++q) {
      wr[q] = gload(W, K, n0, nvalid, q, t + 1);
      xr[q] = gload(xq, ldx, m0, mvalid, q, t + 1);
    }
    const char* wimg = lds + buf * 2 * TILE_B;
    const char* ximg = wimg + TILE_B;
    uint4 a[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wn0 + 16 * i + lr;
      a[i][0] = *reinterpret_cast<const uint4*>(wimg + r * ROWB + (((2 * lg) ^ swz(r)) << 4));
      a[i][1] = *reinterpret_cast<const uint4*>(wimg + r * ROWB + (((2 * lg + 1) ^ swz(r)) << 4));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = wm0 + 16 * j + lr;
      const uint4 b0 =
          *reinterpret_cast<const uint4*>(ximg + r * ROWB + (((2 * lg) ^ swz(r)) << 4));
      const uint4 b1 =
          *reinterpret_cast<const uint4*>(ximg + r * ROWB + (((2 * lg + 1) ^ swz(r)) << 4));
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i][j] = mma128<true>(a[i][0], a[i][1], b0, b1, acc[i][j]);
    }
    if (t + 1 < nk) {
      char* nxt = lds + (buf ^ 1) * 2 * TILE_B;
#pragma unroll
      for (int q = 0; q < CQ; ++q) {
        *reinterpret_cast<uint4*>(nxt + sl + q * 32 * ROWB) = wr[q];
        *reinterpret_cast<uint4*>(nxt + TILE_B + sl + q * 32 * ROWB) = xr[q];
      }
    }
    __syncthreads();
    buf ^= 1;
  }

  // lane holds y^T[n = n0 + wn0 + 16 i + 4 (lane >> 4) + 0..3][m = m0 + wm0 + 16 j + (lane & 15)]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = wm0 + 16 * j + lr;
    if (m >= mvalid) continue;
    const float sm = sx[m0 + m];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = wn0 + 16 * i + 4 * lg;
      if (n >= nvalid) continue;  // N % 4 == 0: the four columns are valid together
      const float4 sc = *reinterpret_cast<const float4*>(scale + n0 + n);
      const uint2 val = make_uint2(pk2<T>(acc[i][j][0] * sm * sc.x, acc[i][j][1] * sm * sc.y),
                                   pk2<T>(acc[i][j][2] * sm * sc.z, acc[i][j][3] * sm * sc.w));
      *reinterpret_cast<uint2*>(y + (long long)(m0 + m) * ldy + n0 + n) = val;
    }
  }
}

}  // namespace w8a8
}  // namespace lumen

namespace {
inline bool misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr,
                         const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
           reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) != 0;
}
}  // namespace

// xq[M, K] (e4m3fn, contiguous), sx[M] = per-row dynamic quantisation of x[M, K] (16-bit, rows at
// stride ldx % 8 == 0, 16-byte aligned base); K % 16 == 0
extern "C" hipError_t lumen_act_quant_fp8(int dtype, const void* x, void* xq, float* sx, int M,
                                          int K, long long ldx, hipStream_t st) {
  if (M < 1 || K < 16 || K % 16 != 0 || ldx % 8 != 0 || ldx < K || sx == nullptr ||
      misaligned16(x, xq))
    return hipErrorInvalidValue;
  dim3 grid(M), block(256);
  if (dtype == lumen::kBF16)
    hipLaunchKernelGGL(lumen::w8a8::act_quant_kernel<lumen::bf16>, grid, block, 0, st,
                       (const lumen::bf16*)x, (unsigned char*)xq, sx, K, ldx);
  else if (dtype == lumen::kF16)
    hipLaunchKernelGGL(lumen::w8a8::act_quant_kernel<lumen::fp16>, grid, block, 0, st,
                       (const lumen::fp16*)x, (unsigned char*)xq, sx, K, ldx);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// y[M, N] = (xq[M, K] @ W[N, K]^T) * sx[M] * scale[N] for 1 <= M <= 4: W contiguous e4m3fn,
// N % 4 == 0, K % 16 == 0, xq rows at stride ldx bytes (% 16), y (16-bit) rows at ldy.
extern "C" hipError_t lumen_w8a8_gemv(int dtype, const void* xq, const float* sx, const void* W,
                                      const float* scale, void* y, int M, int N, int K,
                                      long long ldx, long long ldy, hipStream_t st) {
  if (M < 1 || M > 4 || N < 4 || N % 4 != 0 || K < 16 || K % 16 != 0 || ldx % 16 != 0 ||
      ldx < K || ldy < N || sx == nullptr || scale == nullptr || misaligned16(xq, W))
    return hipErrorInvalidValue;
  // rows per lane and steps in flight as kernels/w8_gemm.hip's GEMV
  const int R = N % 8 == 0 ? 8 : 4;
  dim3 grid(N / R), block(256);
#define LUMEN_W8A8_GEMV(TT, MM, RR, GG)                                                         \
  hipLaunchKernelGGL((lumen::w8a8::w8a8_gemv_kernel<TT, MM, RR, GG>), grid, block, 0, st,       \
                     (const unsigned char*)xq, sx, (const unsigned char*)W, scale, (TT*)y, N,   \
                     K, M, ldx, ldy)
#define LUMEN_W8A8_GEMV_T(TT)                                                                   \
  if (R == 8) {                                                                                 \
    if (M == 1) LUMEN_W8A8_GEMV(TT, 1, 8, 2);                                                   \
    else if (M == 2) LUMEN_W8A8_GEMV(TT, 2, 8, 1);                                              \
    else LUMEN_W8A8_GEMV(TT, 4, 8, 1);                                                          \
  } else {                                                                                      \
    if (M == 1) LUMEN_W8A8_GEMV(TT, 1, 4, 2);                                                   \
    else if (M == 2) LUMEN_W8A8_GEMV(TT, 2, 4, 2);                                              \
    else LUMEN_W8A8_GEMV(TT, 4, 4, 2);                                                          \
  }
  if (dtype == lumen::kBF16) {
    LUMEN_W8A8_GEMV_T(lumen::bf16)
  } else if (dtype == lumen::kF16) {
    LUMEN_W8A8_GEMV_T(lumen::fp16)
  } else {
    return hipErrorInvalidValue;
  }
#undef LUMEN_W8A8_GEMV_T
#undef LUMEN_W8A8_GEMV
  return hipGetLastError();
}

// The same product on the decode MFMA kernel, M <= BM <= 256.  K % 16 == 0; N % 4 == 0; xq rows
// at stride ldx bytes (% 16), y rows at stride ldy (% 4), 16-byte aligned bases.  form 0: the
// scaled K = 128 MFMA, 1: the non-scaled K = 32 one.  1 <= S <= ceil(K / 128) (every slice has a
// k128 step), which implies S <= K / 64 for K >= 128.  S > 1: ``ws`` holds ceil(N / BN) * S * BM *
// BN floats and ``cnt`` ceil(N / BN) zeroed ints (left zero by every launch).
extern "C" hipError_t lumen_w8a8_decode_gemm(int dtype, const void* xq, const float* sx,
                                             const void* W, const float* scale, void* y,
                                             float* ws, int* cnt, int M, int N, int K,
                                             long long ldx, long long ldy, int BM, int BN, int S,
                                             int form, hipStream_t st) {
  if (M < 1 || M > BM || BM > 256 || N < 4 || N % 4 != 0 || K < 16 || K % 16 != 0 ||
      ldx % 16 != 0 || ldy % 4 != 0 || ldx < K || ldy < N || S < 1 || S > (K + 127) / 128 ||
      (form != 0 && form != 1) || sx == nullptr ||
      misaligned16(xq, W, y, scale))
    return hipErrorInvalidValue;
  if (S > 1 && (ws == nullptr || cnt == nullptr)) return hipErrorInvalidValue;
#define LUMEN_W8A8_GO(TT, SC)                                                                   \
  return lumen::w8a8::launch_dgemm<TT, SC>(xq, sx, W, scale, y, ws, cnt, M, N, K, ldx, ldy, BM, \
                                           BN, S, st)
  if (dtype == lumen::kBF16) {
    if (form == 0) LUMEN_W8A8_GO(lumen::bf16, true);
    LUMEN_W8A8_GO(lumen::bf16, false);
  }
  if (dtype == lumen::kF16) {
    if (form == 0) LUMEN_W8A8_GO(lumen::fp16, true);
    LUMEN_W8A8_GO(lumen::fp16, false);
  }
#undef LUMEN_W8A8_GO
  return hipErrorInvalidValue;
}

// The same product on the 128 x 128 block-tiled kernel, M > 256 (any M >= 1 computes correctly).
extern "C" hipError_t lumen_w8a8_gemm(int dtype, const void* xq, const float* sx, const void* W,
                                      const float* scale, void* y, int M, int N, int K,
                                      long long ldx, long long ldy, hipStream_t st) {
  if (M < 1 || N < 4 || N % 4 != 0 || K < 16 || K % 16 != 0 || ldx % 16 != 0 || ldy % 4 != 0 ||
      ldx < K || ldy < N || sx == nullptr || misaligned16(xq, W, y, scale))
    return hipErrorInvalidValue;
  const long long tiles_m = (M + lumen::w8a8::GT - 1) / lumen::w8a8::GT;
  const long long tiles_n = (N + lumen::w8a8::GT - 1) / lumen::w8a8::GT;
  if (tiles_m * tiles_n > 0x7fffffffLL) return hipErrorInvalidValue;
  dim3 grid((unsigned)(tiles_m * tiles_n)), block(lumen::w8a8::NT);
  if (dtype == lumen::kBF16)
    hipLaunchKernelGGL(lumen::w8a8::w8a8_gemm_kernel<lumen::bf16>, grid, block, 0, st,
                       (const unsigned char*)xq, sx, (const unsigned char*)W, scale,
                       (lumen::bf16*)y, M, N, K, ldx, ldy, (int)tiles_m);
  else if (dtype == lumen::kF16)
    hipLaunchKernelGGL(lumen::w8a8::w8a8_gemm_kernel<lumen::fp16>, grid, block, 0, st,
                       (const unsigned char*)xq, sx, (const unsigned char*)W, scale,
                       (lumen::fp16*)y, M, N, K, ldx, ldy, (int)tiles_m);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
