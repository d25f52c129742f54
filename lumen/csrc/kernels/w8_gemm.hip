// Weight-only fp8 (W8A16) projections for serving: y[M, N] = x[M, K] @ (q[N, K] * scale[N])^T.
//
// Reference behaviour: vLLM's `--quantization fp8` (the serving stack the reference declares,
// SURVEY D11 / CS6) stores the decoder projections as e4m3.  Here the weights are OCP e4m3fn with
// one f32 scale per output row, the activations stay bf16 / fp16 and the accumulation f32: the
// weights cross HBM -> CU as fp8 (half the bytes of the 16-bit stream that bounds low-batch
// decode), are converted IN REGISTERS to the 16-bit dot2 / MFMA operand
// (v_cvt_scalef32_pk_{bf16,f16}_fp8, exact, one VALU op per two elements), and the row scale
// multiplies the f32 sum once before the single rounding to the output type.  No 16-bit copy of
// W is written to memory by the two GEMM kernels; `w8_dequant` (the fallback's first half) is the
// only one that does.
//
//  * w8_gemv_kernel     1 <= M <= 4: kernels/skinny_gemm.hip's rows-per-lane GEMV on fp8 rows;
//  * w8_dgemm_kernel    5 <= M <= 256: kernels/decode_gemm.hip's tile / split-K structure with
//                       W streamed straight into the MFMA A operand;
//  * w8_dequant_kernel  [N, K] fp8 + scales -> 16-bit [N, K].
#include "api.h"
#include "common.h"
#include "dgemm.h"
#include "gemv.h"

namespace lumen {
namespace w8 {

typedef float f32x2 __attribute__((ext_vector_type(2)));
using dgemm::f32x4;
using dgemm::Mfma;
using dgemm::ntload16;
using dgemm::swz;
using gemv::cvt2;
using gemv::cvt8;
using gemv::dot2;
using gemv::sum16;

// 8 weights (two fp8 words) . 8 activations (one 16-byte chunk)
template <typename T>
__device__ __forceinline__ float dot8(unsigned wa, unsigned wb, uint4 xv, float c) {
  c = dot2<T>(cvt2<T, false>(wa), xv.x, c);
  c = dot2<T>(cvt2<T, true>(wa), xv.y, c);
  c = dot2<T>(cvt2<T, false>(wb), xv.z, c);
  c = dot2<T>(cvt2<T, true>(wb), xv.w, c);
  return c;
}

// ---- 1 <= M <= 4: rows-per-lane GEMV -----------------------------------------------------------
// lane = one 16-byte chunk (16 k elements) of each of R weight rows: a wave instruction reads
// 1 KiB of ONE row; the lane's x chunk (32 bytes) is loaded once per R rows.  One workgroup =
// R rows; its 4 waves split K in 1024-element steps (GS steps of loads issued before the first
// conversion) and meet in LDS.
template <typename T, int MM, int R, int GS>
__global__ void __launch_bounds__(256)
w8_gemv_kernel(const T* __restrict__ x, const unsigned char* __restrict__ W,
               const float* __restrict__ scale, T* __restrict__ y, int N, int K, int M,
               long long ldx, long long ldy) {
  __shared__ float red[4][MM][R];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n0 = blockIdx.x * R;
  const int S = (K + 1023) >> 10;  // 1024-element steps
  const int s0 = (wid * S) >> 2, s1 = ((wid + 1) * S) >> 2;
  const unsigned char* wp = W + (long long)n0 * K + 16 * lane;
  const T* xp = x + 16 * lane;
  float acc[MM][R];
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
  const uint4 z = make_uint4(0, 0, 0, 0);
  for (int s = s0; s < s1; s += GS) {
    uint4 wv[GS][R], xv[GS][MM][2];
#pragma unroll
    for (int u = 0; u < GS; ++u) {
      const int k = (s + u) * 1024;
      const bool ok = (s + u < s1) && (k + 16 * lane < K);  // K % 16 == 0: whole chunks only
#pragma unroll
      for (int r = 0; r < R; ++r) wv[u][r] = ok ? ntload16(wp + (long long)r * K + k) : z;
#pragma unroll
      for (int m = 0; m < MM; ++m) {
        const T* xr = xp + (long long)m * ldx + k;
        xv[u][m][0] = (ok && m < M) ? *reinterpret_cast<const uint4*>(xr) : z;
        xv[u][m][1] = (ok && m < M) ? *reinterpret_cast<const uint4*>(xr + 8) : z;
      }
    }
#pragma unroll
    for (int u = 0; u < GS; ++u) {
      if (s + u < s1) {  // wave-uniform: no conversions for the steps past this wave's range
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
          for (int m = 0; m < MM; ++m) {
            acc[m][r] = dot8<T>(wv[u][r].x, wv[u][r].y, xv[u][m][0], acc[m][r]);
            acc[m][r] = dot8<T>(wv[u][r].z, wv[u][r].w, xv[u][m][1], acc[m][r]);
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
          (red[0][m][r] + red[1][m][r] + red[2][m][r] + red[3][m][r]) * scale[n0 + r]);
  }
}

// ---- 5 <= M <= 256: W8A16 on v_mfma_f32_16x16x32_{bf16,f16} -------------------------------------
// Block tile = BM rows (the padded decode batch) x BN output columns x a K range (split-K S), 4
// waves; the product is formed transposed, y^T = W x^T (W rows are the A operand), as in
// kernels/decode_gemm.hip, so a lane's four accumulators are four consecutive output columns.
//  * W goes global -> registers as fp8: wave w owns columns [w BN / 4, (w + 1) BN / 4); per k64
//    step a lane loads the 16 bytes W[row 16 i + (lane & 15)][k0 + 16 (lane >> 4) ..], PD steps
//    ahead, and converts them to the A operands of TWO MFMAs (bytes 0..7, bytes 8..15).  The k
//    order inside the step is therefore permuted (MFMA s, lane group g, element j = k0 + 16 g +
//    8 s + j); x's B operand is read from LDS at the same k, and the sum over k does not care.
//    A converted fragment feeds all BM / 16 row blocks of the wave.
//  * x (L2-resident, shared by every wave) goes global -> registers -> LDS in k64 stages, double
//    buffered (one barrier per stage), its 16-byte chunks XOR-swizzled as in decode_gemm.hip.
//  * split-K: see dgemm.h; whoever stores the tile -- with split-K the last arriver -- applies
//    the row scales.
constexpr int BK = 64;     // k elements per stage: one 128-byte LDS row per x row
constexpr int ROWB = 128;
constexpr int PD = 4;      // k64 steps of W in flight per wave
constexpr int NT = 256;

template <typename T, int BM, int BN>
__global__ void __launch_bounds__(NT, 1)
w8_dgemm_kernel(const T* __restrict__ x, const unsigned char* __restrict__ W,
                const float* __restrict__ scale, T* __restrict__ y, float* __restrict__ ws,
                int* __restrict__ cnt, int M, int N, int K, long long ldx, long long ldy,
                int tiles_n, int S, int kt_total) {
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

  // rows past N / M re-read the last valid row (finite data; those outputs are never stored)
  const unsigned char* wp[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
    wp[i] = W + (long long)(n0 + min(nrow0 + 16 * i + lr, nvalid - 1)) * K + (long long)kb * BK +
            16 * lg;
  // x staging: thread -> chunk c of rows r0 + 32 q (32 q leaves the swizzle unchanged)
  const int r0 = threadIdx.x >> 3, c0 = threadIdx.x & 7;
  const T* xg = x + (long long)kb * BK + 8 * c0;
  const int xl = r0 * ROWB + ((c0 ^ swz(r0)) << 4);
  const auto xrow = [&](int q) { return (long long)min(r0 + 32 * q, M - 1) * ldx; };

  f32x4 acc[NI][MJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const uint4 z = make_uint4(0, 0, 0, 0);
  uint4 wc[PD][NI], wn[PD][NI];
#pragma unroll
  for (int u = 0; u < PD; ++u)
#pragma unroll
    for (int i = 0; i < NI; ++i) wc[u][i] = u < nk ? ntload16(wp[i] + u * BK) : z;
#pragma unroll
  for (int q = 0; q < XQ; ++q)
    *reinterpret_cast<uint4*>(lds + xl + q * 32 * ROWB) =
        *reinterpret_cast<const uint4*>(xg + xrow(q));
  __syncthreads();

  int buf = 0;
  for (int t0 = 0; t0 < nk; t0 += PD) {
#pragma unroll
    for (int u = 0; u < PD; ++u)
#pragma unroll
      for (int i = 0; i < NI; ++i)
        wn[u][i] = t0 + PD + u < nk ? ntload16(wp[i] + (t0 + PD + u) * BK) : z;
#pragma unroll
    for (int u = 0; u < PD; ++u) {
      const int t = t0 + u;
      if (t < nk) {  // block-uniform
        // next stage's x (the last step re-reads its own: in bounds, never written to LDS)
        const int tx = min(t + 1, nk - 1);
        uint4 xr[XQ];
#pragma unroll
        for (int q = 0; q < XQ; ++q)
          xr[q] = *reinterpret_cast<const uint4*>(xg + xrow(q) + tx * BK);
        const char* img = lds + buf * STAGE_B;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          uint4 a[NI];
#pragma unroll
          for (int i = 0; i < NI; ++i)
            a[i] = s == 0 ? cvt8<T>(wc[u][i].x, wc[u][i].y) : cvt8<T>(wc[u][i].z, wc[u][i].w);
#pragma unroll
          for (int j = 0; j < MJ; ++j) {
            const int r = 16 * j + lr;
            const uint4 b =
                *reinterpret_cast<const uint4*>(img + r * ROWB + (((2 * lg + s) ^ swz(r)) << 4));
#pragma unroll
            for (int i = 0; i < NI; ++i) acc[i][j] = Mfma<T>::run(a[i], b, acc[i][j]);
          }
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
      for (int i = 0; i < NI; ++i) wc[u][i] = wn[u][i];
  }

  LUMEN_DGEMM_SPLITK_REDUCE_OR_RETURN(NT, NI, MJ, acc, ws, cnt, tile, slice, S,
                                      reinterpret_cast<int*>(lds + 2 * STAGE_B));

  // lane holds y^T[n = n0 + nrow0 + 16 i + 4 (lane >> 4) + 0..3][m = 16 j + (lane & 15)]
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int n = nrow0 + 16 * i + 4 * lg;
    if (n >= nvalid) continue;  // N % 4 == 0: the four columns are valid together
    const float4 sc = *reinterpret_cast<const float4*>(scale + n0 + n);
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      const int m = 16 * j + lr;
      if (m >= M) continue;
      const uint2 val = make_uint2(pk2<T>(acc[i][j][0] * sc.x, acc[i][j][1] * sc.y),
                                   pk2<T>(acc[i][j][2] * sc.z, acc[i][j][3] * sc.w));
      *reinterpret_cast<uint2*>(y + (long long)m * ldy + n0 + n) = val;
    }
  }
}

// one launch per compiled (BM, BN) variant, 4 waves each: the list LUMEN_W8_VARIANTS in api.h
template <typename T>
hipError_t launch_dgemm(const void* x, const void* W, const float* scale, void* y, float* ws,
                        int* cnt, int M, int N, int K, long long ldx, long long ldy, int BM,
                        int BN, int S, hipStream_t st) {
  const int tiles_n = (N + BN - 1) / BN;
  dim3 grid(tiles_n * S), block(NT);
#define LUMEN_W8_CASE(bm, bn)                                                                   \
  if (BM == bm && BN == bn) {                                                                   \
    hipLaunchKernelGGL((w8_dgemm_kernel<T, bm, bn>), grid, block, 0, st, (const T*)x,           \
                       (const unsigned char*)W, scale, (T*)y, ws, cnt, M, N, K, ldx, ldy,       \
                       tiles_n, S, K / BK);                                                     \
    return hipGetLastError();                                                                   \
  }
  LUMEN_W8_VARIANTS(LUMEN_W8_CASE)
#undef LUMEN_W8_CASE
  return hipErrorInvalidValue;
}

// ---- dequantisation: the fallback's first half ---------------------------------------------------
// out[n, k] = round_to_T(f32(q[n, k]) * scale[n]): f32 multiply, one round-to-nearest-even, i.e.
// bit-identical to QuantWeight.dequant().  16 elements per thread where K % 16 == 0.
template <typename T>
__global__ void __launch_bounds__(256)
w8_dequant_kernel(const unsigned char* __restrict__ q, const float* __restrict__ scale,
                  T* __restrict__ out, long long chunks, int kchunks) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  const float s = scale[c / kchunks];
  const uint4 w = *reinterpret_cast<const uint4*>(q + c * 16);
  const unsigned wd[4] = {w.x, w.y, w.z, w.w};
  unsigned o[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(wd[i], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(wd[i], true);
    o[2 * i] = pk2<T>(lo[0] * s, lo[1] * s);
    o[2 * i + 1] = pk2<T>(hi[0] * s, hi[1] * s);
  }
  uint4* op = reinterpret_cast<uint4*>(out + c * 16);
  op[0] = make_uint4(o[0], o[1], o[2], o[3]);
  op[1] = make_uint4(o[4], o[5], o[6], o[7]);
}

}  // namespace w8
}  // namespace lumen

// y[M, N] = x[M, K] @ (W[N, K] * scale[N])^T for 1 <= M <= 4: W contiguous e4m3fn, N % 4 == 0,
// K % 16 == 0, x rows at stride ldx (% 8, so every 16-byte x load is aligned), y rows at ldy.
extern "C" hipError_t lumen_w8_gemv(int dtype, const void* x, const void* W, const float* scale,
                                    void* y, int M, int N, int K, long long ldx, long long ldy,
                                    hipStream_t st) {
  if (M < 1 || M > 4 || N < 4 || N % 4 != 0 || K < 16 || K % 16 != 0 || ldx % 8 != 0 ||
      ldx < K || ldy < N ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W)) & 15) != 0)
    return hipErrorInvalidValue;
  // rows per lane R and 1024-element steps in flight GS as measured (profiles/w8_serve): 8 rows
  // per workgroup where N allows it -- half the workgroups, twice the bytes each wave requests
  // before its first conversion -- beat 4 rows at every Llama-2-7B projection and M
  const int R = N % 8 == 0 ? 8 : 4;
  dim3 grid(N / R), block(256);
#define LUMEN_W8_GEMV(TT, MM, RR, GG)                                                           \
  hipLaunchKernelGGL((lumen::w8::w8_gemv_kernel<TT, MM, RR, GG>), grid, block, 0, st,           \
                     (const TT*)x, (const unsigned char*)W, scale, (TT*)y, N, K, M, ldx, ldy)
#define LUMEN_W8_GEMV_T(TT)                                                                     \
  if (R == 8) {                                                                                 \
    if (M == 1) LUMEN_W8_GEMV(TT, 1, 8, 2);                                                     \
    else if (M == 2) LUMEN_W8_GEMV(TT, 2, 8, 1);                                                \
    else LUMEN_W8_GEMV(TT, 4, 8, 1);                                                            \
  } else {                                                                                      \
    if (M == 1) LUMEN_W8_GEMV(TT, 1, 4, 2);                                                     \
    else if (M == 2) LUMEN_W8_GEMV(TT, 2, 4, 2);                                                \
    else LUMEN_W8_GEMV(TT, 4, 4, 2);                                                            \
  }
  if (dtype == lumen::kBF16) {
    LUMEN_W8_GEMV_T(lumen::bf16)
  } else if (dtype == lumen::kF16) {
    LUMEN_W8_GEMV_T(lumen::fp16)
  } else {
    return hipErrorInvalidValue;
  }
#undef LUMEN_W8_GEMV_T
#undef LUMEN_W8_GEMV
  return hipGetLastError();
}

// y[M, N] = x[M, K] @ (W[N, K] * scale[N])^T on the MFMA kernel.  M <= BM; K % 64 == 0;
// N % 4 == 0; W contiguous e4m3fn [N, K]; x rows at stride ldx (% 8), y rows at stride ldy (% 4),
// 16-byte aligned bases.  S > 1: ``ws`` holds ceil(N / BN) * S * BM * BN floats and ``cnt``
// ceil(N / BN) zeroed ints (the last slice of each tile re-zeroes its counter, so they stay zero
// between launches).
extern "C" hipError_t lumen_w8_decode_gemm(int dtype, const void* x, const void* W,
                                           const float* scale, void* y, float* ws, int* cnt,
                                           int M, int N, int K, long long ldx, long long ldy,
                                           int BM, int BN, int S, hipStream_t st) {
  if (M < 1 || M > BM || N < 4 || N % 4 != 0 || K < 64 || K % 64 != 0 || ldx % 8 != 0 ||
      ldy % 4 != 0 || ldx < K || ldy < N || S < 1 || S > K / 64 ||
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W) |
        reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(scale)) & 15) != 0)
    return hipErrorInvalidValue;
  if (S > 1 && (ws == nullptr || cnt == nullptr)) return hipErrorInvalidValue;
  if (dtype == lumen::kBF16)
    return lumen::w8::launch_dgemm<lumen::bf16>(x, W, scale, y, ws, cnt, M, N, K, ldx, ldy, BM,
                                                BN, S, st);
  if (dtype == lumen::kF16)
    return lumen::w8::launch_dgemm<lumen::fp16>(x, W, scale, y, ws, cnt, M, N, K, ldx, ldy, BM,
                                                BN, S, st);
  return hipErrorInvalidValue;
}

// out[N, K] (16-bit, contiguous) = q[N, K] (e4m3fn, contiguous) * scale[N]; K % 16 == 0,
// 16-byte aligned bases
extern "C" hipError_t lumen_w8_dequant(int dtype, const void* q, const float* scale, void* out,
                                       long long N, long long K, hipStream_t st) {
  if (N < 1 || K < 16 || K % 16 != 0 || K / 16 > 0x7fffffffLL ||
      ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(out)) & 15) != 0)
    return hipErrorInvalidValue;
  const long long chunks = N * (K / 16);
  const long long blocks = (chunks + 255) / 256;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  dim3 grid((unsigned)blocks), block(256);
  if (dtype == lumen::kBF16)
    hipLaunchKernelGGL(lumen::w8::w8_dequant_kernel<lumen::bf16>, grid, block, 0, st,
                       (const unsigned char*)q, scale, (lumen::bf16*)out, chunks, (int)(K / 16));
  else if (dtype == lumen::kF16)
    hipLaunchKernelGGL(lumen::w8::w8_dequant_kernel<lumen::fp16>, grid, block, 0, st,
                       (const unsigned char*)q, scale, (lumen::fp16*)out, chunks, (int)(K / 16));
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
