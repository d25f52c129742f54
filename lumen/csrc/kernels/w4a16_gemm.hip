// MXFP4 weight-only (W4A16, `--quantization mxfp4_a16`) projections for serving:
//
//   weights  ops/quant.py Mxfp4Weight: blocks of 32 consecutive k, one E8M0 scale byte e
//            (2^(e - 127)) and 32 e2m1 codes (two per byte, the low nibble the even k); rows are
//            stored padded to whole blocks with zero nibbles
//   y[m, n]  = round_T(sum_k f32(x[m, k]) f32(wdq[n, k])),  wdq = round_T(code 2^e)  (f32 accum.)
//
// The activations stay bf16 / fp16: no activation quantizer, no row scale.  The weights cross
// HBM -> CU as 4-bit codes and are converted IN REGISTERS to the 16-bit dot2 / MFMA operand by
// v_cvt_scalef32_pk_{bf16,f16}_fp4 (kernels/mxfp4.h: one code byte and the block's 2^e -> one
// packed pair, one VALU op), so no 16-bit copy of W is written to memory.
//
//  * w4a16_gemv_kernel   1 <= M <= 4: kernels/w8_gemm.hip's rows-per-lane GEMV re-cut for 4-bit
//                        rows (a lane's 16-byte load is one MX block);
//  * w4a16_dgemm_kernel  5 <= M <= 256: w8_dgemm_kernel's tile / split-K structure with W
//                        streamed as code words into the A operand of v_mfma_f32_16x16x32.
//
// Lane-to-k map of the MFMA kernel: per k64 stage a lane loads the 8 bytes = 16 codes
// W[row][k0 + 16 g .. + 15] (g = lane >> 4), which lie in ONE block, so one scale byte serves
// them; word s of the two feeds MFMA s.  Element j of lane group g in MFMA s is therefore
// k = k0 + 16 g + 8 s + j -- the permutation of kernels/w8_gemm.hip -- and x's B operand is read
// from LDS at the same k (16-byte chunk 2 g + s of the stage).
#include "api.h"
#include "common.h"
#include "dgemm.h"
#include "gemv.h"
#include "mxfp4.h"

namespace lumen {
namespace w4a16 {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
using dgemm::f32x4;
using dgemm::ld16z;
using dgemm::Mfma;
using dgemm::ntld16z;
using dgemm::swz;
using gemv::dot2;
using gemv::sum16;
using mx::cvt2;
using mx::cvt8;
using mx::e8m0_f32;

// a block's E8M0 byte where ``ok``, 2^0 elsewhere (0xff would be NaN; the codes that go with it
// are dgemm.h's ntld16z zeros, +0.0)
__device__ __forceinline__ unsigned ntld1s(const unsigned char* p, bool ok) {
  unsigned r = 0x7f;
  if (ok) r = __builtin_nontemporal_load(p);
  return r;
}

// ---- 1 <= M <= 4: rows-per-lane GEMV -----------------------------------------------------------
// lane = one 16-byte chunk = 32 codes = ONE MX block of each of R weight rows, plus that block's
// scale byte: a wave instruction reads 1 KiB = 2048 k of ONE row and 64 consecutive scale bytes
// of it; the lane's x chunk (64 bytes per activation row) is loaded once per R rows.  A 2048-k
// step is twice the k of the fp8 GEMV's, so at K = 4096 only two waves of a workgroup can share a
// row: KW (2 or 4) waves split K in 2048-element steps (GS steps of loads issued before the first
// conversion) and meet in LDS, and the workgroup's 4 / KW wave groups take R rows each.  A code
// byte is converted once and used by all M rows of x: 16 conversions + 16 M dot2 per chunk.
template <typename T, int MM, int R, int GS, int KW>
__global__ void __launch_bounds__(256)
w4a16_gemv_kernel(const T* __restrict__ x, const unsigned char* __restrict__ W,
                  const unsigned char* __restrict__ scale, T* __restrict__ y, int N, int K, int M,
                  long long ldx, long long ldy) {
  constexpr int RG = 4 / KW;
  __shared__ float red[4][MM][R];
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kw = wid % KW, rg = wid / KW;
  const int n0 = (blockIdx.x * RG + rg) * R;
  const int KB = (K + 31) >> 5;   // blocks per row: 16 code bytes and one scale byte each
  const int S = (KB + 63) >> 6;   // 2048-element steps
  // a wave group past N (the last workgroup) has no steps: it reads nothing
  const int s0 = n0 < N ? (kw * S) / KW : 0, s1 = n0 < N ? ((kw + 1) * S) / KW : 0;
  const unsigned char* wp = W + (long long)n0 * (16LL * KB) + 16 * lane;
  const unsigned char* sp = scale + (long long)n0 * KB + lane;
  const T* xp = x + 32 * lane;
  float acc[MM][R];
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[m][r] = 0.f;
  for (int s = s0; s < s1; s += GS) {
    uint4 wv[GS][R], xv[GS][MM][4];
    unsigned sv[GS][R];
#pragma unroll
    for (int u = 0; u < GS; ++u) {
      const int b = (s + u) * 64 + lane;        // this lane's block
      const bool ok = (s + u < s1) && b < KB;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool okr = ok && n0 + r < N;       // rows past N are neither read nor written
        wv[u][r] = ntld16z(wp + (long long)r * (16LL * KB) + (s + u) * 1024, okr);
        sv[u][r] = ntld1s(sp + (long long)r * KB + (s + u) * 64, okr);
      }
#pragma unroll
      for (int m = 0; m < MM; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)   // K % 8 == 0: whole 16-byte x chunks; none past K
          xv[u][m][j] = ld16z(xp + (long long)m * ldx + (long long)(s + u) * 2048 + 8 * j,
                              ok && m < M && 32 * b + 8 * j < K);
    }
#pragma unroll
    for (int u = 0; u < GS; ++u) {
      if (s + u < s1) {  // wave-uniform: no conversions for the steps past this wave's range
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float sc = e8m0_f32(sv[u][r]);
          const unsigned wd[4] = {wv[u][r].x, wv[u][r].y, wv[u][r].z, wv[u][r].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint4 a = cvt8<T>(wd[j], sc);
#pragma unroll
            for (int m = 0; m < MM; ++m) {
              float c = acc[m][r];
              c = dot2<T>(a.x, xv[u][m][j].x, c);
              c = dot2<T>(a.y, xv[u][m][j].y, c);
              c = dot2<T>(a.z, xv[u][m][j].z, c);
              c = dot2<T>(a.w, xv[u][m][j].w, c);
              acc[m][r] = c;
            }
          }
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
  if (threadIdx.x < RG * MM * R) {
    const int g = threadIdx.x / (MM * R), m = (threadIdx.x / R) % MM, r = threadIdx.x % R;
    const int n = (blockIdx.x * RG + g) * R + r;
    if (m < M && n < N) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < KW; ++w) v += red[g * KW + w][m][r];
      y[(long long)m * ldy + n] = from_f32<T>(v);
    }
  }
}

// ---- 5 <= M <= 256: W4A16 on v_mfma_f32_16x16x32_{bf16,f16} -------------------------------------
// Block tile = BM rows (the padded decode batch) x BN output columns x a K range (split-K S), 4
// waves; the product is formed transposed, y^T = W x^T (W rows are the A operand), as in
// kernels/w8_gemm.hip, so a lane's four accumulators are four consecutive output columns.
//  * W goes global -> registers as codes: wave w owns columns [w BN / 4, (w + 1) BN / 4); per k64
//    stage a lane loads the 8 bytes W[row 16 i + (lane & 15)][k0 + 16 (lane >> 4) ..] and their
//    block's scale byte, PD stages ahead, and converts them to the A operands of TWO MFMAs (word
//    0, word 1): the lane-to-k map of the header.  A converted fragment feeds all BM / 16 row
//    blocks of the wave.
//  * x (L2-resident, shared by every wave) goes global -> registers -> LDS in k64 stages, double
//    buffered in LDS (one barrier per stage), its 16-byte chunks XOR-swizzled as in
//    decode_gemm.hip.  The registers hold a ring of XD stages: the load of stage t + 1 + XD is
//    issued when stage t + 1 moves to LDS.  The vector-memory counter retires in order, so a
//    stage that consumed the x it had just requested (one stage in flight, as in w8_gemm.hip)
//    waited for every outstanding load, the W prefetch included, once per stage.
//  * the k loop has no branch, for the same reason: behind a lane or stage condition the
//    compiler waits for ALL outstanding loads (s_waitcnt vmcnt(0)) instead of counting.  Every
//    load is unconditional at a clamped, in-bounds address, and a slice runs whole groups of PD
//    stages: x chunks past K (K % 32 == 0: the last stage may be half a stage) and past the
//    slice's last stage are masked to zero on their way to LDS, and the W words that meet them
//    re-read the row's last block (finite codes, times zero).
//  * split-K: see dgemm.h.
constexpr int BK = 64;     // k elements per stage: one 128-byte LDS row per x row, 32 W bytes
constexpr int ROWB = 128;
constexpr int PD = 8;      // k64 stages of W in flight per wave (8 bytes per lane and stage)
constexpr int NT = 256;

template <typename T, int BM, int BN>
__global__ void __launch_bounds__(NT, 1)
w4a16_dgemm_kernel(const T* __restrict__ x, const unsigned char* __restrict__ W,
                   const unsigned char* __restrict__ scale, T* __restrict__ y,
                   float* __restrict__ ws, int* __restrict__ cnt, int M, int N, int K,
                   long long ldx, long long ldy, int S, int kt_total) {
  constexpr int NI = BN / 64, MJ = BM / 16;
  static_assert(NI * 64 == BN && MJ * 16 == BM, "wave tiling");
  constexpr int XQ = BM * 8 / NT;  // 16-byte x chunks per thread per stage
  static_assert(XQ * NT == BM * 8, "x staging");
  constexpr int XD = BM == 256 ? 2 : 4;  // stages of x in flight in registers
  static_assert(PD % XD == 0, "x ring slots are static inside the unrolled PD stages");
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
  const int KB = K >> 5;  // blocks per W row (K % 32 == 0)

  // rows past N / M re-read the last valid row (finite data; those outputs are never stored)
  const unsigned char* wp[NI];
  const unsigned char* sp[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const long long row = n0 + min(nrow0 + 16 * i + lr, nvalid - 1);
    wp[i] = W + row * (16LL * KB) + 8 * (lg & 1);
    sp[i] = scale + row * KB;
  }
  const int wblk = 2 * kb + (lg >> 1);  // this lane's block in stage 0 of the slice
  const auto wload = [&](int i, int t) {
    return __builtin_bit_cast(uint2, __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(
        wp[i] + 16LL * min(wblk + 2 * t, KB - 1))));
  };
  const auto sload = [&](int i, int t) -> unsigned {
    return __builtin_nontemporal_load(sp[i] + min(wblk + 2 * t, KB - 1));
  };
  // x staging: thread -> chunk c0 of rows r0 + 32 q (32 q leaves the swizzle unchanged)
  const int r0 = threadIdx.x >> 3, c0 = threadIdx.x & 7;
  const int xk = kb * BK + 8 * c0;
  const int xl = r0 * ROWB + ((c0 ^ swz(r0)) << 4);
  const auto xload = [&](int q, int t) {  // K % 8 == 0: whole chunks; past K the row's last one
    return *reinterpret_cast<const uint4*>(x + (long long)min(r0 + 32 * q, M - 1) * ldx +
                                           min(xk + t * BK, K - 8));
  };
  // stage t's chunks to LDS image ``img``, those past K or past the slice as zeros
  const auto xstore = [&](char* img, const uint4* v, int t) {
    const unsigned keep = (t < nk && xk + t * BK < K) ? ~0u : 0u;
#pragma unroll
    for (int q = 0; q < XQ; ++q)
      *reinterpret_cast<uint4*>(img + xl + q * 32 * ROWB) =
          make_uint4(v[q].x & keep, v[q].y & keep, v[q].z & keep, v[q].w & keep);
  };

  f32x4 acc[NI][MJ];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < MJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  uint2 wc[PD][NI], wn[PD][NI];
  unsigned sc[PD][NI], sn[PD][NI];
#pragma unroll
  for (int u = 0; u < PD; ++u)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      wc[u][i] = wload(i, u);
      sc[u][i] = sload(i, u);
    }
  uint4 xr[XD][XQ];  // slot t % XD holds stage t + 1 when stage t begins
#pragma unroll
  for (int q = 0; q < XQ; ++q) xr[0][q] = xload(q, 0);
  xstore(lds, xr[0], 0);
#pragma unroll
  for (int d = 0; d < XD; ++d)
#pragma unroll
    for (int q = 0; q < XQ; ++q) xr[d][q] = xload(q, 1 + d);
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
      // stage t + 1 moves to the other LDS buffer (every wave finished reading it before the
      // barrier that ended stage t - 1) and its slot takes the load of stage t + 1 + XD
      xstore(lds + (buf ^ 1) * STAGE_B, xr[u % XD], t + 1);
#pragma unroll
      for (int q = 0; q < XQ; ++q) xr[u % XD][q] = xload(q, t + 1 + XD);
      const char* img = lds + buf * STAGE_B;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        uint4 a[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i)
          a[i] = cvt8<T>(s == 0 ? wc[u][i].x : wc[u][i].y, e8m0_f32(sc[u][i]));
#pragma unroll
        for (int j = 0; j < MJ; ++j) {
          const int r = 16 * j + lr;
          const uint4 b =
              *reinterpret_cast<const uint4*>(img + r * ROWB + (((2 * lg + s) ^ swz(r)) << 4));
#pragma unroll
          for (int i = 0; i < NI; ++i) acc[i][j] = Mfma<T>::run(a[i], b, acc[i][j]);
        }
      }
      // stage t + 1 is written for every wave; every wave is done reading stage t
      __syncthreads();
      buf ^= 1;
    }
#pragma unroll
    for (int u = 0; u < PD; ++u)
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        wc[u][i] = wn[u][i];
        sc[u][i] = sn[u][i];
      }
  }

  LUMEN_DGEMM_SPLITK_REDUCE_OR_RETURN(NT, NI, MJ, acc, ws, cnt, tile, slice, S,
                                      reinterpret_cast<int*>(lds + 2 * STAGE_B));

  // lane holds y^T[n = n0 + nrow0 + 16 i + 4 (lane >> 4) + 0..3][m = 16 j + (lane & 15)]
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int n = nrow0 + 16 * i + 4 * lg;
    if (n >= nvalid) continue;  // N % 4 == 0: the four columns are valid together
#pragma unroll
    for (int j = 0; j < MJ; ++j) {
      const int m = 16 * j + lr;
      if (m >= M) continue;
      const uint2 val = make_uint2(pk2<T>(acc[i][j][0], acc[i][j][1]),
                                   pk2<T>(acc[i][j][2], acc[i][j][3]));
      *reinterpret_cast<uint2*>(y + (long long)m * ldy + n0 + n) = val;
    }
  }
}

// one launch per compiled (BM, BN) variant, 4 waves each: the list LUMEN_W4A16_VARIANTS in api.h
template <typename T>
hipError_t launch_dgemm(const void* x, const void* W, const void* scale, void* y, float* ws,
                        int* cnt, int M, int N, int K, long long ldx, long long ldy, int BM,
                        int BN, int S, hipStream_t st) {
  const int tiles_n = (N + BN - 1) / BN;
  dim3 grid(tiles_n * S), block(NT);
#define LUMEN_W4A16_CASE(bm, bn)                                                                \
  if (BM == bm && BN == bn) {                                                                   \
    hipLaunchKernelGGL((w4a16_dgemm_kernel<T, bm, bn>), grid, block, 0, st, (const T*)x,        \
                       (const unsigned char*)W, (const unsigned char*)scale, (T*)y, ws, cnt, M, \
                       N, K, ldx, ldy, S, (K + BK - 1) / BK);                                   \
    return hipGetLastError();                                                                   \
  }
  LUMEN_W4A16_VARIANTS(LUMEN_W4A16_CASE)
#undef LUMEN_W4A16_CASE
  return hipErrorInvalidValue;
}

// rows per wave group R, steps in flight GS and waves along K KW of the GEMV.  KW: four waves
// share a row where every wave gets at least two of the row's 2048-element steps or the steps
// divide evenly, two otherwise (K = 4096: two steps; 11008: six, three per wave).  cfg = 10 R +
// GS picks a compiled (R, GS) (lumen/bench/w4a16_bench.py measures them); cfg = 0 the default.
template <typename T>
hipError_t launch_gemv(const void* x, const void* W, const void* scale, void* y, int M, int N,
                       int K, long long ldx, long long ldy, int cfg, hipStream_t st) {
  const int steps = ((K + 31) / 32 + 63) / 64;
  const int KW = (steps >= 8 || steps % 4 == 0) ? 4 : 2;
  const int MM = M == 3 ? 4 : M;
  // measured (profiles/w4a16_serve): 4 rows per wave group with one step in flight was the
  // fastest or within noise of it at every Llama-2-7B projection and M
  if (cfg == 0) cfg = 41;
  const int R = cfg / 10, GS = cfg % 10;
  dim3 grid((N + (4 / KW) * R - 1) / ((4 / KW) * R)), block(256);
#define LUMEN_W4A16_GEMV(mm, rr, gg, kk)                                                        \
  if (MM == mm && R == rr && GS == gg && KW == kk) {                                            \
    hipLaunchKernelGGL((w4a16_gemv_kernel<T, mm, rr, gg, kk>), grid, block, 0, st, (const T*)x, \
                       (const unsigned char*)W, (const unsigned char*)scale, (T*)y, N, K, M,    \
                       ldx, ldy);                                                               \
    return hipGetLastError();                                                                   \
  }
#define LUMEN_W4A16_GEMV_K(mm, rr, gg) LUMEN_W4A16_GEMV(mm, rr, gg, 2) LUMEN_W4A16_GEMV(mm, rr, gg, 4)
  // (M = 4, R = 8, GS = 2) is not compiled: its 2 x 8 W chunks and 2 x 16 x chunks do not fit
  LUMEN_W4A16_GEMV_K(1, 4, 1) LUMEN_W4A16_GEMV_K(1, 4, 2) LUMEN_W4A16_GEMV_K(1, 8, 1)
  LUMEN_W4A16_GEMV_K(1, 8, 2) LUMEN_W4A16_GEMV_K(2, 4, 1) LUMEN_W4A16_GEMV_K(2, 4, 2)
  LUMEN_W4A16_GEMV_K(2, 8, 1) LUMEN_W4A16_GEMV_K(2, 8, 2) LUMEN_W4A16_GEMV_K(4, 4, 1)
  LUMEN_W4A16_GEMV_K(4, 4, 2) LUMEN_W4A16_GEMV_K(4, 8, 1)
#undef LUMEN_W4A16_GEMV_K
#undef LUMEN_W4A16_GEMV
  return hipErrorInvalidValue;
}

}  // namespace w4a16
}  // namespace lumen

namespace {
inline bool misaligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
           reinterpret_cast<uintptr_t>(c)) & 15) != 0;
}
}  // namespace

// y[M, N] = x[M, K] @ wdq[N, K]^T for 1 <= M <= 4.  W: [N, 16 ceil(K / 32)] code bytes, scale:
// [N, ceil(K / 32)] E8M0 bytes, both contiguous.  K % 16 == 0; N % 4 == 0; x rows at stride ldx
// (% 8, so every 16-byte x load is aligned), y rows at ldy; 16-byte aligned x and W.  cfg: 0, or
// 10 R + GS for one of the compiled (rows per wave group, steps in flight).
extern "C" hipError_t lumen_w4a16_gemv(int dtype, const void* x, const void* W, const void* scale,
                                       void* y, int M, int N, int K, long long ldx, long long ldy,
                                       int cfg, hipStream_t st) {
  if (M < 1 || M > 4 || N < 4 || N % 4 != 0 || K < 16 || K % 16 != 0 || ldx % 8 != 0 ||
      ldx < K || ldy < N || scale == nullptr || y == nullptr || misaligned16(x, W))
    return hipErrorInvalidValue;
  if (dtype == lumen::kBF16)
    return lumen::w4a16::launch_gemv<lumen::bf16>(x, W, scale, y, M, N, K, ldx, ldy, cfg, st);
  if (dtype == lumen::kF16)
    return lumen::w4a16::launch_gemv<lumen::fp16>(x, W, scale, y, M, N, K, ldx, ldy, cfg, st);
  return hipErrorInvalidValue;
}

// The same product on the MFMA kernel, M <= BM <= 256.  K % 32 == 0 (whole MX blocks); N % 4 == 0;
// x rows at stride ldx (% 8), y rows at stride ldy (% 4), 16-byte aligned x, W and y.  1 <= S <=
// ceil(K / 64) (every slice has a k64 stage).  S > 1: ``ws`` holds ceil(N / BN) * S * BM * BN
// floats and ``cnt`` ceil(N / BN) zeroed ints (left zero by every launch).
extern "C" hipError_t lumen_w4a16_decode_gemm(int dtype, const void* x, const void* W,
                                              const void* scale, void* y, float* ws, int* cnt,
                                              int M, int N, int K, long long ldx, long long ldy,
                                              int BM, int BN, int S, hipStream_t st) {
  if (M < 1 || M > BM || BM > 256 || N < 4 || N % 4 != 0 || K < 32 || K % 32 != 0 ||
      ldx % 8 != 0 || ldy % 4 != 0 || ldx < K || ldy < N || S < 1 || S > (K + 63) / 64 ||
      scale == nullptr || misaligned16(x, W, y))
    return hipErrorInvalidValue;
  if (S > 1 && (ws == nullptr || cnt == nullptr)) return hipErrorInvalidValue;
  if (dtype == lumen::kBF16)
    return lumen::w4a16::launch_dgemm<lumen::bf16>(x, W, scale, y, ws, cnt, M, N, K, ldx, ldy, BM,
                                                   BN, S, st);
  if (dtype == lumen::kF16)
    return lumen::w4a16::launch_dgemm<lumen::fp16>(x, W, scale, y, ws, cnt, M, N, K, ldx, ldy, BM,
                                                   BN, S, st);
  return hipErrorInvalidValue;
}
