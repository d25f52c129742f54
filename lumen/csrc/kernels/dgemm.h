// What the decode-GEMM family shares: kernels/decode_gemm.hip (16-bit), w8_gemm.hip (W8A16),
// w8a8_gemm.hip (W8A8), w4a8_gemm.hip (W4A8) and w4a16_gemm.hip (W4A16).  Each of them owns its
// operand staging, pipeline, MFMA form, scales and final store; the block -> (tile, k slice) map,
// the in-launch split-K reduction and the small load / swizzle / MFMA helpers are here, once.
#pragma once
#include "common.h"

namespace lumen {
namespace dgemm {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x32_{bf16,f16} on 16-byte operands as they are loaded
template <typename T> struct Mfma;
template <> struct Mfma<bf16> {
  static __device__ __forceinline__ f32x4 run(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                   __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  }
};
template <> struct Mfma<fp16> {
  static __device__ __forceinline__ f32x4 run(uint4 a, uint4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a),
                                                  __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};

// 16-byte chunk c of a 128-byte LDS row r lives at chunk c ^ swz(r): a ds_read_b128 fragment read
// (16 rows at one chunk, lane groups of 16) then touches 16 distinct 16-byte bank slots (rows of
// either parity share the 256-byte bank row's halves; the XOR spreads the 8 row pairs)
__device__ __forceinline__ int swz(int r) { return (r >> 1) & 7; }

// weights are read exactly once per step: non-temporal, so they do not evict x / y
__device__ __forceinline__ uint4 ntload16(const void* p) {
  return __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)));
}
// a 16-byte load where ``ok``, zeros elsewhere (chunks past K, steps past a slice).  The load is
// written out, not a call of ntload16: the W4A8 kernels were register-allocated differently
// through the nested call (w8a8_gemm.hip, the other way round, keeps its own nested form)
__device__ __forceinline__ uint4 ntld16z(const void* p, bool ok) {
  uint4 r = make_uint4(0, 0, 0, 0);
  if (ok)
    r = __builtin_bit_cast(uint4, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)));
  return r;
}
__device__ __forceinline__ uint4 ld16z(const void* p, bool ok) {
  uint4 r = make_uint4(0, 0, 0, 0);
  if (ok) r = *reinterpret_cast<const uint4*>(p);
  return r;
}

// Block -> (output tile, k slice).  The grid is tiles * S blocks.  The hardware deals blocks
// round-robin over the 8 XCDs, so the bijective remap below gives every XCD one contiguous run of
// virtual ids: the S slices of a tile, then the next tile, land on one XCD and meet in its L2.
struct TileSlice {
  int tile, slice;
};
__device__ __forceinline__ TileSlice tile_slice(int bid, int nb, int S) {
  const int xcd = bid & 7, q8 = nb >> 3, r8 = nb & 7;
  const int v = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  TileSlice t;
  t.tile = v / S;
  t.slice = v - t.tile * S;
  return t;
}
// A slice takes an even share of the kt_total k steps, the first (kt_total % S) slices one more:
// steps [kb, kb + nk), nk >= 1 wherever S <= kt_total (every launcher checks that).  Its own
// function, called after the kernel's column bounds as the kernels always did: computed next to
// the tile index the same arithmetic was scheduled differently through the whole prologue.
struct KSlice {
  int kb, nk;
};
__device__ __forceinline__ KSlice k_slice(int slice, int S, int kt_total) {
  const int per = kt_total / S, extra = kt_total - per * S;
  KSlice k;
  k.kb = slice * per + min(slice, extra);
  k.nk = per + (slice < extra ? 1 : 0);
  return k;
}

// In-launch split-K reduction, placed after the k loop by all NT threads of the block with the
// slice's partial sums in ``acc`` (f32x4 [NI][MJ]).  Where S > 1, every block but one per tile
// RETURNS from the kernel here; the one that goes on holds the tile's full sums in ``acc``.
//
//  * every slice stores its f32 slab (register-major: element (i, j) of thread t at
//    ((tile * S + slice) * NI * MJ + i * MJ + j) * NT + t, one 1-KiB wave instruction per
//    accumulator tile), waits for the stores, and after a barrier thread 0 takes a ticket on
//    cnt[tile]: agent-scope release fence, relaxed fetch_add;
//  * the first S - 1 arrivers return without storing; the last one resets the counter, and after
//    an agent-scope acquire fence adds the other slabs to its own accumulators in ascending slice
//    order (so S = 2 is one fixed two-term sum; from S = 3 the order depends on who arrives last);
//  * ``lds_flag`` is one LDS word that nothing else uses: it carries thread 0's verdict to the
//    block.
//
// Contract.  ``ws`` holds tiles * S * NT * NI * MJ * 4 floats and ``cnt`` one int per tile, all
// zero before the first launch.  Every kernel of the family may use the same ``ws`` / ``cnt``
// (ops/gemm.py keeps one pair per device and stream), because launches on one stream do not
// overlap: a launch reads only slabs written in that launch, and each tile's counter receives
// exactly S tickets, the last of which puts it back to zero -- so the counters are zero again when
// the launch ends and never need a memset, graph replays included.  Two streams (or two graphs
// that may run at once) need a pair each.
//
// A macro, not a function: as an inlined template taking ``acc`` by reference the same text was
// scheduled and register-allocated differently (up to 3 % slower slab sums on the 256-row tiles,
// one wave per SIMD less for w8_dgemm_kernel<*, 128, 64>; profiles/dgemm_refactor/resources.md).
// Expanded in the kernel's own body it compiles to what each kernel's private copy did.  Its
// own names end in ``_``.
#define LUMEN_DGEMM_SPLITK_REDUCE_OR_RETURN(NT, NI, MJ, acc, ws, cnt, tile, slice, S, lds_flag)    \
  if ((S) > 1) {                                                                                   \
    float* slab_ = (ws) + ((long long)(tile) * (S) + (slice)) * ((NT) * (NI) * (MJ) * 4);          \
    _Pragma("unroll") for (int i_ = 0; i_ < (NI); ++i_)                                            \
      _Pragma("unroll") for (int j_ = 0; j_ < (MJ); ++j_)                                          \
        *reinterpret_cast<::lumen::dgemm::f32x4*>(                                                 \
            slab_ + ((i_ * (MJ) + j_) * (NT) + threadIdx.x) * 4) = (acc)[i_][j_];                  \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                               \
    __syncthreads();                                                                               \
    int* flag_ = (lds_flag);                                                                       \
    if (threadIdx.x == 0) {                                                                        \
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                                           \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                             \
      const int old_ = __hip_atomic_fetch_add((cnt) + (tile), 1, __ATOMIC_RELAXED,                 \
                                              __HIP_MEMORY_SCOPE_AGENT);                           \
      const int last_ = old_ == (S) - 1;                                                           \
      if (last_)                                                                                   \
        __hip_atomic_store((cnt) + (tile), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);         \
      *flag_ = last_;                                                                              \
    }                                                                                              \
    __syncthreads();                                                                               \
    if (!*flag_) return;                                                                           \
    if (threadIdx.x == 0) {                                                                        \
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                                           \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                             \
    }                                                                                              \
    __syncthreads();                                                                               \
    for (int o_ = 0; o_ < (S); ++o_) {                                                             \
      if (o_ == (slice)) continue;                                                                 \
      const float* os_ = (ws) + ((long long)(tile) * (S) + o_) * ((NT) * (NI) * (MJ) * 4);         \
      _Pragma("unroll") for (int i_ = 0; i_ < (NI); ++i_)                                          \
        _Pragma("unroll") for (int j_ = 0; j_ < (MJ); ++j_)                                        \
          (acc)[i_][j_] += *reinterpret_cast<const ::lumen::dgemm::f32x4*>(                        \
              os_ + ((i_ * (MJ) + j_) * (NT) + threadIdx.x) * 4);                                  \
    }                                                                                              \
  }

}  // namespace dgemm
}  // namespace lumen
