// Shared pieces of the sampling kernels (sampling.hip, sampling_rows.hip): order-preserving
// float keys, the row walker and the radix select over count / mass histograms.
#pragma once
#include "common.h"

namespace lumen {

constexpr int kSampNT = 512;

__device__ __forceinline__ uint32_t fkey(float z) {
  const uint32_t u = __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float keyf(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// NPT = 1: the row's scaled logits cached in LDS (V <= kSampLdsV); NPT = 0: re-read from the
// (L2-resident) logits every pass
constexpr int kSampLdsV = 32768;

template <typename T, int NPT>
struct Row {
  const float* zl;  // LDS copy (NPT = 1)
  const T* p;
  int V;
  float invT;
  __device__ __forceinline__ float ld(int j) const { return to_f32(p[j]) * invT; }
  // f(j, z) for every element this thread owns, 8 at a time: the 8 loads are issued before any
  // f runs (f's LDS histogram atomics would otherwise order each load behind the previous
  // element's atomic -- one LDS / L2 round trip per element, ~7 us per pass over V = 32000)
  template <typename F>
  __device__ __forceinline__ void each(F&& f) const {
    constexpr int U = 8;
    int j0 = threadIdx.x;
    // full batches: no per-element bounds test (each one cost an exec-mask branch)
    for (; j0 + (U - 1) * kSampNT < V; j0 += U * kSampNT) {
      float zz[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (NPT > 0) zz[u] = zl[j0 + u * kSampNT];
        else zz[u] = ld(j0 + u * kSampNT);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) f(j0 + u * kSampNT, zz[u]);
    }
    for (; j0 < V; j0 += U * kSampNT) {
      float zz[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + u * kSampNT;
        const int jc = j < V ? j : V - 1;  // clamped: unconditional loads
        if constexpr (NPT > 0) zz[u] = zl[jc];
        else zz[u] = ld(jc);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int j = j0 + u * kSampNT;
        if (j < V) f(j, zz[u]);
      }
    }
  }
};

// Wave 0 picks the digit: bins descend from 255; lane l owns bins 255-4l .. 252-4l.  Finds the
// bin b where the suffix sum (from 255 down, inclusive) first reaches `need`, writes b and the
// need left inside b to sel[0] / sel64[0].
template <typename C>
__device__ __forceinline__ void pick_digit(const C* hist, unsigned long long need, int* sel_b,
                                           unsigned long long* sel_need) {
  const int lane = threadIdx.x;  // wave 0 only
  unsigned long long v[4], s = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    v[q] = hist[255 - 4 * lane - q];
    s += v[q];
  }
  // inclusive prefix over lanes (lane 0 = the top bins); counts fit 32 bits: one shuffle a step
  unsigned long long pre = s;
  if constexpr (sizeof(C) == 4) {
    unsigned p32 = static_cast<unsigned>(s);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(p32, o, 64);
      if (lane >= o) p32 += t;
    }
    pre = p32;
  } else {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned lo = __shfl_up(static_cast<unsigned>(pre), o, 64);
      const unsigned hi = __shfl_up(static_cast<unsigned>(pre >> 32), o, 64);
      if (lane >= o) pre += (static_cast<unsigned long long>(hi) << 32) | lo;
    }
  }
  const unsigned long long hit = __ballot(pre >= need);
  const int first = hit ? __builtin_ctzll(hit) : 63;
  if (lane == first) {
    unsigned long long base = pre - s;
    int b = 255 - 4 * lane - 3;
    unsigned long long left = need - base;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (base + v[q] >= need || q == 3) {
        b = 255 - 4 * lane - q;
        left = need - base;
        break;
      }
      base += v[q];
    }
    *sel_b = b;
    *sel_need = left;
  }
}

// Largest key t with  sum_{key >= t, key >= lo} weight >= need  (need >= 1), weight = 1
// (MASS = false) or the fixed-point mass (MASS = true).  Four 8-bit levels, MSB first.
template <typename T, int NPT, bool MASS>
__device__ __forceinline__ uint32_t radix_select(const Row<T, NPT>& row, float m, uint32_t lo,
                                 unsigned long long need, unsigned* hc, unsigned long long* hm,
                                 int* sel_b, unsigned long long* sel_need) {
  uint32_t prefix = 0, mask = 0;
#pragma unroll 1
  for (int lvl = 0; lvl < 4; ++lvl) {
    const int shift = 24 - 8 * lvl;
    for (int b = threadIdx.x; b < 256; b += kSampNT) {
      if (MASS) hm[b] = 0; else hc[b] = 0;
    }
    __syncthreads();
    row.each([&](int, float z) {
      const uint32_t k = fkey(z);
      if ((k & mask) == prefix && k >= lo) {
        const int d = (k >> shift) & 255;
        if constexpr (MASS) {
          const unsigned long long w =
              static_cast<unsigned long long>(__expf(z - m) * 4294967296.f);
          if (w) atomicAdd(hm + d, w);
        } else {
          atomicAdd(hc + d, 1u);
        }
      }
    });
    __syncthreads();
    if (threadIdx.x < 64) {
      if constexpr (MASS) pick_digit(hm, need, sel_b, sel_need);
      else pick_digit(hc, need, sel_b, sel_need);
    }
    __syncthreads();
    prefix |= static_cast<uint32_t>(*sel_b) << shift;
    mask |= 255u << shift;
    need = *sel_need;
    __syncthreads();
  }
  return prefix;
}

}  // namespace lumen
