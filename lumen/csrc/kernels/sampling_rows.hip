// Per-request sampling state on the device: seeds, min_p, logit_bias and penalties in the
// sampling launch (kernels/sampling.hip stays the entry of steps that use none of them).
//
// Reference behaviour: vLLM 0.6.0's logits processors and Sampler, in its order.  With x the f32
// logits of a sampled row:
//   0. guided decoding: a row with a token table (int16 next[S][V] of its grammar, the device
//      address in g_table, 0 = unguided) and st = g_state[g_slot[row]]: x[j] = -inf where
//      next[st][j] < 0.  -inf stays -inf through the steps below, has the lowest radix key, no
//      top-p mass and never wins the draw, so out_lp is the log-probability under the masked
//      distribution.  After the draw thread 0 stores next[st][token] into g_state when it is
//      >= 0 (one row per slot per step, as for the counts)
//   1. logit_bias (sparse CSR list per row): x[j] += bias (the bias may be -inf; the engine also
//      lowers min_tokens to -inf entries for EOS / the stop ids)
//   2. penalties from the sequence's count row c[j] (int32: bit 31 = "in the prompt", bits 0..30
//      = times generated): repetition (c != 0, rp != 1: x = x > 0 ? x / rp : x * rp), then
//      x -= fp * n + pp * (n > 0), n = c & 0x7fffffff
//   3. temperature, top-k, top-p exactly as sampling.hip
//   4. min_p: keep z >= max(z) + ln(min_p) -- one more threshold, max-combined with tau
//   5. the draw, with (seed, offset, rngrow) per row: element j's noise is
//      rng_u32(uint32(seed) ^ (uint32(offset) * 0x9E3779B9 + 0x7F4A7C15), rngrow * V + j)
//   6. thread 0 writes the token and bumps counts[slot][token] (one row per slot per step is the
//      engine's invariant: a plain load / store)
// Same structure as sampling.hip: one 512-thread workgroup per row, the row in LDS for
// V <= 32768.  Larger vocabularies go through lumen_logits_process into an f32 scratch and the
// no-LDS form over it (`pre` = the logits are already processed).
#include "api.h"
#include "sampling_common.h"

namespace lumen {

// steps 2 of the header on one element
__device__ __forceinline__ float penalize(float x, int c, float rp, float fp, float pp) {
  if (c != 0) {
    if (rp != 1.f) x = x > 0.f ? x / rp : x * rp;
    const float n = static_cast<float>(c & 0x7fffffff);
    x -= fp * n + pp * (n > 0.f ? 1.f : 0.f);
  }
  return x;
}

// bias entries of one row into the row's f32 copy `x` (LDS or global; this workgroup owns it)
__device__ __forceinline__ void add_bias(float* x, int V, const int* __restrict__ bias_idx,
                                         const float* __restrict__ bias_val, int b0, int b1) {
  for (int e = b0 + threadIdx.x; e < b1; e += blockDim.x) {
    const int j = bias_idx[e];
    if (j >= 0 && j < V) atomicAdd(x + j, bias_val[e]);  // a repeated id sums its entries
  }
}

// x[j] = penalize(x[j], cnt[j]) * scale over the row; cnt read 16 bytes at a time when aligned
__device__ __forceinline__ void penalize_row(float* x, const int* __restrict__ cnt, int V,
                                             float rp, float fp, float pp, float scale) {
  const bool al =
      ((reinterpret_cast<uintptr_t>(cnt) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
  const int nv = al ? V / 4 : 0;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const int4 c = reinterpret_cast<const int4*>(cnt)[i];
    float4 v = reinterpret_cast<float4*>(x)[i];
    v.x = penalize(v.x, c.x, rp, fp, pp) * scale;
    v.y = penalize(v.y, c.y, rp, fp, pp) * scale;
    v.z = penalize(v.z, c.z, rp, fp, pp) * scale;
    v.w = penalize(v.w, c.w, rp, fp, pp) * scale;
    reinterpret_cast<float4*>(x)[i] = v;
  }
  for (int j = nv * 4 + threadIdx.x; j < V; j += blockDim.x)
    x[j] = penalize(x[j], cnt[j], rp, fp, pp) * scale;
}

// x[j] = -inf where the grammar's table row forbids token j; 8 entries a load when aligned
// (V % 8 != 0 leaves every second state row unaligned)
__device__ __forceinline__ void mask_row(float* x, const short* __restrict__ nx, int V) {
  const bool al = (reinterpret_cast<uintptr_t>(nx) & 15) == 0;
  const int nv = al ? V / 8 : 0;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const uint4 u = reinterpret_cast<const uint4*>(nx)[i];
    const short* e = reinterpret_cast<const short*>(&u);
#pragma unroll
    for (int t = 0; t < 8; ++t)
      if (e[t] < 0) x[i * 8 + t] = -INFINITY;
  }
  for (int j = nv * 8 + threadIdx.x; j < V; j += blockDim.x)
    if (nx[j] < 0) x[j] = -INFINITY;
}

struct RowArgs {
  const long long* seed;    // [R]
  const long long* offset;  // [R]
  const long long* rngrow;  // [R]
  const float* min_p;       // [R] or null
  const int* bias_ptr;      // [R + 1] or null
  const int* bias_idx;
  const float* bias_val;
  const int* slot;          // [R] (-1: no state) or null
  const float* rp;          // [R] (with counts)
  const float* fp;
  const float* pp;
  int* counts;              // [S, V] or null
  int S;
  int pre;                  // logits already hold the processed x: only the state updates are left
  const long long* g_table; // [R] device address of the row's int16 next[S][V], 0 = unguided; or null
  const int* g_slot;        // [R]
  int* g_state;             // [G] automaton state per slot
  int G;
};

// the table row of this logits row's automaton state (null: unguided); *gslot = its state slot
__device__ __forceinline__ const short* guided_row(const RowArgs& a, int row_i, int V,
                                                   int* gslot) {
  if (!a.g_table || !a.g_slot || !a.g_state) return nullptr;
  const long long addr = a.g_table[row_i];
  const int gs = a.g_slot[row_i];
  if (addr == 0 || gs < 0 || gs >= a.G) return nullptr;
  const int st = a.g_state[gs];
  if (st < 0) return nullptr;
  *gslot = gs;
  return reinterpret_cast<const short*>(addr) + static_cast<size_t>(st) * V;
}

template <typename T, int NPT>
__global__ void __launch_bounds__(kSampNT) sample_rows_kernel(
    const T* __restrict__ logits, const float* __restrict__ temperature,
    const float* __restrict__ top_p, const int* __restrict__ top_k, RowArgs a,
    long long* __restrict__ out_tok, float* __restrict__ out_lp, float* __restrict__ out_tau,
    int V) {
  __shared__ float red[kSampNT / 64];
  __shared__ int redi[kSampNT / 64];
  __shared__ unsigned hc[256];
  __shared__ unsigned long long hm[256];
  __shared__ unsigned long long red64[kSampNT / 64];
  __shared__ int sel_b;
  __shared__ unsigned long long sel_need;
  extern __shared__ __attribute__((aligned(16))) float zlds[];
  const int row_i = blockIdx.x;
  const float temp = temperature[row_i];
  const bool greedy = !(temp > 0.f);
  Row<T, NPT> row;
  row.p = logits + static_cast<size_t>(row_i) * V;
  row.V = V;
  row.invT = greedy ? 1.f : 1.f / temp;
  row.zl = zlds;
  int slot = (a.slot && a.counts) ? a.slot[row_i] : -1;
  if (slot >= a.S) slot = -1;
  int gslot = -1;
  const short* gt = guided_row(a, row_i, V, &gslot);  // uniform over the workgroup
  if constexpr (NPT > 0) {
    const int b0 = (a.bias_ptr && !a.pre) ? a.bias_ptr[row_i] : 0;
    const int b1 = (a.bias_ptr && !a.pre) ? a.bias_ptr[row_i + 1] : 0;
    const bool pen = slot >= 0 && !a.pre;
    const bool msk = gt != nullptr && !a.pre;
    const bool proc = pen || b1 > b0 || msk;  // uniform over the workgroup
    // the fill of sampling.hip; a processed row is filled unscaled and scaled after step 2
    const float fs = proc ? 1.f : row.invT;
    constexpr int E = 16 / static_cast<int>(sizeof(T));
    const bool al = (reinterpret_cast<uintptr_t>(row.p) & 15) == 0;
    const int nv = al ? V / E : 0;
    for (int i0 = threadIdx.x; i0 < nv; i0 += 4 * kSampNT) {
      uint4 u[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = min(i0 + q * kSampNT, nv - 1);  // clamped: unconditional loads
        u[q] = reinterpret_cast<const uint4*>(row.p)[i];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = i0 + q * kSampNT;
        if (i < nv) {
          const T* e = reinterpret_cast<const T*>(&u[q]);
#pragma unroll
          for (int t = 0; t < E; ++t) zlds[i * E + t] = to_f32(e[t]) * fs;
        }
      }
    }
    for (int j = nv * E + threadIdx.x; j < V; j += kSampNT) zlds[j] = to_f32(row.p[j]) * fs;
    __syncthreads();
    if (proc) {
      if (msk) {
        mask_row(zlds, gt, V);
        __syncthreads();
      }
      if (b1 > b0) {
        add_bias(zlds, V, a.bias_idx, a.bias_val, b0, b1);
        __syncthreads();
      }
      if (pen) {
        penalize_row(zlds, a.counts + static_cast<size_t>(slot) * V, V, a.rp[row_i], a.fp[row_i],
                     a.pp[row_i], row.invT);
      } else {
        for (int j = threadIdx.x; j < V; j += kSampNT) zlds[j] *= row.invT;
      }
      __syncthreads();
    }
  }
  float m = -INFINITY;
  row.each([&](int, float z) { m = fmaxf(m, z); });
  const float tmax = m;  // this thread's own maximum
  m = block_max<kSampNT>(m, red);
  float s = 0.f;
  row.each([&](int, float z) { s += __expf(z - m); });
  const float Z = block_sum<kSampNT>(s, red);
  uint32_t tau = 0;  // keep key >= tau (0: everything)
  if (!greedy) {
    const int k = top_k[row_i];
    if (k > 0 && k < V) {
      uint32_t lo = 0;
      if (k <= kSampNT && V >= kSampNT) lo = fkey(-block_max<kSampNT>(-tmax, red));
      tau = radix_select<T, NPT, false>(row, m, lo, static_cast<unsigned long long>(k), hc, hm,
                                        &sel_b, &sel_need);
    }
    const float p = top_p[row_i];
    if (p < 1.f) {
      unsigned long long zk = 0;
      row.each([&](int, float z) {
        if (fkey(z) >= tau) zk += static_cast<unsigned long long>(__expf(z - m) * 4294967296.f);
      });
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_xor(static_cast<unsigned>(zk), o, 64);
        const unsigned hi = __shfl_xor(static_cast<unsigned>(zk >> 32), o, 64);
        zk += (static_cast<unsigned long long>(hi) << 32) | lo;
      }
      if ((threadIdx.x & 63) == 0) red64[threadIdx.x >> 6] = zk;
      __syncthreads();
      zk = 0;
#pragma unroll
      for (int w = 0; w < kSampNT / 64; ++w) zk += red64[w];
      __syncthreads();
      const double tgt = static_cast<double>(fmaxf(p, 0.f)) * static_cast<double>(zk);
      unsigned long long need = static_cast<unsigned long long>(ceil(tgt));
      if (need < 1) need = 1;
      if (need > zk) need = zk;
      const uint32_t tp =
          radix_select<T, NPT, true>(row, m, tau, need, hc, hm, &sel_b, &sel_need);
      tau = tp > tau ? tp : tau;
    }
    // min_p: p_j >= min_p * p_max  <=>  z_j >= m + ln(min_p), whatever top-k / top-p removed
    const float mp = a.min_p ? a.min_p[row_i] : 0.f;
    if (mp > 0.f) {
      const uint32_t tm = fkey(mp >= 1.f ? m : m + logf(mp));
      tau = tm > tau ? tm : tau;
    }
  }
  // argmax over the kept set (with Gumbel noise unless greedy)
  float best = -INFINITY;
  int bi = 0x7fffffff;
  const uint32_t sd = static_cast<uint32_t>(a.seed[row_i]) ^
                      (static_cast<uint32_t>(a.offset[row_i]) * 0x9E3779B9u + 0x7F4A7C15u);
  const uint64_t base = static_cast<uint64_t>(a.rngrow[row_i]) * static_cast<uint64_t>(V);
  row.each([&](int j, float z) {
    if (fkey(z) < tau) return;
    float key = z;
    if (!greedy) {
      const uint32_t r = rng_u32(sd, base + j);
      const float u = (static_cast<float>(r >> 8) + 0.5f) * (1.f / 16777216.f);
      key = z - __logf(-__logf(u));
    }
    if (key > best || (key == best && j < bi)) { best = key; bi = j; }
  });
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) { red[wid] = best; redi[wid] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float b = red[0];
    int idx = redi[0];
    for (int w = 1; w < kSampNT / 64; ++w)
      if (red[w] > b || (red[w] == b && redi[w] < idx)) { b = red[w]; idx = redi[w]; }
    if (idx >= V) idx = 0;
    out_tok[row_i] = idx;
    float zi;
    if constexpr (NPT > 0) zi = zlds[idx]; else zi = row.ld(idx);
    if (out_lp) out_lp[row_i] = zi - m - __logf(Z);
    if (out_tau) out_tau[row_i] = tau ? keyf(tau) : -INFINITY;
    if (slot >= 0) {
      int* c = a.counts + static_cast<size_t>(slot) * V + idx;
      *c = *c + 1;
    }
    if (gt) {
      const int n = gt[idx];
      if (n >= 0) a.g_state[gslot] = n;
    }
  }
}

// Steps 1-2 of the header, materialised: out[r, :] = processed f32 x of row r.
template <typename T>
__global__ void __launch_bounds__(kSampNT) logits_process_kernel(
    const T* __restrict__ logits, RowArgs a, float* __restrict__ out, int V) {
  const int row_i = blockIdx.x;
  const T* p = logits + static_cast<size_t>(row_i) * V;
  float* x = out + static_cast<size_t>(row_i) * V;
  int gslot = -1;
  const short* gt = guided_row(a, row_i, V, &gslot);
  if (gt) {
    for (int j = threadIdx.x; j < V; j += kSampNT) x[j] = gt[j] < 0 ? -INFINITY : to_f32(p[j]);
  } else {
    for (int j = threadIdx.x; j < V; j += kSampNT) x[j] = to_f32(p[j]);
  }
  int slot = (a.slot && a.counts) ? a.slot[row_i] : -1;
  if (slot >= a.S) slot = -1;
  const int b0 = a.bias_ptr ? a.bias_ptr[row_i] : 0;
  const int b1 = a.bias_ptr ? a.bias_ptr[row_i + 1] : 0;
  if (b1 > b0) {
    __threadfence();
    __syncthreads();  // the row is written before other threads add to it
    add_bias(x, V, a.bias_idx, a.bias_val, b0, b1);
  }
  if (slot >= 0) {
    __threadfence();
    __syncthreads();
    penalize_row(x, a.counts + static_cast<size_t>(slot) * V, V, a.rp[row_i], a.fp[row_i],
                 a.pp[row_i], 1.f);
  }
}

// One workgroup per new slot: zero its count row, then scatter the sequence's ids (the first
// n_prompt OR in bit 31, the rest add 1).  Ids outside [0, V) are skipped.
__global__ void __launch_bounds__(kSampNT) sampler_state_init_kernel(
    int* __restrict__ counts, const int* __restrict__ slots, const int* __restrict__ ptr,
    const int* __restrict__ n_prompt, const int* __restrict__ ids, int S, int V) {
  const int i = blockIdx.x;
  const int slot = slots[i];
  if (slot < 0 || slot >= S) return;  // uniform over the workgroup
  int* c = counts + static_cast<size_t>(slot) * V;
  const bool al = (reinterpret_cast<uintptr_t>(c) & 15) == 0;
  const int nv = al ? V / 4 : 0;
  for (int q = threadIdx.x; q < nv; q += kSampNT)
    reinterpret_cast<int4*>(c)[q] = make_int4(0, 0, 0, 0);
  for (int j = nv * 4 + threadIdx.x; j < V; j += kSampNT) c[j] = 0;
  __threadfence();
  __syncthreads();
  const int e0 = ptr[i], e1 = ptr[i + 1], np = n_prompt[i];
  for (int e = e0 + threadIdx.x; e < e1; e += kSampNT) {
    const int t = ids[e];
    if (t < 0 || t >= V) continue;
    if (e - e0 < np) atomicOr(c + t, static_cast<int>(0x80000000u));
    else atomicAdd(c + t, 1);
  }
}

template <typename T>
hipError_t launch_sample_rows(const void* logits, const float* temperature, const float* top_p,
                              const int* top_k, const RowArgs& a, long long* out_tok,
                              float* out_lp, float* out_tau, int rows, int V, hipStream_t st) {
  dim3 grid(rows), block(kSampNT);
  const T* lg = static_cast<const T*>(logits);
  if (V <= kSampLdsV) {
    // the LDS row copy goes past the 64 KiB dynamic default (gfx950 has 160 KiB per CU)
    static bool attr_set = false;
    if (!attr_set) {
      const hipError_t e = hipFuncSetAttribute(
          reinterpret_cast<const void*>(&sample_rows_kernel<T, 1>),
          hipFuncAttributeMaxDynamicSharedMemorySize, kSampLdsV * static_cast<int>(sizeof(float)));
      if (e != hipSuccess) return e;
      attr_set = true;
    }
    hipLaunchKernelGGL((sample_rows_kernel<T, 1>), grid, block, V * sizeof(float), st, lg,
                       temperature, top_p, top_k, a, out_tok, out_lp, out_tau, V);
  } else {
    hipLaunchKernelGGL((sample_rows_kernel<T, 0>), grid, block, 0, st, lg, temperature, top_p,
                       top_k, a, out_tok, out_lp, out_tau, V);
  }
  return hipGetLastError();
}

}  // namespace lumen

// The fused path.  For V > 32768 the kernel applies neither bias nor penalties: the caller
// passes processed f32 logits (lumen_logits_process) with pre = 1.  counts may be null (no
// state): slot is then ignored.  g_table / g_slot / g_state (all three or none) guide rows; with
// pre = 1 the mask is not applied again and the state still advances.  out_tau as in lumen_sample.
extern "C" hipError_t lumen_sample_rows(
    int dtype, const void* logits, const float* temperature, const float* top_p,
    const int* top_k, const long long* seed, const long long* offset, const long long* rngrow,
    const float* min_p, const int* bias_ptr, const int* bias_idx, const float* bias_val,
    const int* slot, const float* rp, const float* fp, const float* pp, int* counts, int S,
    int pre, const long long* g_table, const int* g_slot, int* g_state, int G,
    long long* out_tok, float* out_lp, float* out_tau, int rows, int V, hipStream_t st) {
  if (rows == 0) return hipSuccess;
  if (V < 1 || !seed || !offset || !rngrow) return hipErrorInvalidValue;
  if (counts && slot && !pre && (!rp || !fp || !pp)) return hipErrorInvalidValue;
  if (g_table && (!g_slot || !g_state || G < 1)) return hipErrorInvalidValue;
  if (V > lumen::kSampLdsV && !pre && (bias_ptr || (counts && slot) || g_table))
    return hipErrorInvalidValue;  // the no-LDS form samples processed logits only
  const lumen::RowArgs a{seed, offset, rngrow, min_p, bias_ptr, bias_idx, bias_val, slot,
                         rp, fp, pp, counts, S, pre, g_table, g_slot, g_state, G};
  if (dtype == lumen::kF32)
    return lumen::launch_sample_rows<float>(logits, temperature, top_p, top_k, a, out_tok,
                                            out_lp, out_tau, rows, V, st);
  if (dtype == lumen::kBF16)
    return lumen::launch_sample_rows<lumen::bf16>(logits, temperature, top_p, top_k, a, out_tok,
                                                  out_lp, out_tau, rows, V, st);
  if (dtype == lumen::kF16)
    return lumen::launch_sample_rows<lumen::fp16>(logits, temperature, top_p, top_k, a, out_tok,
                                                  out_lp, out_tau, rows, V, st);
  return hipErrorInvalidValue;
}

extern "C" hipError_t lumen_logits_process(
    int dtype, const void* logits, const int* bias_ptr, const int* bias_idx,
    const float* bias_val, const int* slot, const float* rp, const float* fp, const float* pp,
    const int* counts, int S, const long long* g_table, const int* g_slot, const int* g_state,
    int G, float* out, int rows, int V, hipStream_t st) {
  if (rows == 0) return hipSuccess;
  if (V < 1) return hipErrorInvalidValue;
  if (counts && slot && (!rp || !fp || !pp)) return hipErrorInvalidValue;
  if (g_table && (!g_slot || !g_state || G < 1)) return hipErrorInvalidValue;
  const lumen::RowArgs a{nullptr, nullptr, nullptr, nullptr, bias_ptr, bias_idx, bias_val, slot,
                         rp, fp, pp, const_cast<int*>(counts), S, 0, g_table, g_slot,
                         const_cast<int*>(g_state), G};
  dim3 grid(rows), block(lumen::kSampNT);
  if (dtype == lumen::kF32)
    hipLaunchKernelGGL((lumen::logits_process_kernel<float>), grid, block, 0, st,
                       static_cast<const float*>(logits), a, out, V);
  else if (dtype == lumen::kBF16)
    hipLaunchKernelGGL((lumen::logits_process_kernel<lumen::bf16>), grid, block, 0, st,
                       static_cast<const lumen::bf16*>(logits), a, out, V);
  else if (dtype == lumen::kF16)
    hipLaunchKernelGGL((lumen::logits_process_kernel<lumen::fp16>), grid, block, 0, st,
                       static_cast<const lumen::fp16*>(logits), a, out, V);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

extern "C" hipError_t lumen_sampler_state_init(int* counts, const int* slots, const int* ptr,
                                               const int* n_prompt, const int* ids, int n, int S,
                                               int V, hipStream_t st) {
  if (n == 0) return hipSuccess;
  if (V < 1 || S < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(lumen::sampler_state_init_kernel, dim3(n), dim3(lumen::kSampNT), 0, st,
                     counts, slots, ptr, n_prompt, ids, S, V);
  return hipGetLastError();
}
