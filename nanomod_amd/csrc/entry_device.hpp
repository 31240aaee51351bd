// Device-side helpers that the per-position kernels (K8, K9, K10, K14), the per-read kernels (K11 .. K13) and the q-value kernels share
// (their host half: entry_common.hpp; the classed position walk: pos_walk.hpp; the read walk: read_walk.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wave_ops.hpp"

namespace nmod {

__device__ __forceinline__ double nan_f64() { return __longlong_as_double(0x7FF8000000000000ll); }

// row i of a CSR (off) or fixed-stride batch: its first sample and its length (offsets that decrease: an empty row)
__device__ __forceinline__ void csr_row(const int64_t* off, int64_t stride, int64_t i, int64_t& begin, int64_t& n) {
  if (off) { begin = off[i]; n = off[i + 1] - begin; } else { begin = i * stride; n = stride; }
  if (n < 0) n = 0;
}

// whether any of the G lanes of the caller's group (a row of 16, or the wave) has the flag
template <int G>
__device__ __forceinline__ bool group_any(bool f, int lane) {
  const unsigned long long b = __ballot(f);
  if constexpr (G == 64) return b != 0ull;
  else return ((b >> (lane & 48)) & 0xFFFFull) != 0ull;
}

// sum over the G lanes of the caller's group (a row of 16, or the wave), the same bits in every lane of it (every step adds the
// two halves in both orders).  Reached by whole waves.
template <int G>
__device__ __forceinline__ double group_sum_f64(double v) {
  if constexpr (G == 64) {
    return wave_sum_f64(v);
  } else {
    static_assert(G == 16, "group_sum_f64: a row or the wave");
    auto step = [](double x, auto tag) {
      constexpr int C = decltype(tag)::value;
      long long b = __double_as_longlong(x);
      int lo = dpp_i<C>(0, (int)(unsigned)b);
      int hi = dpp_i<C>(0, (int)(unsigned)((unsigned long long)b >> 32));
      return x + __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
    };
    v = step(v, std::integral_constant<int, NMOD_QP(1, 0, 3, 2)>{});
    v = step(v, std::integral_constant<int, NMOD_QP(2, 3, 0, 1)>{});
    v = step(v, std::integral_constant<int, kDppRowHalfMirror>{});
    v = step(v, std::integral_constant<int, kDppRowMirror>{});
    return v;
  }
}

// Appends i to the work list of its class (cls < 0: to none): the lanes of a class are ballot-compacted, one atomic per wave
// and class on the class's count word.  Reached by whole waves.
template <int NC>
__device__ __forceinline__ void compact_to_lists(int cls, int lane, uint32_t* const (&list)[NC], uint32_t* count, int64_t i) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const unsigned long long mask = __ballot(cls == c);
    if (mask) {
      unsigned at = 0;
      if (lane == 0) at = atomicAdd(&count[c], (unsigned)__popcll(mask));
      at = __builtin_amdgcn_readfirstlane(at);
      if (cls == c) list[c][at + (unsigned)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)i;
    }
  }
}

// sum over a workgroup of WAVES waves, the same bits in every thread: wave sums, then the waves' words in index order.
// sh: WAVES words, free to hold anything else before the call; the caller orders its next use of them after the reads here
// (the leading barrier of the next sum does)
template <int WAVES>
__device__ __forceinline__ double block_sum_f64(double v, double* sh) {
  const double w = wave_sum_f64(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) t += sh[i];
  return t;
}

}  // namespace nmod
