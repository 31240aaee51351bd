// The events of a read, for the kernels that walk them (K11 nmod_rescale_reads, K12 nmod_read_calls, K13 nmod_read_llr): the value of an
// event as a double, the 2-bit code of a base, and the k-mer code rolled over a run of consecutive events.  The walk itself — lists,
// draw, tiles, launches — is read_walk.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nanomod_hip.h"

namespace nmod {

constexpr int kRsRun = 8;                         // consecutive events per lane and step

template <int DT>
__device__ __forceinline__ double rs_load(const void* p, int64_t i) {
#pragma clang fp contract(off)
  if constexpr (DT == NMOD_DTYPE_F32) return (double)static_cast<const float*>(p)[i];
  else if constexpr (DT == NMOD_DTYPE_I16_MILLI) return (double)static_cast<const int16_t*>(p)[i] / 1000.0;
  else return static_cast<const double*>(p)[i];
}

__device__ __forceinline__ int rs_base2(unsigned c) { return c == 'A' ? 0 : (c == 'C' ? 1 : (c == 'G' ? 2 : (c == 'T' ? 3 : -1))); }

// f(j, code) for the events j0 .. j0 + 7 (those below n) of a read whose bases start at b: the code rolls over the bytes
// j0 - center .. j0 + 7 + k - 1 - center; `run` counts the valid bases that end at the current byte
template <class F>
__device__ __forceinline__ void rs_run(const uint8_t* b, int64_t n, int64_t j0, int k, int center, F&& f) {
  const unsigned mask = (1u << (2 * k)) - 1u;             // k <= 8
  unsigned code = 0;
  int run = 0;
  for (int i = 0; i < kRsRun + k - 1; ++i) {
    const int64_t p = j0 - center + i;
    const int v = (p >= 0 && p < n) ? rs_base2(b[p]) : -1;
    code = ((code << 2) | (unsigned)(v & 3)) & mask;
    run = v >= 0 ? run + 1 : 0;
    if (i >= k - 1) {
      const int64_t j = j0 + i - (k - 1);
      if (j < n) f(j, run >= k ? (int)code : -1);
    }
  }
}

}  // namespace nmod
