// What the entries that walk the reads over a list of candidate sites share (K16 nmod_site_pairs, K18's nmod_pair_rows entries in
// site_pairs.hip; K19 nmod_read_sites_count / nmod_read_hmm in read_hmm.hip): the search of the sites a read covers, the read's score at a
// site with the strand-aware event index, the one-workgroup exclusive scan of int64 counts, and the host checks of the shared arguments.
// One copy; nothing here multiplies and adds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nanomod_hip.h"
#include "read_walk.hpp"

namespace nmod {

constexpr int64_t kSpPosMask = ((int64_t)1 << 40) - 1;
constexpr int kSpScanPer = 8, kSpScanChunk = 256 * kSpScanPer;

// the first index in [lo, hi) whose key is >= k (UPPER: > k)
template <bool UPPER>
__device__ __forceinline__ int64_t sp_bound(const int64_t* key, int64_t lo, int64_t hi, int64_t k) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int64_t v = key[mid];
    if (UPPER ? v <= k : v < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// poff[0, nsites): the counts, replaced by their exclusive scan; poff[nsites]: their sum.  One workgroup, a chunk at a time
static __global__ __launch_bounds__(256) void sp_scan_kernel(int64_t* poff, int64_t nsites) {
  __shared__ int64_t sh[256];
  const int tid = threadIdx.x;
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < nsites; c0 += kSpScanChunk) {
    const int64_t base = c0 + (int64_t)tid * kSpScanPer;
    int64_t v[kSpScanPer], s = 0;
#pragma unroll
    for (int e = 0; e < kSpScanPer; ++e) { v[e] = base + e < nsites ? poff[base + e] : 0; s += v[e]; }
    sh[tid] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int64_t t = tid >= d ? sh[tid - d] : 0;
      __syncthreads();
      sh[tid] += t;
      __syncthreads();
    }
    int64_t ex = carry + sh[tid] - s;
    carry += sh[255];
#pragma unroll
    for (int e = 0; e < kSpScanPer; ++e) { if (base + e < nsites) poff[base + e] = ex; ex += v[e]; }
    __syncthreads();                                            // sh is read before the next chunk writes it
  }
  if (tid == 0) poff[nsites] = carry;
}

// One read as the walk hands it to its callers: where its events lie and its scores
struct SpRead {
  int64_t read, start, n; bool minus; const double* sc; const int64_t* key;
  // the score of the read's event at site s; false: no event of this read (keys that do not ascend)
  __device__ __forceinline__ bool score_at(int64_t s, double& l) const {
    const int64_t pos = key[s] & kSpPosMask;
    const int64_t i = minus ? start + n - 1 - pos : pos - start;
    if (i < 0 || i >= n) return false;
    l = sc[i];
    return true;
  }
};

static bool sp_keys_ascend(const int64_t* key, int64_t n) {
  for (int64_t i = 0; i < n; ++i) if (key[i] < 0 || (i > 0 && key[i] <= key[i - 1])) return false;
  return true;
}

// The checks of the reads, the sites and the pair index that the entries which walk the reads share (nmod_site_pairs, the two
// nmod_pair_rows entries; without a pair index, poff NULL and npairs 0, the two K19 entries), before any device work
static bool sp_walk_args_ok(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff, const double* score,
                            int64_t nsites, const int64_t* key, const int64_t* poff, int64_t npairs) {
  if (nreads < 0 || nreads > (int64_t)INT32_MAX) return false;
  if (nsites < 0 || nsites > (int64_t)INT32_MAX - 1 || npairs < 0 || npairs > (int64_t)INT32_MAX) return false;
  if (nreads > 0 && (!cs || !start || !roff)) return false;
  if ((nsites > 0 && !key) || (npairs > 0 && (!poff || nsites < 2))) return false;
  if (prm->memspace == NMOD_MEM_HOST) {
    if (nreads > 0 && !csr_offsets_ok(roff, nreads)) return false;
    if (nreads > 0 && roff[nreads] > 0 && !score) return false;
    if (!sp_keys_ascend(key, nsites)) return false;
    if (poff && (poff[0] != 0 || !csr_offsets_ok(poff, nsites) || poff[nsites] != npairs)) return false;
    if (!poff && npairs != 0) return false;
  } else if (nreads > 0 && !score) {
    return false;
  }
  return true;
}

}  // namespace nmod
