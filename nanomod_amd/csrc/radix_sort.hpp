// Stable LSD radix sort of (uint64 key, uint32 value) pairs on the device — the sort behind nmod_rank_order / nmod_region_rank
// (Python's stable sorted() over the result records).  Hand-written (round 5; rounds 2-4 called rocPRIM's
// radix_sort_pairs here): eight passes of one byte, each
//   rs_hist_kernel     a block per tile of 2 048 pairs: the tile's digit histogram (LDS atomics) -> hist[digit][tile]
//   rs_scan_*          exclusive prefix sums over hist in (digit, tile) order: where each tile's run of each digit starts
//   rs_scatter_kernel  the tile again, eight rounds of 256 pairs in index order: a pair's place = start of its tile's run of its
//                      digit + the pairs of that digit in the tile's earlier rounds + those of lower lanes / waves in this round
//                      (eight ballots match the lanes of a wave that hold the same digit; a count per wave and digit in LDS)
// Equal digits keep their order (tile, round, thread = index order), so the pass is stable and so is the sort.  Eight passes:
// the result is back in the buffers it started in.  Not the timed hot path: 10 M pairs take a few milliseconds per pass.
//
// The kernels and rs_sort_pairs are compiled once, in radix_sort.hip; this header holds the tile constants, the scratch sizes
// and the declaration, which is all that the units that sort (the rankings, the read pivot, the q-values, the k-mer tables, the
// site pairs) need.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace nmod {

constexpr int kRsThreads = 256;
constexpr int kRsItems = 8;
constexpr int kRsTile = kRsThreads * kRsItems;                 // pairs per block
constexpr int kRsScanChunk = 4096;                             // histogram entries per block of the scan kernels

// Scratch the sort needs beside the two pairs of buffers: the histogram (256 entries per tile) and the scan's chunk sums.
inline int64_t rs_tiles(int64_t n) { return (n + kRsTile - 1) / kRsTile; }
inline size_t rs_scratch_bytes(int64_t n) {
  const int64_t m = 256 * rs_tiles(n);
  return (size_t)(m + (m + kRsScanChunk - 1) / kRsScanChunk + 1) * 4;
}
// keys / vals: the pairs, sorted in place (ascending keys, stable); keys_tmp / vals_tmp: as large.  n < 2^31.
// passes < 8: only the low `passes` bytes of the keys are sorted by (the others must be equal); after an odd number of passes
// the result is in keys_tmp / vals_tmp.
hipError_t rs_sort_pairs(uint64_t* keys, uint32_t* vals, uint64_t* keys_tmp, uint32_t* vals_tmp, int64_t n, void* scratch, hipStream_t stream,
                         int passes = 8);

}  // namespace nmod
