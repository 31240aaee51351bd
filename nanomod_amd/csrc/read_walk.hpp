// The scaffold that the kernels which walk reads share (K11 nmod_rescale_reads, K12 nmod_read_calls / nmod_site_calls, K13 nmod_read_llr /
// nmod_site_llr; the events of a read themselves: read_events.hpp).  One copy of: the two work lists and the kernel that fills them, the
// ticket draw of the persistent grids, the wave-local LDS sync, the tile geometry of the windowed kernels, the NaN fill of a read that
// is too large, the per-read integer counts, the launch of the two forms, the host checks of the entries, and the per-position row walk.
// What differs — the tables, the arithmetic per event, the caps and LDS cutoffs — stays with each kernel.  Nothing here multiplies and
// adds: contraction is the callers' concern.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "entry_device.hpp"
#include "read_events.hpp"
#include "special_math.hpp"

namespace nmod {

constexpr int kRwThreads = 256;
constexpr int kRwWaves = kRwThreads / 64;
constexpr int kRwTile = 64 * kRsRun;              // events a wave stages at a time (K12, K13)
static_assert(NMOD_RESCALE_WAVE_MAX == NMOD_CALLS_WAVE_MAX, "one class limit for the three entries");
constexpr int64_t kRwWaveMax = NMOD_CALLS_WAVE_MAX;   // a read of up to this many events takes a wave (list 0), a longer one a workgroup (list 1)

// the reads of each class, in the order the classify kernel's waves appended them
struct ReadLists {
  uint32_t* list[2]; uint32_t* count;             // count[0 .. 1]: the lists' lengths, count[2 .. 3]: their ticket words
};

// a thread per read: the read's class by its length, ballot-compacted into one list per class
static __global__ __launch_bounds__(256) void read_classify_kernel(const int64_t* off, int64_t nreads, int64_t wave_max, ReadLists w) {
  const int lane = threadIdx.x & 63;
  for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < nreads; b0 += (int64_t)gridDim.x * 256) {
    const int64_t i = b0 + threadIdx.x;
    int cls = -1;
    if (i < nreads) {
      int64_t b, n;
      csr_row(off, 0, i, b, n);
      cls = n <= wave_max ? 0 : 1;
    }
    compact_to_lists<2>(cls, lane, w.list, w.count, i);
  }
}

// Host: the lists' share of a call's slab — taken before slab.commit — and, after it, the lists themselves: the pointers, the zeroed
// count and ticket words, and the classify launch on the call's stream.
struct ReadListSpace {
  size_t o_list, o_count;
  ReadListSpace(Slab& slab, size_t nreads) : o_list(slab.take(nreads * 4 * 2)), o_count(slab.take(16)) {}
  // (wave_max: the class step in rows of `off`; K19 classes the reads by their entries, not their events)
  hipError_t fill(const Slab& slab, const int64_t* off, int64_t nreads, int num_cus, hipStream_t stream, ReadLists& w,
                  int64_t wave_max = kRwWaveMax) const {
    w.list[0] = slab.at<uint32_t>(o_list); w.list[1] = w.list[0] + nreads;
    w.count = slab.at<uint32_t>(o_count);
    const hipError_t e = hipMemsetAsync(w.count, 0, 16, stream);
    if (e != hipSuccess) return e;
    const int64_t cb = (nreads + 255) / 256, ccap = (int64_t)num_cus * 16;
    hipLaunchKernelGGL(read_classify_kernel, dim3((unsigned)(cb < ccap ? cb : ccap)), dim3(256), 0, stream, off, nreads, wave_max, w);
    return hipSuccess;
  }
};

// The next item of the caller's list off its ticket word (WAVES == 1: a wave per read, list 0 and count[2]; else the workgroup per read,
// list 1 and count[3]); the list is used up when the item reaches its length.  Reached by whole waves / the whole workgroup.
// Wave form: every lane takes part in the draw and lane 0 alone adds one: the broadcast below is then reached by the whole wave on
// every path.  (Under `if (lane == 0)` the draw would share its condition with the stores of `if (t == 0)` at the end of the callers'
// bodies, and a compiler that threads the two lets the other lanes reach the broadcast without lane 0.)
// Workgroup form: sh_item is a shared word of the caller's; the leading barrier ends the last read's uses of it and of every other
// shared word of the caller (its count and sum words), so the body may write those without a barrier of its own.
template <int WAVES>
__device__ __forceinline__ unsigned draw_read(const ReadLists& w, unsigned& sh_item) {
  uint32_t* ticket = &w.count[WAVES == 1 ? 2 : 3];
  if constexpr (WAVES == 1) {
    const unsigned got = atomicAdd(ticket, (threadIdx.x & 63) == 0 ? 1u : 0u);
    return (unsigned)__builtin_amdgcn_readlane((int)got, 0);
  } else {
    __syncthreads();
    if (threadIdx.x == 0) sh_item = atomicAdd(ticket, 1u);
    __syncthreads();
    return sh_item;
  }
}

// the stores of a wave to its LDS tile are visible to its own later loads, and the other way round
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Tiles of a windowed read (K12, K13).  A wave stages kRwTile consecutive events; the first halo_events(nb_lo) and the last
// halo_events(nb_hi) of them are the window halo, recomputed by the neighbouring tiles, and the `inner` = kRwTile - the two halos between
// them are the tile's own (384 .. 512).
__device__ __forceinline__ int halo_events(int nb) { return kRsRun * ((nb + kRsRun - 1) / kRsRun); }   // whole runs: 0 .. 64
// tile ti of a read of n events: its own events are a0 .. a1 - 1, the staged ones start at s0 (below 0 in the first tile)
__device__ __forceinline__ void tile_span(int64_t ti, int inner, int halo_lo, int64_t n, int64_t& a0, int64_t& s0, int64_t& a1) {
  a0 = ti * inner; s0 = a0 - halo_lo;
  a1 = a0 + inner < n ? a0 + inner : n;
}
// the window of event j, clipped to the read: j + lo .. j + hi
__device__ __forceinline__ void window_bounds(int64_t j, int64_t n, int nb_lo, int nb_hi, int& lo, int& hi) {
  lo = j < nb_lo ? -(int)j : -nb_lo;
  hi = n - 1 - j < nb_hi ? (int)(n - 1 - j) : nb_hi;
}

// the event tracks of a read that is too large (those asked for): NaN, by thread t of the read's T
__device__ __forceinline__ void nan_fill(double* p0, double* p1, double* p2, int64_t begin, int64_t n, int t, int T) {
  const double nan = nan_f64();
  for (int64_t j = t; j < n; j += T) {
    if (p0) p0[begin + j] = nan;
    if (p1) p1[begin + j] = nan;
    if (p2) p2[begin + j] = nan;
  }
}

// The integer counts c... of a read summed over its threads, each in place and in every thread: wave sums, then (WAVES > 1) the waves'
// words through sh_cnt (kRwWaves words per count, the i-th count's at kRwWaves * i: the folds run left to right; their last readers
// are ordered before the next write by draw_read's barrier)
template <int WAVES, class... C>
__device__ __forceinline__ void read_counts(int* sh_cnt, C&... c) {
  ((c = (int)wave_sum_u64((unsigned long long)c)), ...);
  if constexpr (WAVES > 1) {
    int i = 0;
    if ((threadIdx.x & 63) == 0) ((sh_cnt[kRwWaves * i++ + (threadIdx.x >> 6)] = c), ...);
    __syncthreads();
    ((c = 0), ...);
#pragma unroll
    for (int v = 0; v < WAVES; ++v) { i = 0; ((c += sh_cnt[kRwWaves * i++ + v]), ...); }
  }
}

// Host: the two forms of a read kernel, one after the other on the stream, under one cap of workgroups: the dtype and whether the table
// lives in LDS pick the instance.  K: a type whose `template <int DT, int WAVES, bool LDS_TAB> static auto kernel()` names the kernel
template <class K, int DT, bool LDS_TAB, class Args>
static void launch_read_forms(const Args& a, int64_t cap, size_t lds_bytes, hipStream_t stream) {
  hipLaunchKernelGGL((K::template kernel<DT, 1, LDS_TAB>()), dim3(persistent_grid(a.nreads, kRwWaves, cap)), dim3(kRwThreads), lds_bytes, stream, a);
  hipLaunchKernelGGL((K::template kernel<DT, kRwWaves, LDS_TAB>()), dim3(persistent_grid(a.nreads, 1, cap)), dim3(kRwThreads), lds_bytes, stream, a);
}
template <class K, bool LDS_TAB, class Args>
static void launch_read_kernels(const Args& a, int32_t dtype, int64_t cap, size_t lds_bytes, hipStream_t stream) {
  for_dtype(dtype, [&](auto dt) { launch_read_forms<K, decltype(dt)::value, LDS_TAB>(a, cap, lds_bytes, stream); });
}

// Host checks of the entries, in the order they have always run: the count of reads, the model's k and center ...
inline bool read_count_ok(int64_t nreads) { return nreads >= 0 && nreads <= (int64_t)UINT32_MAX - 1; }
inline bool kmer_model_ok(const nmod_rescale_model* m) { return m && m->k >= 1 && m->k <= 8 && m->center >= 0 && m->center < m->k; }
// ... and, after the entry's own, rows_begin (entry_common.hpp): the offsets of a host call, then the device

// Per-position counts over rows of pivoted scores (nmod_site_calls, nmod_site_llr): a wave per row, rows strided over the grid's waves.
// Rule: N counters (the first is n_valid), `count(score, c)` adds one score to them, `frac(c)` is the row's fraction from the totals
template <class Rule>
struct SiteOut { int32_t* n[Rule::N]; double* frac; };

template <class Rule>
static __global__ __launch_bounds__(256) void site_kernel(const double* score, const int64_t* off, int64_t stride, int64_t npos, Rule rule,
                                                          SiteOut<Rule> out) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < npos; row += (int64_t)gridDim.x * 4) {
    int64_t begin, n;
    csr_row(off, stride, row, begin, n);
    unsigned long long c[Rule::N] = {};
    for (int64_t j = lane; j < n; j += 64) rule.count(score[begin + j], c);
#pragma unroll
    for (int i = 0; i < Rule::N; ++i) c[i] = wave_sum_u64(c[i]);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < Rule::N; ++i) if (out.n[i]) out.n[i][row] = (int32_t)c[i];
      if (out.frac) out.frac[row] = rule.frac(c);
    }
  }
}

// the body of a site entry after the checks of its own out struct and threshold
template <class Rule>
static int site_counts(const nmod_params* prm, int64_t npos, const double* score, const int64_t* off, Rule rule, SiteOut<Rule> out) {
  if (npos < 0 || npos > (int64_t)INT32_MAX - 1) return NMOD_ERR_INVALID_ARG;
  if (!off && prm->stride0 <= 0) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && !score) return NMOD_ERR_INVALID_ARG;
  int num_cus = 0;
  const int rc = rows_begin(prm, npos, off, &num_cus);
  if (rc != NMOD_OK || npos == 0) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  const size_t np = (size_t)npos;
  const size_t tot = !host ? 0 : (off ? (size_t)off[npos] : np * (size_t)prm->stride0);

  Slab slab(host);
  slab.in(off, (np + 1) * 8); slab.in(score, tot * 8);
  for (int i = 0; i < Rule::N; ++i) slab.out(out.n[i], np * 4);
  slab.out(out.frac, np * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  hipLaunchKernelGGL(site_kernel<Rule>, dim3(persistent_grid(npos, 4, (int64_t)num_cus * 8)), dim3(256), 0, stream, score, off,
                     off ? 0 : prm->stride0, npos, rule, out);
  return launches_end(slab, stream);
}

}  // namespace nmod
