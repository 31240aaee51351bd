// Read-level input of `detect` on the device: nmod_pivot_reads, nmod_select_tested, nmod_gather_tested (include/nanomod_hip.h).
//
// The reference appends every event of every aligned read to its position's list (mReadSignalBase, myDetect.py:104-124), then
// drops thin positions (mfilter_coverage, myDetect.py:301-314) and tests the positions both groups share in sorted order
// (myDetect.py:421,427-431).  Here a read set is flat arrays (per read: (chrom, strand) id `cs`, start, CSR offsets into the
// events; per event: value and base) and the three entries build the tested CSR rows on the device:
//
//   pivot   rp_check_kernel     per read: validate, clip to [pos_lo, pos_hi], per-cs min / max covered position (atomics)
//           (host)              one round trip: the dense coordinate d = cbase[cs] + pos - cmin[cs] of every covered position
//           rp_diff_kernel      per read: +1 / -1 at the ends of its covered range (a read adds one sample per position)
//           scans               samples per d, row index of every covered d, sample offset of every d
//           rp_rows_kernel      per covered d: key (cs << 40 | pos) and row offset
//           rp_place_kernel     a wave per read: every event takes a slot of its row (atomic cursor) and stores its event index
//           rp_order_kernel     a wave per row of <= kSmallRow samples: the row's event indices ranked in LDS (events are in read
//                               order, so ascending event index = read append order), values and the last read's base written
//                               in that order; larger rows go to a list
//           large rows          one stable radix sort of (list slot << 32 | event index) over all of them (radix_sort.hpp), then
//                               the same placement
//   select  rp_match_kernel     per row of group 1: coverage of both groups, binary search of its key in group 2's keys
//           scans + compaction  tested rows of both groups, their new offsets; a device reduction picks the output dtype
//   gather  rp_gather_kernel    the tested rows in the output dtype; keys, bases and run ids (detect.run_ids) of the tested rows
//
// Atomic slot order differs from run to run; the ranking pass makes the output bytes independent of it.
// Only plain C++ stores and atomics write memory.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <vector>
#include <type_traits>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "radix_sort.hpp"

namespace nmod {
namespace {

constexpr int kPosBits = 40;
constexpr int64_t kPosLimit = (int64_t)1 << kPosBits;
constexpr int kSmallRow = 1024;               // rows ranked in LDS by one wave; larger ones take the radix sort
constexpr int kWaves = 4;                     // waves per block of the per-read / per-row kernels
constexpr int kScanPer = 16, kScanChunk = 256 * kScanPer;
constexpr int64_t kDeviceEncodeAbove = 4000000;   // detect.DEVICE_ENCODE_ABOVE: float64 batches above it pass through

inline unsigned grid_for(int64_t n, int64_t per_block) { return persistent_grid(n, per_block, 65536); }

// ---------------------------------------------------------------------------------------------------- int64 scans
enum { kScanId = 0, kScanNonzero = 1 };
template <int M> __device__ __forceinline__ int64_t scan_in(const int64_t* a, int64_t i) {
  const int64_t v = a[i];
  return M == kScanNonzero ? (int64_t)(v > 0) : v;
}
__device__ __forceinline__ int64_t block_exscan(int64_t v, int64_t* sh, int64_t& total) {     // 256 threads
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int64_t add = threadIdx.x >= (unsigned)d ? sh[threadIdx.x - d] : 0;
    __syncthreads();
    sh[threadIdx.x] += add;
    __syncthreads();
  }
  total = sh[255];
  const int64_t incl = sh[threadIdx.x];
  __syncthreads();
  return incl - v;
}
template <int M> __global__ __launch_bounds__(256) void scan_reduce_kernel(const int64_t* a, int64_t n, int64_t* bsum) {
  __shared__ int64_t sh[256];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanPer;
  int64_t s = 0;
  for (int e = 0; e < kScanPer; ++e) s += base + e < n ? scan_in<M>(a, base + e) : 0;
  int64_t total;
  block_exscan(s, sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
__global__ __launch_bounds__(256) void scan_tops_kernel(int64_t* bsum, int64_t nb, int64_t* total_out) {   // one block
  __shared__ int64_t sh[256];
  int64_t carry = 0;
  for (int64_t b0 = 0; b0 < nb; b0 += 256) {
    const int64_t i = b0 + threadIdx.x;
    const int64_t v = i < nb ? bsum[i] : 0;
    int64_t total;
    const int64_t ex = block_exscan(v, sh, total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0 && total_out) *total_out = carry;
}
// out may alias a: every thread reads its 16 entries before it writes them
template <int M, bool INCL> __global__ __launch_bounds__(256) void scan_apply_kernel(const int64_t* a, int64_t* out, int64_t n,
                                                                                     const int64_t* bsum) {
  __shared__ int64_t sh[256];
  const int64_t base = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * kScanPer;
  int64_t v[kScanPer], s = 0;
  for (int e = 0; e < kScanPer; ++e) { v[e] = base + e < n ? scan_in<M>(a, base + e) : 0; s += v[e]; }
  int64_t total;
  int64_t run = block_exscan(s, sh, total) + bsum[blockIdx.x];
  for (int e = 0; e < kScanPer; ++e) {
    if (base + e < n) out[base + e] = INCL ? run + v[e] : run;
    run += v[e];
  }
}
inline int64_t scan_blocks(int64_t n) { return (n + kScanChunk - 1) / kScanChunk; }
// exclusive (or inclusive) scan of a[0, n) (or of a[i] > 0) into out; the sum goes to *total_out (device) when given.
// bsum: scan_blocks(n) entries.
template <int M, bool INCL>
hipError_t scan_i64(const int64_t* a, int64_t* out, int64_t n, int64_t* bsum, int64_t* total_out, hipStream_t s) {
  const int64_t nb = scan_blocks(n);
  if (nb > 0) hipLaunchKernelGGL(scan_reduce_kernel<M>, dim3((unsigned)nb), dim3(256), 0, s, a, n, bsum);
  hipLaunchKernelGGL(scan_tops_kernel, dim3(1), dim3(256), 0, s, bsum, nb, total_out);
  if (nb > 0) hipLaunchKernelGGL((scan_apply_kernel<M, INCL>), dim3((unsigned)nb), dim3(256), 0, s, a, out, n, (const int64_t*)bsum);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------- pivot
// a read's covered positions after the event-level clip of myDetect.py:112-114 (inclusive; -1 = no bound)
__device__ __forceinline__ bool clip_span(int64_t s, int64_t n, int64_t pos_lo, int64_t pos_hi, int64_t& lo, int64_t& hi) {
  if (n <= 0) return false;
  lo = s; hi = s + n - 1;
  if (pos_lo >= 0 && lo < pos_lo) lo = pos_lo;
  if (pos_hi >= 0 && hi > pos_hi) hi = pos_hi;
  return lo <= hi;
}

__global__ __launch_bounds__(256) void rp_check_kernel(int64_t nreads, int32_t ncs, const int32_t* cs, const int64_t* start,
                                                       const int64_t* roff, int64_t nevents, int64_t pos_lo, int64_t pos_hi,
                                                       int* err, unsigned long long* cmin, unsigned long long* cmax) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nreads; r += (int64_t)gridDim.x * 256) {
    const int64_t a = roff[r], b = roff[r + 1], s = start[r];
    const int32_t c = cs[r];
    bool bad = (r == 0 && a != 0) || b < a || b > nevents || c < 0 || c >= ncs || s < 0 || s >= kPosLimit;
    if (!bad && b - a > kPosLimit - s) bad = true;                           // the read's last position beyond 2^40 - 1
    if (bad) { atomicOr(err, 1); continue; }
    int64_t lo, hi;
    if (clip_span(s, b - a, pos_lo, pos_hi, lo, hi)) {
      atomicMin(&cmin[c], (unsigned long long)lo);
      atomicMax(&cmax[c], (unsigned long long)hi);
    }
  }
}

__global__ __launch_bounds__(256) void rp_diff_kernel(int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                                      int64_t pos_lo, int64_t pos_hi, const int64_t* cmin, const int64_t* cbase,
                                                      unsigned long long* diff) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < nreads; r += (int64_t)gridDim.x * 256) {
    int64_t lo, hi;
    if (!clip_span(start[r], roff[r + 1] - roff[r], pos_lo, pos_hi, lo, hi)) continue;
    const int32_t c = cs[r];
    const int64_t d0 = cbase[c] + lo - cmin[c];
    atomicAdd(&diff[d0], 1ull);
    atomicAdd(&diff[d0 + (hi - lo) + 1], ~0ull);                           // -1
  }
}

__global__ __launch_bounds__(256) void rp_rows_kernel(int64_t S, int32_t ncs, const int64_t* cnt, const int64_t* rowid,
                                                      const int64_t* soff, const int64_t* cmin, const int64_t* cbase,
                                                      const int64_t* totals, int64_t* key_out, int64_t* off_out) {
  for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < S; d += (int64_t)gridDim.x * 256) {
    if (d == 0) off_out[totals[0]] = totals[1];
    if (cnt[d] <= 0) continue;
    int lo = 0, hi = ncs - 1;                                  // the last cs whose dense range starts at or before d
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (cbase[mid] <= d) lo = mid; else hi = mid - 1;
    }
    const int64_t row = rowid[d];
    key_out[row] = ((int64_t)lo << kPosBits) | (cmin[lo] + d - cbase[lo]);
    off_out[row] = soff[d];
  }
}

// a wave per read: event i of a read of n events starting at s lies at s + i ('+', cs even) or s + n - 1 - i ('-', cs odd)
__global__ __launch_bounds__(64 * kWaves) void rp_place_kernel(int64_t nreads, const int32_t* cs, const int64_t* start,
                                                               const int64_t* roff, int64_t pos_lo, int64_t pos_hi,
                                                               const int64_t* cmin, const int64_t* cbase, const int64_t* soff,
                                                               unsigned* cur, uint32_t* eidx) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); r < nreads; r += (int64_t)gridDim.x * kWaves) {
    const int64_t a = roff[r], n = roff[r + 1] - a, s = start[r];
    int64_t lo, hi;
    if (!clip_span(s, n, pos_lo, pos_hi, lo, hi)) continue;
    const int32_t c = cs[r];
    const bool minus = (c & 1) != 0;
    const int64_t dbase = cbase[c] - cmin[c];
    for (int64_t p = lo + lane; p <= hi; p += 64) {
      const int64_t e = a + (minus ? s + n - 1 - p : p - s);
      const int64_t d = dbase + p;
      const int64_t slot = soff[d] + (int64_t)atomicAdd(&cur[d], 1u);
      eidx[slot] = (uint32_t)e;
    }
  }
}

// a wave per row: rank the row's event indices (all distinct) by counting, in LDS; a lane holds up to kSmallRow / 64 of them
template <typename T>
__global__ __launch_bounds__(64 * kWaves) void rp_order_kernel(int64_t npos, const int64_t* off, const uint32_t* eidx, const T* val,
                                                               const uint8_t* base, T* sig_out, uint8_t* base_out,
                                                               unsigned long long* large, int64_t* lrow, int64_t* loff) {
  __shared__ uint32_t sh[kWaves][kSmallRow];
  constexpr int kHeld = kSmallRow / 64;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t* lds = sh[w];
  for (int64_t row = (int64_t)blockIdx.x * kWaves + w; row < npos; row += (int64_t)gridDim.x * kWaves) {
    const int64_t o = off[row];
    const int n = (int)min(off[row + 1] - o, (int64_t)kSmallRow + 1);
    if (n > kSmallRow) {
      if (lane == 0) {
        // list slot (high 32 bits) and sample offset (low 32 bits) from ONE atomic, so that loff[] is the prefix sum of the
        // row lengths in slot order — the layout the sort by (slot << 32 | event) gives.  The large rows' samples number at
        // most the events (< 2^32): the low half never carries into the slot.
        const unsigned long long old = atomicAdd(&large[0], (1ull << 32) | (unsigned long long)(off[row + 1] - o));
        const unsigned long long k = old >> 32;
        lrow[k] = row;
        loff[k] = (int64_t)(old & 0xFFFFFFFFull);
      }
      continue;
    }
    uint32_t v[kHeld];
    int rk[kHeld];
    const int held = (n + 63) >> 6;                 // slots in use: the same for every lane, so the loops below skip the rest
#pragma unroll
    for (int t = 0; t < kHeld; ++t) {
      const int j = lane + 64 * t;
      v[t] = j < n ? eidx[o + j] : 0xFFFFFFFFu;
      if (j < n) lds[j] = v[t];
      rk[t] = 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int k = 0; k < n; ++k) {
      const uint32_t x = lds[k];
#pragma unroll
      for (int t = 0; t < kHeld; ++t)
        if (t < held) rk[t] += x < v[t];
    }
#pragma unroll
    for (int t = 0; t < kHeld; ++t) {
      if (lane + 64 * t < n) {
        sig_out[o + rk[t]] = val[v[t]];
        if (rk[t] == n - 1) base_out[row] = base[v[t]];             // the last read's base (myDetect.py:122)
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");          // every lane has read the row before the next one lands
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

__global__ __launch_bounds__(64 * kWaves) void rp_large_keys_kernel(int64_t nlarge, const int64_t* lrow, const int64_t* loff,
                                                                    const int64_t* off, const uint32_t* eidx, uint64_t* keys,
                                                                    uint32_t* vals) {
  const int lane = threadIdx.x & 63;
  for (int64_t k = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); k < nlarge; k += (int64_t)gridDim.x * kWaves) {
    const int64_t o = off[lrow[k]], n = off[lrow[k] + 1] - o, dst = loff[k];
    for (int64_t j = lane; j < n; j += 64) {
      keys[dst + j] = ((uint64_t)k << 32) | eidx[o + j];
      vals[dst + j] = 0u;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void rp_large_place_kernel(int64_t total, const uint64_t* keys, const int64_t* lrow,
                                                             const int64_t* loff, const int64_t* off, const T* val,
                                                             const uint8_t* base, T* sig_out, uint8_t* base_out) {
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < total; j += (int64_t)gridDim.x * 256) {
    const uint64_t key = keys[j];
    const int64_t k = (int64_t)(key >> 32);
    const uint32_t e = (uint32_t)key;
    const int64_t row = lrow[k], o = off[row], i = j - loff[k];
    sig_out[o + i] = val[e];
    if (o + i == off[row + 1] - 1) base_out[row] = base[e];
  }
}

template <typename T>
int order_rows(int64_t npos, const int64_t* off, const uint32_t* eidx, const void* val, const uint8_t* base, void* sig_out,
               uint8_t* base_out, unsigned long long* large, int64_t* lrow, int64_t* loff, int dev, hipStream_t s) {
  hipLaunchKernelGGL(rp_order_kernel<T>, dim3(grid_for(npos, kWaves * 16)), dim3(64 * kWaves), 0, s, npos, off, eidx,
                     (const T*)val, base, (T*)sig_out, base_out, large, lrow, loff);
  NMOD_HIP(hipGetLastError());
  unsigned long long h = 0;
  NMOD_HIP(hipMemcpyAsync(&h, large, sizeof(h), hipMemcpyDeviceToHost, s));
  NMOD_HIP(hipStreamSynchronize(s));
  const int64_t nlarge = (int64_t)(h >> 32), total = (int64_t)(h & 0xFFFFFFFFull);
  if (nlarge == 0) return NMOD_OK;
  if (total >= INT32_MAX) return NMOD_ERR_INVALID_ARG;                        // the radix sort's index range (documented in the header)
  const size_t kb = (size_t)align256(total * 8), vb = (size_t)align256(total * 4);
  DevScratch ls;
  NMOD_HIP(ls.alloc(2 * kb + 2 * vb + rs_scratch_bytes(total), s, dev));
  char* p = static_cast<char*>(ls.p);
  uint64_t* ka = (uint64_t*)p; uint64_t* kb2 = (uint64_t*)(p + kb);
  uint32_t* va = (uint32_t*)(p + 2 * kb); uint32_t* vb2 = (uint32_t*)(p + 2 * kb + vb);
  hipLaunchKernelGGL(rp_large_keys_kernel, dim3(grid_for(nlarge, kWaves)), dim3(64 * kWaves), 0, s, nlarge, (const int64_t*)lrow,
                     (const int64_t*)loff, off, eidx, ka, va);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(rs_sort_pairs(ka, va, kb2, vb2, total, p + 2 * kb + 2 * vb, s));
  hipLaunchKernelGGL(rp_large_place_kernel<T>, dim3(grid_for(total, 256 * 8)), dim3(256), 0, s, total, (const uint64_t*)ka,
                     (const int64_t*)lrow, (const int64_t*)loff, off, (const T*)val, base, (T*)sig_out, base_out);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(ls.release(s));
  return NMOD_OK;
}

// the pivot works on device-resident tables only
int begin_call(const nmod_params* prm) {
  if (check_prm_common(prm) != NMOD_OK || prm->memspace != NMOD_MEM_DEVICE) return NMOD_ERR_INVALID_ARG;
  return select_device(prm, nullptr);
}

// ---------------------------------------------------------------------------------------------------- select / gather
// row i of group 1 is tested when both groups cover its key at least min_cov times (myDetect.py:301-314,421)
__global__ __launch_bounds__(256) void rp_match_kernel(int64_t npos0, const int64_t* key0, const int64_t* off0, int64_t npos1,
                                                       const int64_t* key1, const int64_t* off1, int64_t min_cov, int64_t* flag,
                                                       int64_t* match) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npos0; i += (int64_t)gridDim.x * 256) {
    int64_t f = 0, j = -1;
    if (off0[i + 1] - off0[i] >= min_cov) {
      const int64_t k = key0[i];
      int64_t lo = 0, hi = npos1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (key1[mid] < k) lo = mid + 1; else hi = mid;
      }
      if (lo < npos1 && key1[lo] == k && off1[lo + 1] - off1[lo] >= min_cov) { f = 1; j = lo; }
    }
    flag[i] = f; match[i] = j;
  }
}

__global__ __launch_bounds__(256) void rp_compact_kernel(int64_t npos0, const int64_t* flag, const int64_t* tidx, const int64_t* match,
                                                         const int64_t* off0, const int64_t* off1, int64_t* rows0, int64_t* rows1,
                                                         int64_t* len0, int64_t* len1) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npos0; i += (int64_t)gridDim.x * 256) {
    if (!flag[i]) continue;
    const int64_t t = tidx[i], j = match[i];
    rows0[t] = i; rows1[t] = j;
    len0[t] = off0[i + 1] - off0[i]; len1[t] = off1[j + 1] - off1[j];
  }
}

__device__ __forceinline__ double value_of(float v) { return (double)v; }
__device__ __forceinline__ double value_of(double v) { return v; }
__device__ __forceinline__ double value_of(int16_t k) { return (double)k / 1000.0; }

// detect.encode_signals per sample: bit 0 float32-exact, bit 1 on the 0.001 grid with |k| <= 32767.  A wave clears a bit with
// one atomic only while the bit is still set, and stops once nothing is left to decide: the flags word is read, not
// contended (almost every row of real data clears bit 0, and same-address atomics from every wave serialise).
// int16 milli-units are on the grid by definition and k / 1000.0 is float32-exact exactly when 125 divides k.
template <typename T>
__global__ __launch_bounds__(64 * kWaves) void rp_dtype_kernel(int64_t ntested, const int64_t* rows, const int64_t* off, const T* sig,
                                                               int* bits) {
  constexpr bool kMilli = std::is_same<T, int16_t>::value;
  constexpr int kAll = kMilli ? 1 : 3;
  const int lane = threadIdx.x & 63;
  for (int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t < ntested; t += (int64_t)gridDim.x * kWaves) {
    const int have = __hip_atomic_load(bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kAll;
    if (have == 0) return;                                               // (the same value for every lane of the wave)
    const int64_t o = off[rows[t]], n = off[rows[t] + 1] - o;
    bool f32 = true, grid = true;
    for (int64_t j = lane; j < n; j += 64) {
      if constexpr (kMilli) {
        f32 = f32 && (int)sig[o + j] % 125 == 0;
      } else {
        const double v = value_of(sig[o + j]);
        f32 = f32 && (double)(float)v == v;
        const double k = rint(v * 1000.0);
        grid = grid && fabs(k) <= 32767.0 && k / 1000.0 == v;
      }
    }
    const bool any_f32 = __any(!f32), any_grid = __any(!grid);
    if (lane == 0 && any_f32 && (have & 1)) atomicAnd(bits, ~1);
    if (lane == 0 && any_grid && (have & 2)) atomicAnd(bits, ~2);
  }
}

__device__ __forceinline__ void conv(float v, float& o) { o = v; }
__device__ __forceinline__ void conv(double v, double& o) { o = v; }
__device__ __forceinline__ void conv(int16_t v, int16_t& o) { o = v; }
__device__ __forceinline__ void conv(double v, float& o) { o = (float)v; }
__device__ __forceinline__ void conv(double v, int16_t& o) { o = (int16_t)rint(v * 1000.0); }
__device__ __forceinline__ void conv(int16_t v, float& o) { o = (float)((double)v / 1000.0); }
__device__ __forceinline__ void conv(int16_t v, double& o) { o = (double)v / 1000.0; }
__device__ __forceinline__ void conv(float v, double& o) { o = (double)v; }
__device__ __forceinline__ void conv(float v, int16_t& o) { o = (int16_t)rint((double)v * 1000.0); }

template <typename TI, typename TO>
__global__ __launch_bounds__(64 * kWaves) void rp_gather_kernel(int64_t ntested, const int64_t* rows, const int64_t* off, const TI* sig,
                                                                const int64_t* off_out, TO* sig_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t < ntested; t += (int64_t)gridDim.x * kWaves) {
    const int64_t o = off[rows[t]], n = off[rows[t] + 1] - o, d = off_out[t];
    for (int64_t j = lane; j < n; j += 64) conv(sig[o + j], sig_out[d + j]);
  }
}

// keys and bases of the tested rows; brk[t] = 1 where a new run starts (detect.run_ids: a change of cs or a gap in pos)
__global__ __launch_bounds__(256) void rp_meta_kernel(int64_t ntested, const int64_t* rows0, const int64_t* rows1, const int64_t* key1,
                                                      const uint8_t* base0, const uint8_t* base1, int64_t* key_out,
                                                      uint8_t* base0_out, uint8_t* base1_out, int64_t* brk) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < ntested; t += (int64_t)gridDim.x * 256) {
    const int64_t k = key1[rows1[t]];
    key_out[t] = k;
    base0_out[t] = base0[rows0[t]];
    base1_out[t] = base1[rows1[t]];
    brk[t] = (t == 0 || key1[rows1[t - 1]] + 1 != k || (k & (kPosLimit - 1)) == 0) ? 1 : 0;
  }
}
__global__ __launch_bounds__(256) void rp_run_kernel(int64_t ntested, const int64_t* incl, int32_t* run_out) {
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < ntested; t += (int64_t)gridDim.x * 256) run_out[t] = (int32_t)(incl[t] - 1);
}

template <typename TI>
int launch_gather(int32_t out_dtype, int64_t ntested, const int64_t* rows, const int64_t* off, const void* sig, const int64_t* off_out,
                  void* sig_out, hipStream_t s) {
  const dim3 g(grid_for(ntested, kWaves * 16)), b(64 * kWaves);
  if (out_dtype == NMOD_DTYPE_F32)
    hipLaunchKernelGGL((rp_gather_kernel<TI, float>), g, b, 0, s, ntested, rows, off, (const TI*)sig, off_out, (float*)sig_out);
  else if (out_dtype == NMOD_DTYPE_I16_MILLI)
    hipLaunchKernelGGL((rp_gather_kernel<TI, int16_t>), g, b, 0, s, ntested, rows, off, (const TI*)sig, off_out, (int16_t*)sig_out);
  else
    hipLaunchKernelGGL((rp_gather_kernel<TI, double>), g, b, 0, s, ntested, rows, off, (const TI*)sig, off_out, (double*)sig_out);
  NMOD_HIP(hipGetLastError());
  return NMOD_OK;
}

// off[0] == 0, non-decreasing, off[npos] == nsig: checked on the device before anything indexes through it
__global__ __launch_bounds__(256) void rp_check_off_kernel(int64_t npos, const int64_t* off, int64_t nsig, int* err) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i <= npos; i += (int64_t)gridDim.x * 256) {
    const int64_t v = off[i];
    if ((i == 0 && v != 0) || (i > 0 && v < off[i - 1]) || (i == npos && v != nsig) || v < 0 || v > nsig) atomicOr(err, 1);
  }
}

}  // namespace
}  // namespace nmod

using namespace nmod;

extern "C" int nmod_pivot_reads(const nmod_params* prm, int64_t nreads, int32_t ncs, const int32_t* cs, const int64_t* start,
                                const int64_t* roff, const void* val, const uint8_t* base, int64_t pos_lo, int64_t pos_hi,
                                int64_t cap_pos, int64_t* key_out, int64_t* off_out, void* sig_out, uint8_t* base_out,
                                int64_t* npos_out, int64_t* nsamples_out) {
  if (npos_out) *npos_out = 0;
  if (nsamples_out) *nsamples_out = 0;
  int rc = begin_call(prm);
  if (rc != NMOD_OK) return rc;
  if (nreads < 0 || ncs < 0 || cap_pos < 0 || !roff || !off_out || !npos_out || !nsamples_out || (pos_lo >= 0 && pos_hi >= 0 && pos_hi < pos_lo) ||
      pos_lo < -1 || pos_hi < -1 || (nreads > 0 && (!cs || !start || ncs == 0)))
    return NMOD_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)prm->stream;
  int64_t nevents = 0;
  NMOD_HIP(hipMemcpyAsync(&nevents, roff + nreads, 8, hipMemcpyDeviceToHost, s));
  NMOD_HIP(hipStreamSynchronize(s));
  if (nevents < 0 || nevents > (int64_t)UINT32_MAX) return NMOD_ERR_INVALID_ARG;   // event indices are 32-bit
  if (nevents > 0 && (!val || !base || !sig_out)) return NMOD_ERR_INVALID_ARG;
  // ---- per-cs covered range
  const int64_t nc = ncs > 0 ? ncs : 1;
  DevScratch head;
  const size_t head_bytes = 256 + (size_t)align256(nc * 8) * 2 + (size_t)align256((nc + 1) * 8);
  NMOD_HIP(head.alloc(head_bytes, s, prm->device));
  char* hp = static_cast<char*>(head.p);
  int* err = (int*)hp;
  int64_t* totals = (int64_t*)(hp + 64);                        // [npos, nsamples]
  unsigned long long* large = (unsigned long long*)(hp + 128);  // rows beyond kSmallRow << 32 | their samples
  int64_t* cmin = (int64_t*)(hp + 256);
  int64_t* cmax = (int64_t*)(hp + 256 + align256(nc * 8));
  int64_t* cbase = (int64_t*)(hp + 256 + 2 * align256(nc * 8));
  NMOD_HIP(hipMemsetAsync(hp, 0, 256, s));
  NMOD_HIP(hipMemsetAsync(cmin, 0xFF, nc * 8, s));
  NMOD_HIP(hipMemsetAsync(cmax, 0, nc * 8, s));
  if (nreads > 0) {
    hipLaunchKernelGGL(rp_check_kernel, dim3(grid_for(nreads, 256)), dim3(256), 0, s, nreads, ncs, cs, start, roff, nevents, pos_lo, pos_hi,
                       err, (unsigned long long*)cmin, (unsigned long long*)cmax);
    NMOD_HIP(hipGetLastError());
  }
  std::vector<int64_t> hmin(nc), hmax(nc), hbase(nc + 1);
  int herr = 0;
  NMOD_HIP(hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, s));
  NMOD_HIP(hipMemcpyAsync(hmin.data(), cmin, nc * 8, hipMemcpyDeviceToHost, s));
  NMOD_HIP(hipMemcpyAsync(hmax.data(), cmax, nc * 8, hipMemcpyDeviceToHost, s));
  NMOD_HIP(hipStreamSynchronize(s));
  if (herr) return NMOD_ERR_INVALID_ARG;
  int64_t S = 0;
  for (int64_t c = 0; c < nc; ++c) {
    hbase[c] = S;
    if (hmin[c] >= 0 && hmin[c] <= hmax[c]) S += hmax[c] - hmin[c] + 1;       // (an unset min reads back as -1)
    else hmin[c] = 0;
  }
  hbase[nc] = S;
  if (S == 0) {
    NMOD_HIP(hipMemsetAsync(off_out, 0, 8, s));
    NMOD_HIP(hipStreamSynchronize(s));
    return NMOD_OK;
  }
  NMOD_HIP(hipMemcpyAsync(cmin, hmin.data(), nc * 8, hipMemcpyHostToDevice, s));
  NMOD_HIP(hipMemcpyAsync(cbase, hbase.data(), (nc + 1) * 8, hipMemcpyHostToDevice, s));
  // ---- samples per dense position, rows, offsets.  Scratch: 28 B per dense position + 4 B per event (+ 16 B per large row)
  const int64_t nlcap = nevents / (kSmallRow + 1) + 1;
  const size_t b_cnt = align256((S + 1) * 8), b_row = align256(S * 8), b_cur = align256(S * 4), b_eidx = align256(nevents * 4),
               b_l = align256(nlcap * 8), b_bs = align256(scan_blocks(S + 1) * 8);
  DevScratch body;
  NMOD_HIP(body.alloc(b_cnt + 2 * b_row + b_cur + b_eidx + 2 * b_l + b_bs, s, prm->device));
  char* p = static_cast<char*>(body.p);
  int64_t* cnt = (int64_t*)p; p += b_cnt;
  int64_t* rowid = (int64_t*)p; p += b_row;
  int64_t* soff = (int64_t*)p; p += b_row;
  unsigned* cur = (unsigned*)p; p += b_cur;
  uint32_t* eidx = (uint32_t*)p; p += b_eidx;
  int64_t* lrow = (int64_t*)p; p += b_l;
  int64_t* loff = (int64_t*)p; p += b_l;
  int64_t* bsum = (int64_t*)p;
  NMOD_HIP(hipMemsetAsync(cnt, 0, (S + 1) * 8, s));
  NMOD_HIP(hipMemsetAsync(cur, 0, S * 4, s));
  hipLaunchKernelGGL(rp_diff_kernel, dim3(grid_for(nreads, 256)), dim3(256), 0, s, nreads, cs, start, roff, pos_lo, pos_hi,
                     (const int64_t*)cmin, (const int64_t*)cbase, (unsigned long long*)cnt);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP((scan_i64<kScanId, true>(cnt, cnt, S, bsum, nullptr, s)));
  NMOD_HIP((scan_i64<kScanNonzero, false>(cnt, rowid, S, bsum, totals, s)));
  NMOD_HIP((scan_i64<kScanId, false>(cnt, soff, S, bsum, totals + 1, s)));
  int64_t ht[2];
  NMOD_HIP(hipMemcpyAsync(ht, totals, 16, hipMemcpyDeviceToHost, s));
  NMOD_HIP(hipStreamSynchronize(s));
  if (ht[0] > cap_pos || (ht[0] > 0 && !key_out) || (ht[0] > 0 && !base_out)) return NMOD_ERR_INVALID_ARG;
  hipLaunchKernelGGL(rp_rows_kernel, dim3(grid_for(S, 256 * 8)), dim3(256), 0, s, S, ncs, (const int64_t*)cnt, (const int64_t*)rowid,
                     (const int64_t*)soff, (const int64_t*)cmin, (const int64_t*)cbase, (const int64_t*)totals, key_out, off_out);
  NMOD_HIP(hipGetLastError());
  hipLaunchKernelGGL(rp_place_kernel, dim3(grid_for(nreads, kWaves)), dim3(64 * kWaves), 0, s, nreads, cs, start, roff, pos_lo, pos_hi,
                     (const int64_t*)cmin, (const int64_t*)cbase, (const int64_t*)soff, cur, eidx);
  NMOD_HIP(hipGetLastError());
  const int64_t npos = ht[0];
  if (prm->dtype == NMOD_DTYPE_F32)
    rc = order_rows<float>(npos, off_out, eidx, val, base, sig_out, base_out, large, lrow, loff, prm->device, s);
  else if (prm->dtype == NMOD_DTYPE_I16_MILLI)
    rc = order_rows<int16_t>(npos, off_out, eidx, val, base, sig_out, base_out, large, lrow, loff, prm->device, s);
  else
    rc = order_rows<double>(npos, off_out, eidx, val, base, sig_out, base_out, large, lrow, loff, prm->device, s);
  if (rc != NMOD_OK) return rc;
  NMOD_HIP(body.release(s));
  NMOD_HIP(head.release(s));
  NMOD_HIP(hipStreamSynchronize(s));
  *npos_out = ht[0];
  *nsamples_out = ht[1];
  return NMOD_OK;
}

extern "C" int nmod_select_tested(const nmod_params* prm, int64_t min_coverage,
                                  int64_t npos0, const int64_t* key0, const int64_t* off0, const void* sig0, int64_t nsig0,
                                  int64_t npos1, const int64_t* key1, const int64_t* off1, const void* sig1, int64_t nsig1,
                                  int64_t cap, int64_t* rows0, int64_t* rows1, int64_t* off0_out, int64_t* off1_out,
                                  int64_t* ntested_out, int64_t* nsamples0_out, int64_t* nsamples1_out, int32_t* dtype_out) {
  if (ntested_out) *ntested_out = 0;
  if (nsamples0_out) *nsamples0_out = 0;
  if (nsamples1_out) *nsamples1_out = 0;
  int rc = begin_call(prm);
  if (rc != NMOD_OK) return rc;
  if (npos0 < 0 || npos1 < 0 || nsig0 < 0 || nsig1 < 0 || cap < 0 || !off0 || !off1 || !off0_out || !off1_out || !ntested_out ||
      !nsamples0_out || !nsamples1_out || !dtype_out || (npos0 > 0 && !key0) || (npos1 > 0 && !key1) || (nsig0 > 0 && !sig0) ||
      (nsig1 > 0 && !sig1))
    return NMOD_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)prm->stream;
  const int64_t m = npos0 > 0 ? npos0 : 1;
  const size_t b = align256(m * 8), b_bs = align256((scan_blocks(m) + 1) * 8);
  DevScratch scr;
  NMOD_HIP(scr.alloc(256 + 3 * b + b_bs, s, prm->device));
  char* p = static_cast<char*>(scr.p);
  int* err = (int*)p;
  int64_t* tot = (int64_t*)(p + 64);
  int* bits = (int*)(p + 128);
  int64_t* flag = (int64_t*)(p + 256);
  int64_t* match = (int64_t*)(p + 256 + b);
  int64_t* tidx = (int64_t*)(p + 256 + 2 * b);
  int64_t* bsum = (int64_t*)(p + 256 + 3 * b);
  NMOD_HIP(hipMemsetAsync(p, 0, 256, s));
  hipLaunchKernelGGL(rp_check_off_kernel, dim3(grid_for(npos0 + 1, 256)), dim3(256), 0, s, npos0, off0, nsig0, err);
  hipLaunchKernelGGL(rp_check_off_kernel, dim3(grid_for(npos1 + 1, 256)), dim3(256), 0, s, npos1, off1, nsig1, err);
  NMOD_HIP(hipGetLastError());
  int herr = 0;
  NMOD_HIP(hipMemcpyAsync(&herr, err, 4, hipMemcpyDeviceToHost, s));
  NMOD_HIP(hipStreamSynchronize(s));
  if (herr) return NMOD_ERR_INVALID_ARG;
  int64_t nt = 0;
  if (npos0 > 0 && npos1 > 0) {
    hipLaunchKernelGGL(rp_match_kernel, dim3(grid_for(npos0, 256)), dim3(256), 0, s, npos0, key0, off0, npos1, key1, off1, min_coverage,
                       flag, match);
    NMOD_HIP(hipGetLastError());
    NMOD_HIP((scan_i64<kScanId, false>(flag, tidx, npos0, bsum, tot, s)));
    NMOD_HIP(hipMemcpyAsync(&nt, tot, 8, hipMemcpyDeviceToHost, s));
    NMOD_HIP(hipStreamSynchronize(s));
  }
  if (nt > cap || (nt > 0 && (!rows0 || !rows1))) return NMOD_ERR_INVALID_ARG;
  int32_t out_dtype = prm->dtype;
  int64_t ns[2] = {0, 0};
  if (nt == 0) {
    NMOD_HIP(hipMemsetAsync(off0_out, 0, 8, s));
    NMOD_HIP(hipMemsetAsync(off1_out, 0, 8, s));
  } else {
    // the tested rows' lengths go to off*_out[0, nt) and are scanned there in place; the sums land at off*_out[nt]
    hipLaunchKernelGGL(rp_compact_kernel, dim3(grid_for(npos0, 256)), dim3(256), 0, s, npos0, (const int64_t*)flag, (const int64_t*)tidx,
                       (const int64_t*)match, off0, off1, rows0, rows1, off0_out, off1_out);
    NMOD_HIP(hipGetLastError());
    NMOD_HIP((scan_i64<kScanId, false>(off0_out, off0_out, nt, bsum, off0_out + nt, s)));
    NMOD_HIP((scan_i64<kScanId, false>(off1_out, off1_out, nt, bsum, off1_out + nt, s)));
    NMOD_HIP(hipMemcpyAsync(&ns[0], off0_out + nt, 8, hipMemcpyDeviceToHost, s));
    NMOD_HIP(hipMemcpyAsync(&ns[1], off1_out + nt, 8, hipMemcpyDeviceToHost, s));
    NMOD_HIP(hipStreamSynchronize(s));
    // detect.encode_pair over the tested samples: one dtype for both groups
    const bool passthrough = prm->dtype == NMOD_DTYPE_F32 || (prm->dtype == NMOD_DTYPE_F64 && ns[0] + ns[1] > kDeviceEncodeAbove);
    if (!passthrough) {
      const int three = 3;
      NMOD_HIP(hipMemcpyAsync(bits, &three, 4, hipMemcpyHostToDevice, s));
      const dim3 g(grid_for(nt, kWaves * 16)), bl(64 * kWaves);
      for (int grp = 0; grp < 2; ++grp) {
        const int64_t* rows = grp ? rows1 : rows0; const int64_t* off = grp ? off1 : off0; const void* sig = grp ? sig1 : sig0;
        if (prm->dtype == NMOD_DTYPE_I16_MILLI)
          hipLaunchKernelGGL(rp_dtype_kernel<int16_t>, g, bl, 0, s, nt, (const int64_t*)rows, off, (const int16_t*)sig, bits);
        else
          hipLaunchKernelGGL(rp_dtype_kernel<double>, g, bl, 0, s, nt, (const int64_t*)rows, off, (const double*)sig, bits);
      }
      NMOD_HIP(hipGetLastError());
      int hb = 0;
      NMOD_HIP(hipMemcpyAsync(&hb, bits, 4, hipMemcpyDeviceToHost, s));
      NMOD_HIP(hipStreamSynchronize(s));
      out_dtype = (hb & 1) ? NMOD_DTYPE_F32 : (hb & 2) ? NMOD_DTYPE_I16_MILLI : NMOD_DTYPE_F64;
      if (prm->dtype == NMOD_DTYPE_I16_MILLI && !(hb & 1)) out_dtype = NMOD_DTYPE_I16_MILLI;
    }
  }
  NMOD_HIP(scr.release(s));
  NMOD_HIP(hipStreamSynchronize(s));
  *ntested_out = nt; *nsamples0_out = ns[0]; *nsamples1_out = ns[1]; *dtype_out = out_dtype;
  return NMOD_OK;
}

extern "C" int nmod_gather_tested(const nmod_params* prm, int64_t ntested, const int64_t* rows0, const int64_t* rows1,
                                  const int64_t* off0, const void* sig0, const uint8_t* base0,
                                  const int64_t* off1, const void* sig1, const uint8_t* base1, const int64_t* key1,
                                  int32_t out_dtype, const int64_t* off0_out, const int64_t* off1_out, void* sig0_out, void* sig1_out,
                                  int32_t* run_out, int64_t* key_out, uint8_t* base0_out, uint8_t* base1_out) {
  int rc = begin_call(prm);
  if (rc != NMOD_OK) return rc;
  if (ntested < 0 || !elem_bytes(out_dtype) || (prm->dtype == NMOD_DTYPE_F32 && out_dtype != NMOD_DTYPE_F32)) return NMOD_ERR_INVALID_ARG;
  if (ntested == 0) return NMOD_OK;
  if (!rows0 || !rows1 || !off0 || !off1 || !sig0 || !sig1 || !base0 || !base1 || !key1 || !off0_out || !off1_out || !sig0_out ||
      !sig1_out || !run_out || !key_out || !base0_out || !base1_out)
    return NMOD_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)prm->stream;
  for (int grp = 0; grp < 2; ++grp) {
    const int64_t* rows = grp ? rows1 : rows0; const int64_t* off = grp ? off1 : off0; const void* sig = grp ? sig1 : sig0;
    const int64_t* oo = grp ? off1_out : off0_out; void* so = grp ? sig1_out : sig0_out;
    if (prm->dtype == NMOD_DTYPE_F32) rc = launch_gather<float>(out_dtype, ntested, rows, off, sig, oo, so, s);
    else if (prm->dtype == NMOD_DTYPE_I16_MILLI) rc = launch_gather<int16_t>(out_dtype, ntested, rows, off, sig, oo, so, s);
    else rc = launch_gather<double>(out_dtype, ntested, rows, off, sig, oo, so, s);
    if (rc != NMOD_OK) return rc;
  }
  DevScratch scr;
  scr.park = true;                                  // enqueued only: the slab is kept for the stream's next call (scratch_pool.hpp)
  const size_t b = align256(ntested * 8);
  NMOD_HIP(scr.alloc(b + align256((scan_blocks(ntested) + 1) * 8), s, prm->device));
  int64_t* brk = (int64_t*)scr.p;
  int64_t* bsum = (int64_t*)((char*)scr.p + b);
  hipLaunchKernelGGL(rp_meta_kernel, dim3(grid_for(ntested, 256)), dim3(256), 0, s, ntested, rows0, rows1, key1, base0, base1, key_out,
                     base0_out, base1_out, brk);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP((scan_i64<kScanId, true>(brk, brk, ntested, bsum, nullptr, s)));
  hipLaunchKernelGGL(rp_run_kernel, dim3(grid_for(ntested, 256)), dim3(256), 0, s, ntested, (const int64_t*)brk, run_out);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(scr.release(s));
  return NMOD_OK;
}
