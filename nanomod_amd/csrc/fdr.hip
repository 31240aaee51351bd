// nmod_fdr_adjust — Benjamini-Hochberg / Benjamini-Yekutieli q-values of whole p-value tracks on the device (K7).
// The reference has no multiple-testing step; the definition is scipy.stats.false_discovery_control's, applied to the valid
// elements (0 <= p <= 1) of a track, every other element getting q = NaN.  Per track, all on the caller's stream:
//   fdr_key_kernel          p -> (64-bit key, index): the bit image of p orders like p on [0, 1]; invalid elements get the all-ones
//                           key and sort last.  m = number of valid elements, counted per wave, one atomic per wave
//   rs_sort_pairs           the library's LSD radix sort (radix_sort.hpp), eight one-byte passes over (key, index)
//   fdr_cm_kernel           BY only: c_m = sum_{k<=m} 1/k from the device's m (compensated sum below 64, the asymptotic series above)
//   fdr_tile_min_kernel     a block per tile of 2 048 sorted keys: a_i = fl(p_(i) * fl(m / i)) [* c_m], the tile's minimum
//   fdr_tile_suffix_kernel  one block: tmin[t] <- min of the tiles after t (exclusive suffix minimum)
//   fdr_apply_kernel        the tile again: reverse inclusive min-scan of a_i seeded with the tile's carry, q[index] = min(1, .),
//                           NaN for the invalid tail; #{q <= alpha} and the largest rejected key: wave reductions, LDS, one atomic
//                           of each per block
//   fdr_summary_kernel      the track's nmod_fdr_summary from the device words
// Reduce-then-scan over separate launches: no workgroup waits for another.  a_i >= 0 and finite, so minima are taken on bit
// images with integer min; the all-ones word stands for "no element".  Equal p get equal q whatever order the sort left them
// in (the running minimum from the right sees the whole tie run), so stability is not relied on.  m, c_m and the summary never
// leave the device: with NMOD_MEM_DEVICE the call returns without synchronising.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "entry_device.hpp"
#include "radix_sort.hpp"

namespace nmod {

constexpr int kFdrThreads = 256;
constexpr int kFdrItems = 8;
constexpr int kFdrTile = kFdrThreads * kFdrItems;      // sorted elements per block of the step-up passes (tests/test_fdr_gpu.py names it)
constexpr uint64_t kFdrNone = ~0ull;                   // key of an invalid element; identity of the integer min
constexpr int kFdrDirectSum = 64;                      // c_m: compensated direct sum below, asymptotic series from here on

// per-track device words
struct FdrState { unsigned long long m, rejected, maxkey; double cm; };

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  auto step = [](uint64_t x, auto tag) {
    constexpr int C = decltype(tag)::value;
    const unsigned lo = (unsigned)dpp_i<C>(0, (int)(unsigned)x);
    const unsigned hi = (unsigned)dpp_i<C>(0, (int)(unsigned)(x >> 32));
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    return o > x ? o : x;
  };
  v = step(v, std::integral_constant<int, NMOD_QP(1, 0, 3, 2)>{});
  v = step(v, std::integral_constant<int, NMOD_QP(2, 3, 0, 1)>{});
  v = step(v, std::integral_constant<int, kDppRowHalfMirror>{});
  v = step(v, std::integral_constant<int, kDppRowMirror>{});
  uint64_t r = 0;
#pragma unroll
  for (int row = 0; row < 4; ++row) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, row * 16);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), row * 16);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    r = o > r ? o : r;
  }
  return r;
}

__global__ __launch_bounds__(256) void fdr_key_kernel(const double* p, int64_t n, uint64_t* keys, uint32_t* idx, FdrState* st) {
  unsigned long long cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    double v = p[i];
    const bool ok = v >= 0.0 && v <= 1.0;               // false for NaN
    if (v == 0.0) v = 0.0;                              // -0.0 -> +0.0
    keys[i] = ok ? (uint64_t)__double_as_longlong(v) : kFdrNone;
    idx[i] = (uint32_t)i;
    cnt += ok ? 1ull : 0ull;
  }
  cnt = wave_sum_u64(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&st->m, cnt);
}

// c_m = H_m.  Below kFdrDirectSum a Kahan sum, smallest terms first; from there ln m + gamma + 1/(2m) - 1/(12m^2) + 1/(120m^4) -
// 1/(252m^6), whose first omitted term 1/(240m^8) is below 1e-16 of H_m at m = 64.
__global__ void fdr_cm_kernel(FdrState* st) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long m = st->m;
  double c;
  if (m < (unsigned long long)kFdrDirectSum) {
    double s = 0.0, comp = 0.0;
    for (unsigned long long k = m; k >= 1; --k) {
      const double y = 1.0 / (double)k - comp;
      const double t = s + y;
      comp = (t - s) - y;
      s = t;
    }
    c = m ? s : 1.0;
  } else {
    const double x = (double)m, r = 1.0 / x, r2 = r * r;
    const double tail = r * (0.5 - r * (1.0 / 12.0 - r2 * (1.0 / 120.0 - r2 * (1.0 / 252.0))));
    c = log(x) + (0.57721566490153286061 + tail);
  }
  st->cm = c;
}

// a_i of the element of 0-based rank r (i = r + 1) as a bit image; kFdrNone past the valid elements
__device__ __forceinline__ uint64_t fdr_a_bits(uint64_t key, int64_t r, int64_t m, double dm, bool by, double cm) {
  if (r >= m) return kFdrNone;
  const double ratio = dm / (double)(r + 1);            // fl(m / i), then one product: scipy's ps *= m / i
  double a = __longlong_as_double((long long)key) * ratio;
  if (by) a = a * cm;
  return (uint64_t)__double_as_longlong(a);
}

__device__ __forceinline__ uint64_t fdr_min_u64(uint64_t a, uint64_t b) { return a < b ? a : b; }

__global__ __launch_bounds__(kFdrThreads) void fdr_tile_min_kernel(const uint64_t* keys, int64_t n, const FdrState* st, int by, uint64_t* tmin) {
  __shared__ uint64_t sh[kFdrThreads];
  const int64_t m = (int64_t)st->m;
  const double dm = (double)m, cm = st->cm;
  const int64_t base = (int64_t)blockIdx.x * kFdrTile;
  uint64_t v = kFdrNone;
#pragma unroll
  for (int e = 0; e < kFdrItems; ++e) {
    const int64_t r = base + e * kFdrThreads + threadIdx.x;            // any order: only the tile's minimum is wanted
    if (r < n) v = fdr_min_u64(v, fdr_a_bits(keys[r], r, m, dm, by != 0, cm));
  }
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int d = kFdrThreads / 2; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) sh[threadIdx.x] = fdr_min_u64(sh[threadIdx.x], sh[threadIdx.x + d]);
    __syncthreads();
  }
  if (threadIdx.x == 0) tmin[blockIdx.x] = sh[0];
}

// inclusive suffix minimum over the 256 threads of a block: thread t gets min over threads t..255 (sh: 256 words)
__device__ __forceinline__ uint64_t fdr_block_suffix_min(uint64_t v, uint64_t* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < kFdrThreads; d <<= 1) {
    const uint64_t o = threadIdx.x + d < (unsigned)kFdrThreads ? sh[threadIdx.x + d] : kFdrNone;
    __syncthreads();
    sh[threadIdx.x] = fdr_min_u64(sh[threadIdx.x], o);
    __syncthreads();
  }
  const uint64_t r = sh[threadIdx.x];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kFdrThreads) void fdr_tile_suffix_kernel(uint64_t* tmin, int64_t ntiles) {          // one block
  __shared__ uint64_t sh[kFdrThreads];
  uint64_t carry = kFdrNone;                                            // min of everything after the chunk in hand
  for (int64_t hi = ntiles; hi > 0; hi -= kFdrThreads) {                // chunks of 256 tiles, last first
    const int64_t i = hi - kFdrThreads + threadIdx.x;
    const uint64_t v = i >= 0 ? tmin[i] : kFdrNone;
    const uint64_t incl = fdr_block_suffix_min(v, sh);                  // min over i..hi-1
    sh[threadIdx.x] = incl;
    __syncthreads();
    const uint64_t after = threadIdx.x + 1 < (unsigned)kFdrThreads ? sh[threadIdx.x + 1] : kFdrNone;   // min over i+1..hi-1
    const uint64_t chunk_min = sh[0];
    __syncthreads();
    if (i >= 0) tmin[i] = fdr_min_u64(after, carry);
    carry = fdr_min_u64(carry, chunk_min);
  }
}

__global__ __launch_bounds__(kFdrThreads) void fdr_apply_kernel(const uint64_t* keys, const uint32_t* idx, int64_t n, FdrState* st, int by,
                                                                double alpha, const uint64_t* tmin, double* q) {
  __shared__ uint64_t sh[kFdrThreads];
  __shared__ unsigned long long wrej[kFdrThreads / 64];
  __shared__ uint64_t wmax[kFdrThreads / 64];
  const int64_t m = (int64_t)st->m;
  const double dm = (double)m, cm = st->cm;
  // a thread owns kFdrItems consecutive ranks: one block-wide scan of the threads' minima serves the whole tile
  const int64_t r0 = (int64_t)blockIdx.x * kFdrTile + (int64_t)threadIdx.x * kFdrItems;
  uint64_t key[kFdrItems], a[kFdrItems];
  uint64_t mine = kFdrNone;
#pragma unroll
  for (int e = 0; e < kFdrItems; ++e) {
    const int64_t r = r0 + e;
    key[e] = r < n ? keys[r] : kFdrNone;
    a[e] = r < n ? fdr_a_bits(key[e], r, m, dm, by != 0, cm) : kFdrNone;
    mine = fdr_min_u64(mine, a[e]);
  }
  const uint64_t incl = fdr_block_suffix_min(mine, sh);                 // threads t..255
  sh[threadIdx.x] = incl;
  __syncthreads();
  uint64_t run = threadIdx.x + 1 < (unsigned)kFdrThreads ? sh[threadIdx.x + 1] : kFdrNone;
  run = fdr_min_u64(run, tmin[blockIdx.x]);                             // everything after this thread's last rank
  unsigned long long rej = 0;
  uint64_t maxkey = 0;
#pragma unroll
  for (int e = kFdrItems - 1; e >= 0; --e) {
    const int64_t r = r0 + e;
    run = fdr_min_u64(run, a[e]);
    if (r < n) {
      double qv;
      if (r < m) {
        qv = fmin(1.0, __longlong_as_double((long long)run));
        if (qv <= alpha) { ++rej; maxkey = key[e] > maxkey ? key[e] : maxkey; }
      } else {
        qv = nan_f64();
      }
      q[idx[r]] = qv;
    }
  }
  rej = wave_sum_u64(rej);
  maxkey = wave_max_u64(maxkey);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { wrej[wave] = rej; wmax[wave] = maxkey; }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long tr = 0;
    uint64_t tm = 0;
#pragma unroll
    for (int w = 0; w < kFdrThreads / 64; ++w) { tr += wrej[w]; tm = wmax[w] > tm ? wmax[w] : tm; }
    if (tr) {
      atomicAdd(&st->rejected, tr);
      atomicMax(&st->maxkey, (unsigned long long)tm);
    }
  }
}

__global__ void fdr_summary_kernel(const FdrState* st, int64_t n, nmod_fdr_summary* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  out->tested = (int64_t)st->m;
  out->excluded = n - (int64_t)st->m;
  out->rejected = (int64_t)st->rejected;
  out->p_crit = st->rejected ? __longlong_as_double((long long)st->maxkey) : nan_f64();
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_fdr_adjust(const nmod_params* prm, int64_t n, int32_t ntracks, const double* const* p, int32_t method, double alpha,
                               double* const* q_out, nmod_fdr_summary* summary) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;       // (a p-value track is fp64)
  if (n < 0 || n > (int64_t)INT32_MAX - 1 || ntracks < 1 || ntracks > 8 || !p || !q_out) return NMOD_ERR_INVALID_ARG;
  if (method != NMOD_FDR_BH && method != NMOD_FDR_BY) return NMOD_ERR_INVALID_ARG;
  if (!(alpha > 0.0 && alpha <= 1.0)) return NMOD_ERR_INVALID_ARG;
  for (int t = 0; n > 0 && t < ntracks; ++t) if (!p[t] || !q_out[t]) return NMOD_ERR_INVALID_ARG;      // (an empty track has no address)
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (n == 0 && (host || !summary)) {
    for (int t = 0; summary && t < ntracks; ++t) { memset(&summary[t], 0, sizeof(summary[t])); summary[t].p_crit = NAN; }
    return NMOD_OK;
  }
  const int rc = select_device(prm, nullptr);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t cnt = (size_t)n;
  const int64_t ntiles = (n + kFdrTile - 1) / kFdrTile;

  // one slab: keys, keys_tmp, tile minima, per-track state, idx, idx_tmp, histogram; for the host entry one track (the tracks
  // go through it one after another) and the summaries
  Slab slab(host);
  const size_t o_keys = slab.take(cnt * 8), o_keys_tmp = slab.take(cnt * 8), o_tmin = slab.take((size_t)(ntiles + 1) * 8);
  const size_t o_state = slab.take(sizeof(FdrState) * 8);
  const size_t o_track = slab.take(host ? cnt * 8 : 0), o_idx = slab.take(cnt * 4), o_idx_tmp = slab.take(cnt * 4);
  const size_t o_hist = slab.take(n ? rs_scratch_bytes(n) : 0);
  nmod_fdr_summary* dsum = summary;
  slab.out(dsum, sizeof(nmod_fdr_summary) * (size_t)ntracks);
  NMOD_HIP(slab.commit(stream, prm->device));
  uint64_t* keys = slab.at<uint64_t>(o_keys); uint64_t* keys_tmp = slab.at<uint64_t>(o_keys_tmp); uint64_t* tmin = slab.at<uint64_t>(o_tmin);
  FdrState* state = slab.at<FdrState>(o_state);
  double* dtrack = slab.at<double>(o_track);
  uint32_t* idx = slab.at<uint32_t>(o_idx); uint32_t* idx_tmp = slab.at<uint32_t>(o_idx_tmp);
  void* hist = slab.at<char>(o_hist);

  NMOD_HIP(hipMemsetAsync(state, 0, sizeof(FdrState) * 8, stream));
  const unsigned kblocks = (unsigned)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  for (int t = 0; t < ntracks; ++t) {             // one after another through the same scratch
    FdrState* st = state + t;
    const double* src = p[t];
    double* dst = q_out[t];
    if (n > 0) {
      if (host) {
        NMOD_HIP(hipMemcpyAsync(dtrack, p[t], cnt * 8, hipMemcpyHostToDevice, stream));
        src = dtrack; dst = dtrack;
      }
      hipLaunchKernelGGL(fdr_key_kernel, dim3(kblocks), dim3(256), 0, stream, src, n, keys, idx, st);
      NMOD_HIP(rs_sort_pairs(keys, idx, keys_tmp, idx_tmp, n, hist, stream));
      if (method == NMOD_FDR_BY) hipLaunchKernelGGL(fdr_cm_kernel, dim3(1), dim3(64), 0, stream, st);
      hipLaunchKernelGGL(fdr_tile_min_kernel, dim3((unsigned)ntiles), dim3(kFdrThreads), 0, stream, (const uint64_t*)keys, n,
                         (const FdrState*)st, (int)method, tmin);
      hipLaunchKernelGGL(fdr_tile_suffix_kernel, dim3(1), dim3(kFdrThreads), 0, stream, tmin, ntiles);
      hipLaunchKernelGGL(fdr_apply_kernel, dim3((unsigned)ntiles), dim3(kFdrThreads), 0, stream, (const uint64_t*)keys, (const uint32_t*)idx, n,
                         st, (int)method, alpha, (const uint64_t*)tmin, dst);
      if (host) NMOD_HIP(hipMemcpyAsync(q_out[t], dtrack, cnt * 8, hipMemcpyDeviceToHost, stream));
    }
    if (dsum) hipLaunchKernelGGL(fdr_summary_kernel, dim3(1), dim3(64), 0, stream, (const FdrState*)st, n, dsum + t);
  }
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(slab.finish(stream));
  return NMOD_OK;
}
