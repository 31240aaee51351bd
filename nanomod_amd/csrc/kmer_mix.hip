// nmod_kmer_mix — learn the modified k-mer table from a mixed sample on the device (K17).  The reference project has
// no such step; the definition is the one in include/nanomod_hip.h (tests/kmix_ref.py restates it in numpy).  Per k-mer code the
// unmodified component is fixed at a control table's (mean0, sd0), the events of the code's positions are pooled into an integer
// histogram over the window lo .. lo + 4 095 of the 0.001 grid, and K8's EM runs on the histogram.  All on the caller's stream:
//   kmix_window_kernel    a thread per code: usable or not, and the window's first integer lo
//   kmix_classify_kernel  a thread per position: the status from its code and size, and the sort key (its code; a position that takes
//                         no part sorts behind every code)
//   rs_sort_pairs         grouping of the position indices by code (one to three one-byte passes)
//   kmix_items_kernel     one workgroup: where each code's positions start in the sorted order (a search per code), and an exclusive
//                         scan of ceil(count / kKmixChunk) over the codes: item i of code c is positions
//                         cstart[c] + (i - istart[c]) * kKmixChunk .. of the sorted order
//   kmix_hist_kernel<DT>  the hot path.  Persistent workgroups draw items by ticket (read_walk.hpp: draw_read's workgroup form).  Per
//                         item: a 4 096-word LDS histogram, a wave per row — int16 rows in aligned 8-byte pieces, a piece per lane,
//                         whatever 2-byte offset the row starts at — a sample inside the window is an LDS integer atomic add on its
//                         bin, a sample outside goes to a per-lane counter; then the non-zero bins go to the code's row of the global
//                         histogram with 32-bit integer atomics and the three counts are added once per item.
//   kmix_em_kernel        a workgroup of 256 threads per code: thread t holds bins t, t + 256, ... (16 counts and their x in
//                         registers) over all iterations; every sum is that fixed chain per thread, then block_sum_f64.  Everything a
//                         decision rests on is a block sum, the same bits in every thread: the control flow is uniform.
// Integer sums do not depend on their order and the EM reads the histogram only: a code's outputs are the same bits for any order of
// the positions, CSR or stride, host or device memory, whatever else is in the batch and any CU count.  No float atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "entry_device.hpp"
#include "radix_sort.hpp"

namespace nmod {

constexpr int kKmixThreads = 256;                 // both kernels: four waves
constexpr int kKmixWaves = kKmixThreads / 64;
constexpr int kKmixPer = NMOD_KMIX_BINS / kKmixThreads;   // bins a thread of the EM keeps
constexpr int kKmixChunk = 256;                   // positions per item (tests/test_kmer_mix_gpu.py names it); not a measured value
constexpr int kKmixBlocksPerCu = 8;               // 16 KiB of LDS and four waves each
constexpr int kKmixVec = 4;                       // int16 samples per lane and step: one aligned 8-byte load
constexpr int kKmixItemThreads = 1024;
constexpr int32_t kKmixNoWindow = INT32_MIN;      // lo of an unusable code

struct KmixArgs {
  const void* sig; const int64_t* off; int64_t stride; const int32_t* code;
  int64_t npos; int32_t ncodes;
  const double* mean0; const double* sd0;
  int model, max_iter; long long min_samples; double tol;
  int32_t* lo;                                    // per code: the window's first integer, kKmixNoWindow: unusable
  uint32_t* cstart; uint32_t* istart;             // ncodes + 1 each: the code's first place in the sorted order, its first item
  unsigned long long* cnt;                        // 3 x ncodes: n_used, n_outside, n_positions; then the ticket word
  unsigned* ticket;
  uint32_t* hist;                                 // ncodes x NMOD_KMIX_BINS: out.hist or scratch
  uint64_t* key; uint32_t* val;                   // the sort's pairs
  nmod_kmix_out out;
};

__host__ __device__ inline bool kmix_usable(double mean0, double sd0) {
  return fabs(mean0) <= 1000.0 && sd0 > 0.0 && sd0 <= 1.7976931348623157e308;      // (NaN compares false)
}

__global__ __launch_bounds__(256) void kmix_window_kernel(KmixArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.ncodes) return;
  const double m = a.mean0[c];
  a.lo[c] = kmix_usable(m, a.sd0[c]) ? (int32_t)llrint(1000.0 * m) - NMOD_KMIX_HALF : kKmixNoWindow;
}

__global__ __launch_bounds__(256) void kmix_classify_kernel(KmixArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.npos) return;
  const int64_t n = a.off ? a.off[p + 1] - a.off[p] : a.stride;
  int c = a.code[p];
  unsigned st = 0;
  if (c < 0 || c >= a.ncodes) st |= NMOD_STATUS_NO_CODE;
  if (n <= 0) st |= NMOD_STATUS_EMPTY;
  if (n > (int64_t)NMOD_MAX_DEEP) st |= NMOD_STATUS_TOO_LARGE;
  if (st || a.lo[c] == kKmixNoWindow) c = a.ncodes;             // (lo is read for a code inside [0, ncodes) only)
  if (a.out.pos_status) a.out.pos_status[p] = (uint8_t)st;
  a.key[p] = (uint64_t)c;
  a.val[p] = (uint32_t)p;
}

__device__ __forceinline__ uint32_t kmix_lower_bound(const uint64_t* keys, int64_t n, uint64_t k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] < k) lo = mid + 1; else hi = mid; }
  return (uint32_t)lo;
}

// one workgroup.  skey: the sorted keys.  Thread t takes the codes t * per .. t * per + per - 1
__global__ __launch_bounds__(kKmixItemThreads) void kmix_items_kernel(KmixArgs a, const uint64_t* skey) {
  __shared__ unsigned sh[kKmixItemThreads];
  const int t = threadIdx.x, nc = a.ncodes;
  const int per = (nc + kKmixItemThreads - 1) / kKmixItemThreads;
  const int c0 = t * per < nc ? t * per : nc, c1 = c0 + per < nc ? c0 + per : nc;
  unsigned items = 0;
  uint32_t begin = c0 < c1 ? kmix_lower_bound(skey, a.npos, (uint64_t)c0) : 0u;
  for (int c = c0; c < c1; ++c) {
    const uint32_t end = kmix_lower_bound(skey, a.npos, (uint64_t)c + 1);
    a.cstart[c] = begin;
    if (c == nc - 1) a.cstart[nc] = end;
    items += (end - begin + (kKmixChunk - 1)) / kKmixChunk;
    begin = end;
  }
  sh[t] = items;
  __syncthreads();
  for (int d = 1; d < kKmixItemThreads; d <<= 1) {              // inclusive scan over the threads
    const unsigned add = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  unsigned run = sh[t] - items;
  for (int c = c0; c < c1; ++c) {
    a.istart[c] = run;
    run += (a.cstart[c + 1] - a.cstart[c] + (kKmixChunk - 1)) / kKmixChunk;     // (cstart[c1]: the next thread's store, before the scan's barriers)
  }
  if (t == kKmixItemThreads - 1) a.istart[nc] = sh[t];
}

// the samples of one row into the workgroup's histogram, by one wave; n_in / n_out: the lane's counts of the row
template <int DT>
__device__ __forceinline__ void kmix_row(const void* sig, int64_t b, int64_t e, int lo, unsigned* h, int lane, unsigned& n_in, unsigned& n_out,
                                         bool& nonfinite) {
  if constexpr (DT == NMOD_DTYPE_I16_MILLI) {
    const int16_t* sg = static_cast<const int16_t*>(sig);
    // aligned pieces of kKmixVec samples: the first starts at or below b.  A piece that is loaded holds at least one sample of
    // [b, e) and is aligned, so it lies in a page the vector has (kmer_model.hip: km_i16_kernel)
    const int64_t mis = (int64_t)(((reinterpret_cast<uintptr_t>(sg) >> 1) + (uint64_t)b) & (uint64_t)(kKmixVec - 1));
    for (int64_t s = b - mis + (int64_t)lane * kKmixVec; s < e; s += 64 * kKmixVec) {
      const int2 raw = *reinterpret_cast<const int2*>(sg + s);
      const int w[2] = {raw.x, raw.y};
#pragma unroll
      for (int k = 0; k < kKmixVec; ++k) {
        const int64_t idx = s + k;
        if (idx >= b && idx < e) {
          const int x = (k & 1) ? (w[k >> 1] >> 16) : (int)(short)(w[k >> 1] & 0xFFFF);
          const unsigned bin = (unsigned)(x - lo);
          if (bin < (unsigned)NMOD_KMIX_BINS) { atomicAdd(&h[bin], 1u); ++n_in; } else { ++n_out; }
        }
      }
    }
  } else {
    for (int64_t i = b + lane; i < e; i += 64) {
      double x;
      if constexpr (DT == NMOD_DTYPE_F32) x = (double)static_cast<const float*>(sig)[i]; else x = static_cast<const double*>(sig)[i];
      const bool fin = fabs(x) <= 1.7976931348623157e308;
      nonfinite |= !fin;
      const double d = rint(1000.0 * x) - (double)lo;           // exact: both are integers far below 2^53 wherever the test can pass
      if (fin && d >= 0.0 && d < (double)NMOD_KMIX_BINS) { atomicAdd(&h[(int)d], 1u); ++n_in; } else { ++n_out; }
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kKmixThreads) void kmix_hist_kernel(KmixArgs a, const uint32_t* sval) {
  __shared__ unsigned h[NMOD_KMIX_BINS];
  __shared__ unsigned long long s_cnt[3];
  __shared__ unsigned s_item;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nc = a.ncodes;
  const unsigned total = a.istart[nc];
  unsigned item = blockIdx.x;                                    // the first item is the block's own, the others come by ticket
  while (item < total) {
#pragma unroll
    for (int j = 0; j < kKmixPer; ++j) h[threadIdx.x + kKmixThreads * j] = 0u;
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0ull;
    // the item's code: the last c with istart[c] <= item (a code without items shares its istart with the next one)
    int c = 0;
    for (int hi = nc; c + 1 < hi;) { const int mid = (c + hi) >> 1; if (a.istart[mid] <= item) c = mid; else hi = mid; }
    const uint32_t first = a.cstart[c] + (item - a.istart[c]) * (uint32_t)kKmixChunk;
    const uint32_t cend = a.cstart[c + 1], last = cend - first < (uint32_t)kKmixChunk ? cend : first + (uint32_t)kKmixChunk;
    const int lo = a.lo[c];
    __syncthreads();
    unsigned long long n_in = 0, n_out = 0;
    unsigned n_pos = 0;
    for (uint32_t r = first + wave; r < last; r += kKmixWaves) {
      const int64_t p = (int64_t)sval[r];
      int64_t b, n;
      csr_row(a.off, a.stride, p, b, n);
      unsigned ri = 0, ro = 0;
      bool nonfinite = false;
      kmix_row<DT>(a.sig, b, b + n, lo, h, lane, ri, ro, nonfinite);
      n_in += ri; n_out += ro;
      n_pos += __ballot(ri != 0u) != 0ull ? 1u : 0u;
      if constexpr (DT != NMOD_DTYPE_I16_MILLI) {
        if (__ballot(nonfinite) != 0ull && lane == 0 && a.out.pos_status) a.out.pos_status[p] = (uint8_t)NMOD_STATUS_NONFINITE;
      }
    }
    n_in = wave_sum_u64(n_in);
    n_out = wave_sum_u64(n_out);
    if (lane == 0) {
      if (n_in) atomicAdd(&s_cnt[0], n_in);
      if (n_out) atomicAdd(&s_cnt[1], n_out);
      if (n_pos) atomicAdd(&s_cnt[2], (unsigned long long)n_pos);
    }
    __syncthreads();
    uint32_t* row = a.hist + (size_t)c * NMOD_KMIX_BINS;
#pragma unroll
    for (int j = 0; j < kKmixPer; ++j) {
      const unsigned v = h[threadIdx.x + kKmixThreads * j];
      if (v) atomicAdd(&row[threadIdx.x + kKmixThreads * j], v);
    }
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&a.cnt[(size_t)threadIdx.x * nc + c], s_cnt[threadIdx.x]);
    __syncthreads();                                             // the item's words are read before the next item's are stored
    if (threadIdx.x == 0) s_item = gridDim.x + atomicAdd(a.ticket, 1u);
    __syncthreads();
    item = s_item;
  }
}

// softplus(x) = ln(1 + e^x) without overflow
__device__ __forceinline__ double kmix_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

__device__ __forceinline__ void kmix_write(const nmod_kmix_out& o, int c, double pi, double m, double sd, double llr, int iters, unsigned status) {
  if (o.pi) o.pi[c] = pi;
  if (o.mu_mod) o.mu_mod[c] = m;
  if (o.sd_mod) o.sd_mod[c] = sd;
  if (o.llr) o.llr[c] = llr;
  if (o.iters) o.iters[c] = iters;
  if (o.status) o.status[c] = (uint8_t)status;
}

template <int MODEL>
__global__ __launch_bounds__(kKmixThreads) void kmix_em_kernel(KmixArgs a) {
  constexpr bool FREE = MODEL == 1;
  __shared__ double sh[kKmixWaves];
  __shared__ unsigned long long sh_s1;
  const int c = blockIdx.x, nc = a.ncodes, t = threadIdx.x;
  const int lo = a.lo[c];
  const bool usable = lo != kKmixNoWindow;
  const unsigned long long n = a.cnt[c];
  const double nan = nan_f64();
  if (t == 0) {
    if (a.out.n_used) a.out.n_used[c] = (int64_t)n;
    if (a.out.n_outside) a.out.n_outside[c] = (int64_t)a.cnt[(size_t)nc + c];
    if (a.out.n_positions) a.out.n_positions[c] = (int64_t)a.cnt[2 * (size_t)nc + c];
  }
  const long long need = a.min_samples > 2 ? a.min_samples : 2;
  if (!usable || (long long)n < need) {                          // (n < 2^32)
    if (t == 0) kmix_write(a.out, c, nan, nan, nan, nan, 0, usable ? NMOD_KMIX_TOO_FEW : NMOD_KMIX_NO_MODEL);
    return;
  }
  const uint32_t* row = a.hist + (size_t)c * NMOD_KMIX_BINS;
  double hb[kKmixPer], x[kKmixPer], rr[kKmixPer];
  long long s1 = 0;
  if (t == 0) sh_s1 = 0ull;
#pragma unroll
  for (int j = 0; j < kKmixPer; ++j) {
    const int b = t + kKmixThreads * j;
    const unsigned cntb = row[b];
    hb[j] = (double)cntb;
    x[j] = (double)(lo + b) / 1000.0;
    s1 += (long long)cntb * (long long)(lo + b);
  }
  __syncthreads();
  const unsigned long long ws1 = wave_sum_u64((unsigned long long)s1);          // (two's complement: the signed sum)
  if ((t & 63) == 0) atomicAdd(&sh_s1, ws1);
  __syncthreads();
  const long long S1 = (long long)sh_s1;

  const double dn = (double)n, mu = a.mean0[c], s = a.sd0[c], s2 = s * s, vfloor = s2 / 16.0, hs = 1.0 / (2.0 * s2);
  const double ybar = ((double)S1 / dn) / 1000.0;
  double pi = 0.5, m = mu + 2.0 * (ybar - mu), v = s2;
  int iters = 0;
  bool active = true, degenerate = false, floored = false;
  double c0 = 0.0, hv = 0.0;
  auto set_at = [&] {
    c0 = log((1.0 - pi) / pi);
    if constexpr (FREE) c0 += 0.5 * log(v / s2);
    hv = 1.0 / (2.0 * v);
  };
  auto tb = [&](double xb) { const double dy = xb - m, dm = xb - mu; return c0 + dy * dy * hv - dm * dm * hs; };
  for (int k = 1; k <= a.max_iter && active; ++k) {
    set_at();
    double sr = 0.0, sy = 0.0;
#pragma unroll
    for (int j = 0; j < kKmixPer; ++j) {
      const double r = hb[j] != 0.0 ? hb[j] * (1.0 / (1.0 + exp(tb(x[j])))) : 0.0;     // h_b r_b
      sr += r;
      sy += r * x[j];
      rr[j] = r;
    }
    sr = block_sum_f64<kKmixWaves>(sr, sh);
    sy = block_sum_f64<kKmixWaves>(sy, sh);
    if (!(sr > 0.0)) { degenerate = true; break; }              // every responsibility underflowed
    const double pn = sr / dn, mn = sy / sr;
    double vn = v;
    bool fl = false;
    if constexpr (FREE) {                                       // the second pass, about the new mean
      double sq = 0.0;
#pragma unroll
      for (int j = 0; j < kKmixPer; ++j) { const double e = x[j] - mn; sq += rr[j] * (e * e); }
      vn = block_sum_f64<kKmixWaves>(sq, sh) / sr;
      fl = vn < vfloor;
      if (fl) vn = vfloor;
    }
    double delta = fmax(fabs(pn - pi), fabs(mn - m) / s);
    if constexpr (FREE) delta = fmax(delta, fabs(sqrt(vn) - sqrt(v)) / s);
    pi = pn; m = mn; v = vn; floored = fl; iters = k;
    if (a.tol > 0.0 && delta <= a.tol) active = false;
  }
  if (degenerate) {
    if (t == 0) kmix_write(a.out, c, nan, nan, nan, nan, 0, NMOD_KMIX_DEGENERATE);
    return;
  }
  // final evaluation: llr
  set_at();
  const double l1 = log(1.0 - pi);
  double ll = 0.0;
#pragma unroll
  for (int j = 0; j < kKmixPer; ++j) ll += hb[j] != 0.0 ? hb[j] * (l1 + kmix_softplus(-tb(x[j]))) : 0.0;
  ll = 2.0 * block_sum_f64<kKmixWaves>(ll, sh);
  if (t == 0) kmix_write(a.out, c, pi, m, sqrt(v), ll, iters, (active ? NMOD_KMIX_NOT_CONVERGED : 0) | (floored ? NMOD_KMIX_VAR_FLOORED : 0));
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_kmer_mix(const nmod_params* prm, int64_t npos, const void* sig, const int64_t* off, const int32_t* code,
                             int32_t ncodes, const double* mean0, const double* sd0, const nmod_kmix_opts* opts,
                             const nmod_kmix_out* out) {
  if (check_prm_common(prm) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > (int64_t)INT32_MAX - 1 || ncodes < 1 || ncodes > NMOD_MAX_KMER_CODES) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_kmix_out)) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_kmix_opts)) return NMOD_ERR_INVALID_ARG;
  if (!mean0 || !sd0) return NMOD_ERR_INVALID_ARG;
  if (opts->model != 0 && opts->model != 1) return NMOD_ERR_INVALID_ARG;
  if (opts->max_iter < 1 || opts->max_iter > 10000 || !(opts->tol >= 0.0) || isinf(opts->tol) || opts->min_samples < 0) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && (!sig || !code)) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && !off && prm->stride0 <= 0) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && npos > 0) {
    if (off && !csr_offsets_ok(off, npos)) return NMOD_ERR_INVALID_ARG;
    for (int64_t i = 0; i < npos; ++i) if (code[i] < -1 || code[i] >= ncodes) return NMOD_ERR_INVALID_ARG;
  }
  const size_t nc = (size_t)ncodes, np = (size_t)npos;
  if (npos == 0 && host) {                                        // nothing to pool: no device is needed
    for (size_t c = 0; c < nc; ++c) {
      if (out->n_positions) out->n_positions[c] = 0;
      if (out->n_used) out->n_used[c] = 0;
      if (out->n_outside) out->n_outside[c] = 0;
      if (out->pi) out->pi[c] = NAN;
      if (out->mu_mod) out->mu_mod[c] = NAN;
      if (out->sd_mod) out->sd_mod[c] = NAN;
      if (out->llr) out->llr[c] = NAN;
      if (out->iters) out->iters[c] = 0;
      if (out->status) out->status[c] = kmix_usable(mean0[c], sd0[c]) ? NMOD_KMIX_TOO_FEW : NMOD_KMIX_NO_MODEL;
    }
    if (out->hist) memset(out->hist, 0, nc * NMOD_KMIX_BINS * 4);
    return NMOD_OK;
  }
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t esz = elem_bytes(prm->dtype);
  const size_t tot = host ? (size_t)(off ? off[npos] : npos * prm->stride0) : 0;
  const size_t hist_bytes = nc * NMOD_KMIX_BINS * 4;

  KmixArgs a;
  memset(&a, 0, sizeof(a));
  a.sig = sig; a.off = off; a.stride = off ? 0 : prm->stride0; a.code = code;
  a.npos = npos; a.ncodes = ncodes;
  a.mean0 = mean0; a.sd0 = sd0;
  a.model = opts->model; a.max_iter = opts->max_iter; a.min_samples = opts->min_samples; a.tol = opts->tol;
  a.out = *out;

  // one slab: the windows, the starts, the counts with the ticket word, the histogram unless the caller gave one, the sort's
  // buffers; for the host entry the inputs (the samples with 16 spare bytes: kmix_hist_kernel reads whole aligned pieces) and outputs
  Slab slab(host);
  const size_t o_lo = slab.take(nc * 4), o_cs = slab.take((nc + 1) * 4), o_is = slab.take((nc + 1) * 4), o_cnt = slab.take(nc * 24 + 8);
  const size_t o_hist = slab.take(out->hist ? 0 : hist_bytes);
  const size_t o_key = slab.take(np * 16), o_val = slab.take(np * 8), o_rs = slab.take(rs_scratch_bytes(npos));
  slab.in(a.sig, tot * esz, 16); slab.in(a.off, (np + 1) * 8); slab.in(a.code, np * 4);
  slab.in(a.mean0, nc * 8); slab.in(a.sd0, nc * 8);
  slab.out(a.out.n_positions, nc * 8); slab.out(a.out.n_used, nc * 8); slab.out(a.out.n_outside, nc * 8);
  slab.out(a.out.pi, nc * 8); slab.out(a.out.mu_mod, nc * 8); slab.out(a.out.sd_mod, nc * 8); slab.out(a.out.llr, nc * 8);
  slab.out(a.out.iters, nc * 4); slab.out(a.out.status, nc); slab.out(a.out.hist, hist_bytes); slab.out(a.out.pos_status, np);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.lo = slab.at<int32_t>(o_lo); a.cstart = slab.at<uint32_t>(o_cs); a.istart = slab.at<uint32_t>(o_is);
  a.cnt = slab.at<unsigned long long>(o_cnt); a.ticket = reinterpret_cast<unsigned*>(a.cnt + 3 * nc);
  a.hist = a.out.hist ? a.out.hist : slab.at<uint32_t>(o_hist);
  a.key = slab.at<uint64_t>(o_key); a.val = slab.at<uint32_t>(o_val);
  uint64_t* key_tmp = a.key + np; uint32_t* val_tmp = a.val + np;

  NMOD_HIP(hipMemsetAsync(a.cnt, 0, nc * 24 + 8, stream));
  NMOD_HIP(hipMemsetAsync(a.hist, 0, hist_bytes, stream));
  const unsigned code_blocks = (unsigned)((nc + 255) / 256);
  hipLaunchKernelGGL(kmix_window_kernel, dim3(code_blocks), dim3(256), 0, stream, a);
  const int passes = ncodes < 256 ? 1 : (ncodes < 65536 ? 2 : 3);             // the largest key is ncodes
  if (npos > 0) {
    hipLaunchKernelGGL(kmix_classify_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, a);
    NMOD_HIP(rs_sort_pairs(a.key, a.val, key_tmp, val_tmp, npos, slab.at<char>(o_rs), stream, passes));
  }
  const bool in_tmp = (passes & 1) != 0;
  const uint64_t* skey = in_tmp ? key_tmp : a.key;
  const uint32_t* sval = in_tmp ? val_tmp : a.val;
  hipLaunchKernelGGL(kmix_items_kernel, dim3(1), dim3(kKmixItemThreads), 0, stream, a, skey);
  if (npos > 0) {
    // at most npos / kKmixChunk whole items and one ragged item per code that has positions
    const int64_t max_items = npos / kKmixChunk + (npos < (int64_t)ncodes ? npos : (int64_t)ncodes);
    const dim3 grid(persistent_grid(max_items, 1, (int64_t)num_cus * kKmixBlocksPerCu));
    for_dtype(prm->dtype, [&](auto dt) {
      hipLaunchKernelGGL(kmix_hist_kernel<decltype(dt)::value>, grid, dim3(kKmixThreads), 0, stream, a, sval);
    });
  }
  if (a.model == 1) hipLaunchKernelGGL(kmix_em_kernel<1>, dim3((unsigned)nc), dim3(kKmixThreads), 0, stream, a);
  else hipLaunchKernelGGL(kmix_em_kernel<0>, dim3((unsigned)nc), dim3(kKmixThreads), 0, stream, a);
  return launches_end(slab, stream);
}
