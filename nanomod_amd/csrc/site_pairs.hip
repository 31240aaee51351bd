// nmod_pair_index / nmod_site_pairs — same-read co-occurrence of modification calls at pairs of candidate sites: per pair the 2 x 2
// table of the reads with a call at both sites, log odds ratio, phi and the two-sided exact test, on the device (K16).
// The reference project has no such step; the definition is the one in include/nanomod_hip.h (tests/pairs_ref.py restates it).  The
// walk over the reads is read_walk.hpp's, shared with K11 .. K13; all on the caller's stream:
//   sp_index_kernel      a thread per site: the number of its partners, an upper bound of key + max_dist inside its cs
//   sp_scan_kernel       one workgroup: the exclusive scan of those counts in place (poff)
//   read_classify_kernel (read_walk.hpp) a thread per read: the read's class by its length
//   sp_read_kernel<1, .> a wave per read of up to NMOD_CALLS_WAVE_MAX events, four waves a workgroup
//   sp_read_kernel<4, .> a workgroup of four waves per longer read
//   sp_pair_kernel       a thread per pair: first / second, status, log_or, se, phi, and p_fisher while the support has up to
//                        NMOD_PAIRS_THREAD_MAX tables; the pairs beyond go to a list
//   sp_pair_wave_kernel  a wave per listed pair: p_fisher by product scans over the lanes
// A read finds the candidate sites it covers by two binary searches in the keys (site_search.hpp, with the scan kernel, the read's score at
// a site and the host checks: shared with K19, read_hmm.hip).  Their calls are gathered from the scores, one gather
// per site with the strand-aware event index, and staged one byte per site in a window of kSpWin sites of wave- or workgroup-private
// LDS.  The first window of a tile holds the tile's own sites: a thread keeps the calls of the sites it owns in registers and walks
// their partners from the stage; the partners beyond the tile follow window by window (the forward halo), so neither the sites a read
// covers nor max_dist are bounded by the stage.  Counters: integer atomics only, on the int32 counters in device memory (direct form)
// or on a table in LDS that a workgroup flushes at the end of its persistent loop, one global atomic per non-zero counter (table form,
// up to NMOD_PAIRS_LDS_MAX pairs): the counts depend on neither the form nor the order of the reads.  No float atomics anywhere.
//
// nmod_pair_rows_count / nmod_pair_rows_fill — the rows of K18 (nmod_pair_linkage, site_linkage.hip) on the same walk, sp_walk_reads,
// whose work per (read, site) and per (read, pair) is a parameter: per pair the reads whose scores at both sites are valid.
//   sp_rows_kernel<., false>  the walk with "the score is valid" as the staged byte: one integer atomic per (read, pair) on the pair's count
//   sp_scan_kernel            the counts' exclusive scan in place (prow_off)
//   lr_init_kernel            every slot of the fill names itself and sorts last
//   sp_rows_kernel<., true>   the walk again: a read takes the next free row of its pair (an atomic cursor) and writes its key
//                             pair << 32 | read, its slot and its two scores
//   rs_sort_pairs             (radix_sort.hpp) the keys ascending: within a pair the rows in the order of the reads
//   lr_gather_kernel          sa, sb and read in that order: the same bytes whatever order the atomics fell in
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "radix_sort.hpp"
#include "read_walk.hpp"
#include "site_search.hpp"

namespace nmod {

constexpr int kSpWin = 256;                       // sites of a window of the stage: one byte each
constexpr int kSpNone = 2;                        // the staged byte of a site without a call (0: CAN, 1: MOD)

// what the walk over the reads takes: the reads, the scores, the sites and their pair index, the two lists of the reads
struct SpWalk {
  int64_t nreads; const int32_t* cs; const int64_t* start; const int64_t* roff; const double* score;
  int64_t nsites; const int64_t* key; const int64_t* poff; int64_t npairs;
  ReadLists w;
};

struct SpArgs : SpWalk {
  double thr; int32_t min_reads;
  int32_t* counts;                                // the caller's, or the slab's when the caller asked for none
  nmod_pairs_out out;
  uint32_t* big; uint32_t* big_count;             // the pairs whose p_fisher takes a wave
};

// K18's rows (nmod_pair_rows_count / nmod_pair_rows_fill): per pair the reads whose scores at both sites are valid
struct SpRowArgs : SpWalk {
  unsigned long long* cnt;                        // count: reads per pair (prow_off before its scan)
  const int64_t* prow_off; int64_t nrows;         // fill: the rows of pair j are prow_off[j] .. prow_off[j + 1] - 1
  int32_t* cursor;                                // the rows of each pair taken so far
  uint64_t* keys; uint32_t* vals; double* ta; double* tb;   // per slot: pair << 32 | read, the slot, the two scores
};

// ---------------------------------------------------------------------------------------------------------------- the pair index

__global__ __launch_bounds__(256) void sp_index_kernel(const int64_t* key, int64_t nsites, int64_t max_dist, int64_t* cnt) {
  for (int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x; a < nsites; a += (int64_t)gridDim.x * 256) {
    const int64_t k = key[a], last = k | kSpPosMask;            // the last key of a's cs
    const int64_t lim = k + max_dist < last ? k + max_dist : last;
    cnt[a] = sp_bound<true>(key, a + 1, nsites, lim) - (a + 1);
  }
}

// ---------------------------------------------------------------------------------------------------------------- the read kernel

// The walk of a persistent grid over the reads of list WAVES == 1 ? 0 : 1 (a wave per read, the workgroup's waves independent; else the
// workgroup per read): site search, staged windows, forward halo.  What happens per (read, site) and per (read, pair) is the callers':
//   state_of(rd, s)            the byte staged for site s of the read, kSpNone: the read takes no part in a pair of s
//   per_pair(rd, idx, ca, cb, s, b)   pair idx = (s, b) with the staged bytes ca, cb of its two sites, neither kSpNone
template <int WAVES, class StateOf, class PerPair>
__device__ __forceinline__ void sp_walk_reads(const SpWalk& a, uint8_t* stage, unsigned& sh_item, StateOf state_of, PerPair per_pair) {
  constexpr int CLS = WAVES == 1 ? 0 : 1;
  constexpr int T = WAVES * 64;                                 // threads of a read
  constexpr int PER = kSpWin / T;                               // sites of a tile a thread owns
  const int lane = threadIdx.x & 63;
  const int t = WAVES == 1 ? lane : (int)threadIdx.x;
  const unsigned cnt = a.w.count[CLS];
  const int64_t nsites = a.nsites, npairs = a.npairs;
  auto sync = [] { if constexpr (WAVES == 1) wave_lds_sync(); else __syncthreads(); };

  for (;;) {
    const unsigned item = draw_read<WAVES>(a.w, sh_item);
    if (item >= cnt) break;
    const int64_t read = (int64_t)a.w.list[CLS][item];
    int64_t begin, n;
    csr_row(a.roff, 0, read, begin, n);
    const int64_t cs = a.cs[read], start = a.start[read];
    if (n <= 0 || cs < 0 || start < 0 || start > kSpPosMask) continue;
    const int64_t last_pos = start + n - 1 < kSpPosMask ? start + n - 1 : kSpPosMask;
    // the candidate sites the read covers: c_lo .. c_hi - 1 (the same search in every thread of the read)
    const int64_t c_lo = sp_bound<false>(a.key, 0, nsites, (cs << 40) | start);
    const int64_t c_hi = sp_bound<true>(a.key, c_lo, nsites, (cs << 40) | last_pos);
    if (c_hi - c_lo < 2) continue;
    const SpRead rd{read, start, n, (cs & 1) != 0, a.score + begin, a.key};

    for (int64_t a0 = c_lo; a0 < c_hi - 1; a0 += kSpWin) {      // a tile of own sites a0 .. a_end - 1
      const int64_t a_end = a0 + kSpWin < c_hi ? a0 + kSpWin : c_hi;
      // the partners of the tile end where those of its last site do: the partner ranges ascend with the site
      int64_t reach = a_end + (a.poff[a_end] - a.poff[a_end - 1]);
      reach = reach < c_hi ? reach : c_hi;
      int ca[PER]; int64_t pb[PER], ea[PER];
      for (int64_t w0 = a0; w0 < reach; w0 += kSpWin) {         // (reach >= a_end > a0: the first window is the tile itself)
        const int wn = (int)(reach - w0 < kSpWin ? reach - w0 : kSpWin);
        for (int e = t; e < wn; e += T) stage[e] = (uint8_t)state_of(rd, w0 + e);
        sync();
        if (w0 == a0) {
#pragma unroll
          for (int j = 0; j < PER; ++j) {
            const int64_t s = a0 + t + T * j;
            ca[j] = kSpNone; pb[j] = 0; ea[j] = 0;
            if (s < a_end) {
              ca[j] = stage[t + T * j];
              pb[j] = a.poff[s];
              const int64_t e = s + 1 + (a.poff[s + 1] - pb[j]);
              ea[j] = e < c_hi ? e : c_hi;
            }
          }
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          if (ca[j] == kSpNone) continue;
          const int64_t s = a0 + t + T * j;
          const int64_t b0 = s + 1 > w0 ? s + 1 : w0, b1 = ea[j] < w0 + wn ? ea[j] : w0 + wn;
          for (int64_t b = b0; b < b1; ++b) {
            const int cb = stage[b - w0];
            if (cb == kSpNone) continue;
            const int64_t idx = pb[j] + (b - s - 1);
            if (idx < 0 || idx >= npairs) continue;             // (a poff that is not the keys': outside the counters)
            per_pair(rd, idx, ca[j], cb, s, b);
          }
        }
        sync();                                                 // the window is read before the next one is staged
      }
    }
  }
}

// K16: the staged byte is the read's call at the site, a pair's counter takes one.
// TABLE: the counters of the call live in the workgroup's LDS until the end
template <int WAVES, bool TABLE>
__global__ __launch_bounds__(kRwThreads) void sp_read_kernel(SpArgs a) {
  extern __shared__ int lds_tab[];                              // 4 * npairs counters when TABLE, else nothing
  __shared__ uint8_t lds_stage[WAVES == 1 ? kRwWaves : 1][kSpWin];
  __shared__ unsigned sh_item;
  const int ncell = TABLE ? (int)(4 * a.npairs) : 0;
  if constexpr (TABLE) {
    for (int c = threadIdx.x; c < ncell; c += kRwThreads) lds_tab[c] = 0;
    __syncthreads();
  }
  const double thr = a.thr;
  int32_t* const counts = a.counts;
  sp_walk_reads<WAVES>(a, lds_stage[WAVES == 1 ? threadIdx.x >> 6 : 0], sh_item,
    [thr](const SpRead& rd, int64_t s) -> int {
      double l;
      if (!rd.score_at(s, l)) return kSpNone;
      return l >= thr ? 1 : (l <= -thr ? 0 : kSpNone);
    },
    [=](const SpRead&, int64_t idx, int ca, int cb, int64_t, int64_t) {
      const int64_t cell = 4 * idx + 2 * ca + cb;
      if constexpr (TABLE) atomicAdd(&lds_tab[cell], 1); else atomicAdd(&counts[cell], 1);
    });
  if constexpr (TABLE) {
    __syncthreads();
    for (int c = threadIdx.x; c < ncell; c += kRwThreads) {
      const int v = lds_tab[c];
      if (v) atomicAdd(&a.counts[c], v);
    }
  }
}

// K18's rows: the staged byte says whether the read's score at the site is valid.  FILL false: a pair's count takes one; true: the read
// takes the next free row of its pair, in the order the atomics fall (lr_gather_kernel puts the rows of a pair in order)
template <int WAVES, bool FILL>
__global__ __launch_bounds__(kRwThreads) void sp_rows_kernel(SpRowArgs a) {
  __shared__ uint8_t lds_stage[WAVES == 1 ? kRwWaves : 1][kSpWin];
  __shared__ unsigned sh_item;
  sp_walk_reads<WAVES>(a, lds_stage[WAVES == 1 ? threadIdx.x >> 6 : 0], sh_item,
    [](const SpRead& rd, int64_t s) -> int {
      double l;
      return rd.score_at(s, l) && fabs(l) <= kDblMax ? 1 : kSpNone;
    },
    [&a](const SpRead& rd, int64_t idx, int, int, int64_t s, int64_t b) {
      if constexpr (!FILL) {
        atomicAdd(&a.cnt[idx], 1ull);
      } else {
        const int64_t r0 = a.prow_off[idx], r1 = a.prow_off[idx + 1];
        const int64_t slot = r0 + atomicAdd(&a.cursor[idx], 1);
        if (slot < r0 || slot >= r1 || slot >= a.nrows) return;   // (offsets that are not this call's counts: outside the rows)
        double la = 0.0, lb = 0.0;
        rd.score_at(s, la);
        rd.score_at(b, lb);
        a.keys[slot] = ((uint64_t)idx << 32) | (uint64_t)(uint32_t)rd.read;
        a.vals[slot] = (uint32_t)slot;
        a.ta[slot] = la; a.tb[slot] = lb;
      }
    });
}

// before the fill: every slot names itself and sorts last, so that a slot no read took (offsets that are not this call's counts) is
// still a row of the gather
__global__ __launch_bounds__(256) void lr_init_kernel(uint64_t* keys, uint32_t* vals, int64_t nrows) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nrows; i += (int64_t)gridDim.x * 256) { keys[i] = ~0ull; vals[i] = (uint32_t)i; }
}

// after the sort of the keys: row i is the slot vals[i]
__global__ __launch_bounds__(256) void lr_gather_kernel(const uint64_t* keys, const uint32_t* vals, const double* ta, const double* tb, int64_t nrows,
                                                        double* sa, double* sb, int32_t* read) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nrows; i += (int64_t)gridDim.x * 256) {
    const uint32_t v = vals[i];
    const bool ok = v < (uint64_t)nrows && keys[i] != ~0ull;
    if (sa) sa[i] = ok ? ta[v] : nan_f64();
    if (sb) sb[i] = ok ? tb[v] : nan_f64();
    if (read) read[i] = (int32_t)(uint32_t)keys[i];
  }
}

// ---------------------------------------------------------------------------------------------------------------- the pair kernels

struct SpTable {
  int64_t n11, n10, n01, n00, N, r1, c1, lo, hi, mode;
  __device__ __forceinline__ void load(const int32_t* counts, int64_t j) {
    const int4 c = *reinterpret_cast<const int4*>(counts + 4 * j);
    n00 = c.x; n01 = c.y; n10 = c.z; n11 = c.w;
    N = n11 + n10 + n01 + n00; r1 = n11 + n10; c1 = n11 + n01;
    lo = r1 + c1 - N > 0 ? r1 + c1 - N : 0;
    hi = r1 < c1 ? r1 : c1;
    mode = ((r1 + 1) * (c1 + 1)) / (N + 2);
    mode = mode < lo ? lo : (mode > hi ? hi : mode);
  }
  // w(x + 1) / w(x) and w(x - 1) / w(x)
  __device__ __forceinline__ double up(int64_t x) const { return (double)((c1 - x) * (r1 - x)) / (double)((x + 1) * (N - c1 - r1 + x + 1)); }
  __device__ __forceinline__ double down(int64_t x) const { return (double)(x * (N - c1 - r1 + x)) / (double)((c1 - x + 1) * (r1 - x + 1)); }
};

__device__ __forceinline__ double sp_finish_p(double T, double S) {
  double p = T / S;
  p = p < 1.0 ? p : 1.0;
  return p > kDblMin ? p : kDblMin;
}

// one thread, the support of up to NMOD_PAIRS_THREAD_MAX tables
__device__ double sp_fisher_thread(const SpTable& q) {
  double wo = 1.0;                                              // w(n11): the same chain as below
  if (q.n11 > q.mode) { for (int64_t x = q.mode; x < q.n11; ++x) wo = wo * q.up(x); }
  else { for (int64_t x = q.mode; x > q.n11; --x) wo = wo * q.down(x); }
  const double cut = wo * (1.0 + 1e-7);
  double U = 0.0, TU = 0.0, D = 0.0, TD = 0.0, w = 1.0;
  for (int64_t x = q.mode; x < q.hi; ++x) { w = w * q.up(x); U += w; TU += w <= cut ? w : 0.0; }
  w = 1.0;
  for (int64_t x = q.mode; x > q.lo; --x) { w = w * q.down(x); D += w; TD += w <= cut ? w : 0.0; }
  const double S = (1.0 + U) + D, T = ((1.0 <= cut ? 1.0 : 0.0) + TU) + TD;
  return sp_finish_p(T, S);
}

// the inclusive product scan over the lanes: steps 1 .. 32, v[l] = v[l] * v[l - d] for l >= d
__device__ __forceinline__ double sp_wave_prod_scan(double v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(v, d);
    v = lane >= d ? v * o : v;
  }
  return v;
}

// One side of the mode by the whole wave: f(w) per weight, in tile order.  UP: elements mode + 1 + 64 t + lane, else mode - 1 - 64 t - lane
template <bool UP, class F>
__device__ __forceinline__ void sp_wave_side(const SpTable& q, int lane, F f) {
  const int64_t len = UP ? q.hi - q.mode : q.mode - q.lo;       // elements of the side
  double carry = 1.0;
  for (int64_t t0 = 0; t0 < len; t0 += 64) {
    const int64_t k = t0 + lane;                                // the element's distance from the mode, less one
    const int64_t x = UP ? q.mode + k : q.mode - k;             // the table the step starts from
    const double r = k < len ? (UP ? q.up(x) : q.down(x)) : 0.0;
    const double w = carry * sp_wave_prod_scan(r, lane);
    f(k, w);
    carry = __shfl(w, 63);
  }
}

__device__ double sp_fisher_wave(const SpTable& q, int lane) {
  // w(n11): the weight of its element of its side
  double wo = 1.0;
  if (q.n11 != q.mode) {
    const int64_t ko = (q.n11 > q.mode ? q.n11 - q.mode : q.mode - q.n11) - 1;
    double mine = 0.0;
    auto pick = [&](int64_t k, double w) { if (k == ko) mine = w; };
    if (q.n11 > q.mode) sp_wave_side<true>(q, lane, pick); else sp_wave_side<false>(q, lane, pick);
    wo = __shfl(mine, (int)(ko & 63));
  }
  const double cut = wo * (1.0 + 1e-7);
  double s = 0.0, tl = 0.0;
  auto add = [&](int64_t, double w) { s += w; tl += w <= cut ? w : 0.0; };
  sp_wave_side<true>(q, lane, add);
  sp_wave_side<false>(q, lane, add);
  const double S = 1.0 + wave_sum_f64(s), T = (1.0 <= cut ? 1.0 : 0.0) + wave_sum_f64(tl);
  return sp_finish_p(T, S);
}

__global__ __launch_bounds__(256) void sp_pair_kernel(SpArgs a) {
  const int lane = threadIdx.x & 63;
  const nmod_pairs_out& o = a.out;
  const double nan = nan_f64();
  for (int64_t j0 = (int64_t)blockIdx.x * 256; j0 < a.npairs; j0 += (int64_t)gridDim.x * 256) {
    const int64_t j = j0 + threadIdx.x;
    int cls = -1;
    if (j < a.npairs) {
      SpTable q;
      q.load(a.counts, j);
      if (o.first || o.second) {
        const int64_t s = sp_bound<true>(a.poff, 0, a.nsites + 1, j) - 1;   // the last site whose pairs start at or before j
        if (o.first) o.first[j] = (int32_t)s;
        if (o.second) o.second[j] = (int32_t)(s + 1 + (j - a.poff[s]));
      }
      const int64_t r0 = q.N - q.r1, c0 = q.N - q.c1;
      const bool few = q.N < a.min_reads, degenerate = q.r1 == 0 || r0 == 0 || q.c1 == 0 || c0 == 0;
      if (o.status) o.status[j] = (uint8_t)((few ? NMOD_PAIRS_TOO_FEW : 0) | (degenerate ? NMOD_PAIRS_DEGENERATE : 0));
      if (few) {
        if (o.log_or) o.log_or[j] = nan;
        if (o.se) o.se[j] = nan;
        if (o.phi) o.phi[j] = nan;
        if (o.p_fisher) o.p_fisher[j] = nan;
      } else {
        const double h11 = (double)q.n11 + 0.5, h10 = (double)q.n10 + 0.5, h01 = (double)q.n01 + 0.5, h00 = (double)q.n00 + 0.5;
        if (o.log_or) o.log_or[j] = log((h11 * h00) / (h10 * h01));
        if (o.se) o.se[j] = sqrt(((1.0 / h11 + 1.0 / h10) + 1.0 / h01) + 1.0 / h00);
        if (o.phi) o.phi[j] = degenerate ? nan : (double)(q.n11 * q.n00 - q.n10 * q.n01) / sqrt((double)(q.r1 * r0) * (double)(q.c1 * c0));
        if (o.p_fisher) {
          if (q.hi - q.lo + 1 <= NMOD_PAIRS_THREAD_MAX) o.p_fisher[j] = sp_fisher_thread(q); else cls = 0;
        }
      }
    }
    uint32_t* const lists[1] = {a.big};
    compact_to_lists<1>(cls, lane, lists, a.big_count, j);
  }
}

__global__ __launch_bounds__(256) void sp_pair_wave_kernel(SpArgs a) {
  const int lane = threadIdx.x & 63;
  const unsigned cnt = *a.big_count;
  for (unsigned i = blockIdx.x * 4 + (threadIdx.x >> 6); i < cnt; i += gridDim.x * 4) {
    const int64_t j = a.big[i];
    SpTable q;
    q.load(a.counts, j);
    const double p = sp_fisher_wave(q, lane);
    if (lane == 0) a.out.p_fisher[j] = p;
  }
}

static void sp_walk_args(SpWalk& a, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff, const double* score,
                         int64_t nsites, const int64_t* key, const int64_t* poff, int64_t npairs) {
  a.nreads = nreads; a.cs = cs; a.start = start; a.roff = roff; a.score = score;
  a.nsites = nsites; a.key = key; a.poff = poff; a.npairs = npairs;
}

// the inputs of a host call that the walk reads, staged
static void sp_walk_stage(Slab& slab, SpWalk& a, size_t tot) {
  const size_t nr = (size_t)a.nreads, ns = (size_t)a.nsites;
  slab.in(a.cs, nr * 4); slab.in(a.start, nr * 8); slab.in(a.roff, (nr + 1) * 8); slab.in(a.score, tot * 8);
  slab.in(a.key, ns * 8); slab.in(a.poff, (ns + 1) * 8);
}

// the two forms of the rows kernel under eight workgroups a CU
template <bool FILL>
static void sp_launch_rows(const SpRowArgs& a, int num_cus, hipStream_t stream) {
  const int64_t cap = (int64_t)num_cus * 8;
  hipLaunchKernelGGL((sp_rows_kernel<1, FILL>), dim3(persistent_grid(a.nreads, kRwWaves, cap)), dim3(kRwThreads), 0, stream, a);
  hipLaunchKernelGGL((sp_rows_kernel<kRwWaves, FILL>), dim3(persistent_grid(a.nreads, 1, cap)), dim3(kRwThreads), 0, stream, a);
}

template <int WAVES, bool TABLE>
static void sp_launch_read(const SpArgs& a, int64_t cap, hipStream_t stream) {
  const size_t lds = TABLE ? (size_t)a.npairs * 16 : 0;
  hipLaunchKernelGGL((sp_read_kernel<WAVES, TABLE>), dim3(persistent_grid(a.nreads, WAVES == 1 ? kRwWaves : 1, cap)), dim3(kRwThreads), lds,
                     stream, a);
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_pair_index(const nmod_params* prm, int64_t nsites, const int64_t* key, int64_t max_dist, int64_t* poff_out,
                               int64_t* npairs_out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (nsites < 0 || nsites > (int64_t)INT32_MAX - 1 || max_dist < 1 || max_dist > NMOD_PAIRS_MAX_DIST) return NMOD_ERR_INVALID_ARG;
  if (!poff_out || !npairs_out || (nsites > 0 && !key)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && !sp_keys_ascend(key, nsites)) return NMOD_ERR_INVALID_ARG;
  if (host && nsites == 0) { poff_out[0] = 0; *npairs_out = 0; return NMOD_OK; }
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t ns = (size_t)nsites;
  int64_t* poff = poff_out;
  int64_t total = 0;

  Slab slab(host);
  slab.in(key, ns * 8); slab.out(poff, (ns + 1) * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  if (nsites > 0)
    hipLaunchKernelGGL(sp_index_kernel, dim3(persistent_grid(nsites, 256, (int64_t)num_cus * 16)), dim3(256), 0, stream, key, nsites, max_dist, poff);
  hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(256), 0, stream, poff, nsites);
  NMOD_HIP(hipMemcpyAsync(&total, poff + nsites, 8, hipMemcpyDeviceToHost, stream));
  NMOD_HIP(hipStreamSynchronize(stream));
  const int rc_end = launches_end(slab, stream);
  if (rc_end != NMOD_OK) return rc_end;
  if (total > (int64_t)INT32_MAX) return NMOD_ERR_INVALID_ARG;
  *npairs_out = total;
  return NMOD_OK;
}

extern "C" int nmod_site_pairs(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                               const double* score, int64_t nsites, const int64_t* key, const int64_t* poff, int64_t npairs,
                               const nmod_pairs_opts* opts, const nmod_pairs_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_pairs_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_pairs_out)) return NMOD_ERR_INVALID_ARG;
  if (!(opts->thr > 0.0) || !(opts->thr <= kDblMax) || opts->min_reads < 1 || (opts->flags & ~NMOD_PAIRS_FORCE_DIRECT)) return NMOD_ERR_INVALID_ARG;
  if (!sp_walk_args_ok(prm, nreads, cs, start, roff, score, nsites, key, poff, npairs)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (npairs == 0) return NMOD_OK;
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t nr = (size_t)nreads, np = (size_t)npairs;
  const size_t tot = host && nreads > 0 ? (size_t)roff[nreads] : 0;

  SpArgs a;
  memset(&a, 0, sizeof(a));
  sp_walk_args(a, nreads, cs, start, roff, score, nsites, key, poff, npairs);
  a.thr = opts->thr; a.min_reads = opts->min_reads;
  a.out = *out;

  // one slab: the read lists, the list of the pairs a wave computes, counters where the caller asked for none; for the host entry the
  // inputs and outputs as well
  Slab slab(host);
  const ReadListSpace lists(slab, nr);
  const size_t o_big = slab.take(np * 4), o_bigc = slab.take(4);
  const size_t o_counts = a.out.counts ? 0 : slab.take(np * 16);
  sp_walk_stage(slab, a, tot);
  slab.out(a.out.counts, np * 16); slab.out(a.out.first, np * 4); slab.out(a.out.second, np * 4);
  slab.out(a.out.log_or, np * 8); slab.out(a.out.se, np * 8); slab.out(a.out.phi, np * 8); slab.out(a.out.p_fisher, np * 8);
  slab.out(a.out.status, np);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.big = slab.at<uint32_t>(o_big); a.big_count = slab.at<uint32_t>(o_bigc);
  a.counts = a.out.counts ? a.out.counts : slab.at<int32_t>(o_counts);

  NMOD_HIP(hipMemsetAsync(a.counts, 0, np * 16, stream));
  NMOD_HIP(hipMemsetAsync(a.big_count, 0, 4, stream));
  if (nreads > 0) {
    NMOD_HIP(lists.fill(slab, a.roff, nreads, num_cus, stream, a.w));
    // at most eight workgroups a CU (the wave form's 94 VGPRs keep five resident; one that starts late finds the tickets drawn and
    // leaves), four for a call of few enough pairs to have an LDS table (4 x 33 KiB of the CU's 160) — in either form, so that the
    // two forms are compared on one grid
    const int64_t cap = (int64_t)num_cus * (npairs <= NMOD_PAIRS_LDS_MAX ? 4 : 8);
    if (npairs <= NMOD_PAIRS_LDS_MAX && !(opts->flags & NMOD_PAIRS_FORCE_DIRECT)) {
      sp_launch_read<1, true>(a, cap, stream);
      sp_launch_read<kRwWaves, true>(a, cap, stream);
    } else {
      sp_launch_read<1, false>(a, cap, stream);
      sp_launch_read<kRwWaves, false>(a, cap, stream);
    }
  }
  const bool stats = a.out.first || a.out.second || a.out.log_or || a.out.se || a.out.phi || a.out.p_fisher || a.out.status;
  if (stats) {
    hipLaunchKernelGGL(sp_pair_kernel, dim3(persistent_grid(npairs, 256, (int64_t)num_cus * 16)), dim3(256), 0, stream, a);
    if (a.out.p_fisher)
      hipLaunchKernelGGL(sp_pair_wave_kernel, dim3(persistent_grid(npairs, 4, (int64_t)num_cus * 8)), dim3(256), 0, stream, a);
  }
  return launches_end(slab, stream);
}

extern "C" int nmod_pair_rows_count(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                    const double* score, int64_t nsites, const int64_t* key, const int64_t* poff, int64_t npairs,
                                    int64_t* prow_off_out, int64_t* nrows_out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!prow_off_out || !nrows_out) return NMOD_ERR_INVALID_ARG;
  if (!sp_walk_args_ok(prm, nreads, cs, start, roff, score, nsites, key, poff, npairs)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && npairs == 0) { prow_off_out[0] = 0; *nrows_out = 0; return NMOD_OK; }
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t nr = (size_t)nreads, np = (size_t)npairs;
  const size_t tot = host && nreads > 0 ? (size_t)roff[nreads] : 0;
  int64_t* prow_off = prow_off_out;
  int64_t total = 0;

  SpRowArgs a;
  memset(&a, 0, sizeof(a));
  sp_walk_args(a, nreads, cs, start, roff, score, nsites, key, poff, npairs);

  Slab slab(host);
  const ReadListSpace lists(slab, nr);
  sp_walk_stage(slab, a, tot);
  slab.out(prow_off, (np + 1) * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.cnt = reinterpret_cast<unsigned long long*>(prow_off);
  NMOD_HIP(hipMemsetAsync(prow_off, 0, (np + 1) * 8, stream));
  if (nreads > 0 && npairs > 0) {
    NMOD_HIP(lists.fill(slab, a.roff, nreads, num_cus, stream, a.w));
    sp_launch_rows<false>(a, num_cus, stream);
  }
  hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(256), 0, stream, prow_off, npairs);
  NMOD_HIP(hipMemcpyAsync(&total, prow_off + npairs, 8, hipMemcpyDeviceToHost, stream));
  NMOD_HIP(hipStreamSynchronize(stream));
  const int rc_end = launches_end(slab, stream);
  if (rc_end != NMOD_OK) return rc_end;
  if (total > (int64_t)INT32_MAX) return NMOD_ERR_INVALID_ARG;
  *nrows_out = total;
  return NMOD_OK;
}

extern "C" int nmod_pair_rows_fill(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                   const double* score, int64_t nsites, const int64_t* key, const int64_t* poff, int64_t npairs,
                                   const int64_t* prow_off, int64_t nrows, double* sa, double* sb, int32_t* read) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (nrows < 0 || nrows > (int64_t)INT32_MAX || !prow_off) return NMOD_ERR_INVALID_ARG;
  if (!sp_walk_args_ok(prm, nreads, cs, start, roff, score, nsites, key, poff, npairs)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && (prow_off[0] != 0 || !csr_offsets_ok(prow_off, npairs) || prow_off[npairs] != nrows)) return NMOD_ERR_INVALID_ARG;
  if (nrows > 0 && (npairs == 0 || nreads == 0)) return NMOD_ERR_INVALID_ARG;
  if (nrows == 0) return NMOD_OK;
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t nr = (size_t)nreads, np = (size_t)npairs, nw = (size_t)nrows;
  const size_t tot = host ? (size_t)roff[nreads] : 0;

  SpRowArgs a;
  memset(&a, 0, sizeof(a));
  sp_walk_args(a, nreads, cs, start, roff, score, nsites, key, poff, npairs);
  a.prow_off = prow_off; a.nrows = nrows;

  // one slab: the read lists, the cursors, per slot its key, its number and its two scores, the sort's second buffers and scratch; for
  // the host entry the inputs and outputs as well
  Slab slab(host);
  const ReadListSpace lists(slab, nr);
  const size_t o_cursor = slab.take(np * 4), o_keys = slab.take(nw * 8), o_keys2 = slab.take(nw * 8), o_vals = slab.take(nw * 4),
               o_vals2 = slab.take(nw * 4), o_ta = slab.take(nw * 8), o_tb = slab.take(nw * 8), o_sort = slab.take(rs_scratch_bytes(nrows));
  sp_walk_stage(slab, a, tot);
  slab.in(a.prow_off, (np + 1) * 8);
  slab.out(sa, nw * 8); slab.out(sb, nw * 8); slab.out(read, nw * 4);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.cursor = slab.at<int32_t>(o_cursor);
  a.keys = slab.at<uint64_t>(o_keys); a.vals = slab.at<uint32_t>(o_vals);
  a.ta = slab.at<double>(o_ta); a.tb = slab.at<double>(o_tb);

  NMOD_HIP(hipMemsetAsync(a.cursor, 0, np * 4, stream));
  const unsigned row_grid = persistent_grid(nrows, 256, (int64_t)num_cus * 16);
  hipLaunchKernelGGL(lr_init_kernel, dim3(row_grid), dim3(256), 0, stream, a.keys, a.vals, nrows);
  NMOD_HIP(lists.fill(slab, a.roff, nreads, num_cus, stream, a.w));
  sp_launch_rows<true>(a, num_cus, stream);
  // pair << 32 | read ascending: the slots of a pair are contiguous already, the sort puts them in the order of the reads
  NMOD_HIP(rs_sort_pairs(a.keys, a.vals, slab.at<uint64_t>(o_keys2), slab.at<uint32_t>(o_vals2), nrows, slab.at<char>(o_sort), stream));
  hipLaunchKernelGGL(lr_gather_kernel, dim3(row_grid), dim3(256), 0, stream, (const uint64_t*)a.keys, (const uint32_t*)a.vals, (const double*)a.ta,
                     (const double*)a.tb, nrows, sa, sb, read);
  return launches_end(slab, stream);
}
