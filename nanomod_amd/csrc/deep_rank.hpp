// K1, deep form (NMOD_FLAG_DEEP): positions with a group beyond NMOD_MAX_RANKED (65 535) samples and both groups within
// NMOD_MAX_DEEP (2^24 - 1).  NanoMod tests whatever coverage it is given (getKStest hands both groups to scipy,
// myDetect.py:327-363); amplicon and plasmid runs put more than 65 535 reads on a base.  big_rank_kernel (one workgroup per
// position, a bitonic network in HBM) would leave most of the machine idle on a few such positions, so this form spreads
// every position over many workgroups.  The deep positions of a batch are cut into tiles of kDeepTile keys (each group padded
// with +inf to whole tiles) and processed in rounds of at most kDeepRoundTiles tiles (2^27 keys, at least one position):
//   1. deep_tile_kernel   one workgroup per tile: loads the samples as keys (float32 for float32 / int16 input, float64 for
//                         NMOD_DTYPE_F64 — no probe, no redo), the tile's fp64 sum, the non-finite check, a bitonic sort in LDS;
//   2. deep_mean_kernel   one workgroup per position: the group sums from the tile sums (fixed order: deterministic);
//      deep_q_kernel      one workgroup per tile: sum (x - mean)^2 of its keys (the two-pass fp64 moments of big_rank.hpp);
//   3. deep_merge_kernel  log2(group / tile) merge-path passes over the whole round, 2 048 outputs per workgroup: every pass
//                         splits every position's output over many workgroups (the split of a workgroup's range is found once,
//                         its inputs staged in LDS);
//   4. deep_rank_kernel   one workgroup per tile of sorted keys: every run end of group 2 ranks itself into group 1 by binary
//                         search and applies big_rank_kernel's per-run formulas (rank sum, tie term, the KS candidates in
//                         ks_2samp's float form and as the exact integer numerator); group 1's own ties from its run ends;
//                         partial results go to per-position 64-bit slots by atomics;
//   5. deep_finalize_kernel  one thread per position: finalize_position (pvalue_kernels.hpp) on these facts.
// Bounds (n0, n1 <= NMOD_MAX_DEEP = 2^24 - 1, so that every quantity below is exact):
//   * KS numerator |c0 n1 - c1 n0| <= n0 n1 < 2^48: exact in uint64 and in fp64 (the rational D is one correctly rounded division);
//   * mwu_s = sum over group 1 of (#{b < a} + #{b <= a}) <= 2 n0 n1 < 2^49, i.e. twice the rank sum's part beyond
//     n0 (n0 + 1) / 2 (U = n0 n1 - mwu_s / 2): exact in fp64, as scipy's float64 sum of half-integer ranks is;
//   * the tie term sum (t^3 - t) <= (n0 + n1)^3 < 2^75: accumulated exactly as a 128-bit (hi, lo) pair of uint64 — the
//     per-run terms from 64 x 64 -> 128 products, the slots with carry — and converted to fp64 once, correctly rounded;
//   * ranks and counts fit int32 / int64 everywhere; the sample sums are fp64 as in every other form.
// Scratch (ping-pong key buffers of one round, per-tile sums, per-position slots) comes from the library's pool, sized from
// the classifier's totals in the round trip the large-position pass already makes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "rank_stats.hpp"
#include "big_rank.hpp"
#include "pvalue_kernels.hpp"

namespace nmod {

constexpr int kDeepThreads = kBigThreads;                 // 256 (big_bitonic and big_block_sum assume it)
constexpr int kDeepTileShift = 13;
constexpr int kDeepTile = 1 << kDeepTileShift;             // keys per tile: 32 KB of fp32 / 64 KB of fp64 keys in LDS
constexpr int kDeepMergePer = 8;                           // merge outputs per thread
constexpr int kDeepChunk = kDeepThreads * kDeepMergePer;   // merge outputs per workgroup (divides kDeepTile)
constexpr int64_t kDeepMaxPosTiles = 2 * (((int64_t)NMOD_MAX_DEEP + kDeepTile - 1) >> kDeepTileShift);   // 4 096
constexpr int64_t kDeepRoundTiles = ((int64_t)1 << 27) >> kDeepTileShift;                             // 16 384 tiles = 2^27 keys
constexpr int64_t kDeepRoundStride = kDeepRoundTiles - kDeepMaxPosTiles;   // a round takes the positions that START in its stride
static_assert(kDeepTile % kDeepChunk == 0 && kDeepRoundStride > 0, "deep tiles");

// per deep position (index in the deep list), cleared before the batch
struct DeepAcc {
  unsigned long long s;                 // mwu_s
  unsigned long long tie_lo, tie_hi;    // sum (t^3 - t), 128 bits
  unsigned long long ks_num;            // max |c0 n1 - c1 n0|
  unsigned long long dmax_bits;         // max |fl(c0/n0) - fl(c1/n1)| (non-negative doubles order like their bits)
  unsigned int nonfinite, pad;
  double sum[2];                        // sample sums per group (key units)
};

struct DeepArgs {
  const void* sig0; const void* sig1; const int64_t* off0; const int64_t* off1; int64_t stride0, stride1;
  const int32_t* pos_list; const int32_t* class_meta; int32_t deep_class;    // the deep list: class deep_class of the binning
  int64_t ndeep;
  int64_t* ptile;                       // [ndeep + 1] first tile of each position, ptile[ndeep] = all tiles
  int64_t* roundtab;                    // [nrounds + 1] first tile of each round, roundtab[nrounds] = all tiles
  int32_t nrounds, round;
  const void* src; void* dst;           // key buffers of the round (tile / merge / rank kernels)
  int64_t width;                        // merge pass: length of the sorted runs it merges
  double* tile_sum; double* tile_q;     // [all tiles]
  DeepAcc* acc;
  int32_t all;
};

struct DeepSeg {                        // the segment (position, group) a tile belongs to
  int64_t i; int64_t pos; int g;
  int64_t o, n;                         // sample offset and count of the group
  int64_t n_other;                      // the other group's count
  int64_t tile0;                        // first tile of the segment (global)
  int64_t pos_tile0;                    // first tile of the position
  int64_t tiles0;                       // tiles of group 1
};

__host__ __device__ inline int64_t deep_tiles(int64_t n) { return (n + kDeepTile - 1) >> kDeepTileShift; }

__device__ __forceinline__ const int32_t* deep_list(const DeepArgs& a) { return a.pos_list + a.class_meta[kClassStride + a.deep_class]; }

__device__ __forceinline__ void deep_rows(const DeepArgs& a, int64_t pos, int64_t& o0, int64_t& n0, int64_t& o1, int64_t& n1) {
  if (a.stride0 > 0) { o0 = pos * a.stride0; n0 = a.stride0; } else { o0 = a.off0[pos]; n0 = a.off0[pos + 1] - o0; }
  if (a.stride1 > 0) { o1 = pos * a.stride1; n1 = a.stride1; } else { o1 = a.off1[pos]; n1 = a.off1[pos + 1] - o1; }
}

// the position that holds global tile t: the largest i with ptile[i] <= t (ptile[0] = 0, strictly increasing)
__device__ __forceinline__ int64_t deep_find(const int64_t* ptile, int64_t n, int64_t t) {
  int64_t lo = 0, hi = n;                                      // first i in [0, n) with ptile[i] > t, minus one
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (ptile[mid] <= t) lo = mid + 1; else hi = mid; }
  return lo - 1;
}

__device__ __forceinline__ DeepSeg deep_seg(const DeepArgs& a, int64_t t) {
  DeepSeg s;
  s.i = deep_find(a.ptile, a.ndeep, t);
  s.pos = deep_list(a)[s.i];
  int64_t o0, n0, o1, n1;
  deep_rows(a, s.pos, o0, n0, o1, n1);
  s.pos_tile0 = a.ptile[s.i];
  s.tiles0 = deep_tiles(n0);
  s.g = (t - s.pos_tile0 < s.tiles0) ? 0 : 1;
  s.o = s.g ? o1 : o0; s.n = s.g ? n1 : n0; s.n_other = s.g ? n0 : n1;
  s.tile0 = s.pos_tile0 + (s.g ? s.tiles0 : 0);
  return s;
}

// ---- 128-bit unsigned sums (the tie term)
struct DeepU128 { unsigned long long lo, hi; };
__device__ __forceinline__ void u128_add(DeepU128& x, DeepU128 y) {
  const unsigned long long lo = x.lo + y.lo;
  x.hi += y.hi + (lo < x.lo ? 1ull : 0ull);
  x.lo = lo;
}
__device__ __forceinline__ DeepU128 u128_mul(unsigned long long a, unsigned long long b) {
  DeepU128 r; r.lo = a * b; r.hi = __umul64hi(a, b); return r;
}
__device__ __forceinline__ DeepU128 u128_sub_small(DeepU128 x, unsigned long long y) {
  DeepU128 r; r.lo = x.lo - y; r.hi = x.hi - (x.lo < y ? 1ull : 0ull); return r;
}
__device__ __forceinline__ DeepU128 t3_minus_t(unsigned long long t) { return u128_sub_small(u128_mul(t * t, t), t); }   // t < 2^26
// correctly rounded: the top 64 bits with a sticky bit for the rest, converted once, scaled exactly
__device__ __forceinline__ double u128_to_double(DeepU128 x) {
  if (x.hi == 0ull) return (double)x.lo;
  const int sh = 64 - __clzll((long long)x.hi);               // 1 .. 64
  if (sh == 64) {
    const unsigned long long top = x.hi | (x.lo != 0ull ? 1ull : 0ull);
    return ldexp((double)top, 64);
  }
  const unsigned long long top = (x.hi << (64 - sh)) | (x.lo >> sh) | ((x.lo << (64 - sh)) != 0ull ? 1ull : 0ull);
  return ldexp((double)top, sh);
}

// ---------------------------------------------------------------- 0. the tile table (one workgroup)
constexpr int kDeepPlanThreads = 1024;
__global__ __launch_bounds__(kDeepPlanThreads) void deep_plan_kernel(DeepArgs a) {
  __shared__ int64_t sh[kDeepPlanThreads];
  const int tid = threadIdx.x;
  const int32_t* list = deep_list(a);
  int64_t carry = 0;
  for (int64_t base = 0; base < a.ndeep; base += kDeepPlanThreads) {
    const int64_t i = base + tid;
    int64_t v = 0;
    if (i < a.ndeep) { int64_t o0, n0, o1, n1; deep_rows(a, list[i], o0, n0, o1, n1); v = deep_tiles(n0) + deep_tiles(n1); }
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < kDeepPlanThreads; d <<= 1) {          // inclusive scan
      const int64_t add = tid >= d ? sh[tid - d] : 0;
      __syncthreads();
      sh[tid] += add;
      __syncthreads();
    }
    if (i < a.ndeep) a.ptile[i] = carry + sh[tid] - v;
    carry += sh[kDeepPlanThreads - 1];
    __syncthreads();
  }
  if (tid == 0) a.ptile[a.ndeep] = carry;
  __threadfence();
  __syncthreads();
  for (int r = tid; r <= a.nrounds; r += kDeepPlanThreads) {
    const int64_t start = (int64_t)r * kDeepRoundStride;
    int64_t lo = 0, hi = a.ndeep;                                // first i with ptile[i] >= start (ndeep: none)
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (a.ptile[mid] < start) lo = mid + 1; else hi = mid; }
    a.roundtab[r] = (r == a.nrounds || lo >= a.ndeep) ? carry : a.ptile[lo];
  }
}

// ---------------------------------------------------------------- 1. keys, tile sums, tile sort
template <int DTYPE>
__global__ __launch_bounds__(kDeepThreads) void deep_tile_kernel(DeepArgs a) {
  typedef typename BigKey<DTYPE>::type K;
  extern __shared__ __attribute__((aligned(16))) unsigned char deep_lds[];
  K* keys = reinterpret_cast<K*>(deep_lds);
  __shared__ double red[kDeepThreads / 64];
  const int tid = threadIdx.x;
  const int64_t t0 = a.roundtab[a.round], t1 = a.roundtab[a.round + 1];
  const K inf = (K)__builtin_inff();
  K* dst = reinterpret_cast<K*>(a.dst);
  for (int64_t t = t0 + blockIdx.x; t < t1; t += gridDim.x) {
    const DeepSeg s = deep_seg(a, t);
    const void* sig = s.g ? a.sig1 : a.sig0;
    const int64_t first = (t - s.tile0) << kDeepTileShift;    // first sample of the tile within its group
    double sum = 0.0;
    bool bad = false;
    for (int k = tid; k < kDeepTile; k += kDeepThreads) {
      const int64_t j = first + k;
      K v = inf;
      if (j < s.n) {
        v = big_load<DTYPE>(sig, s.o + j);
        sum += (double)v;
        if constexpr (DTYPE != 1) bad = bad || !(fabs((double)v) <= 1.7976931348623157e308);
      }
      keys[k] = v;
    }
    sum = big_block_sum(sum, red);                              // (its barriers also order the LDS stores above)
    if (tid == 0) a.tile_sum[t] = sum;
    if (__ballot(bad) != 0ull && (tid & 63) == 0) atomicOr(&a.acc[s.i].nonfinite, 1u);
    big_bitonic(keys, kDeepTile);
    K* out = dst + ((t - t0) << kDeepTileShift);
    for (int k = tid; k < kDeepTile; k += kDeepThreads) out[k] = keys[k];
    __syncthreads();
  }
}

// ---------------------------------------------------------------- 2. moments: group sums (per position), sum (x - mean)^2 (per tile)
__global__ __launch_bounds__(kDeepThreads) void deep_mean_kernel(DeepArgs a) {
  __shared__ double red[kDeepThreads / 64];
  const int64_t t0 = a.roundtab[a.round], t1 = a.roundtab[a.round + 1];
  if (t0 >= t1) return;
  const int64_t i0 = deep_find(a.ptile, a.ndeep, t0), i1 = deep_find(a.ptile, a.ndeep, t1 - 1) + 1;
  for (int64_t i = i0 + blockIdx.x; i < i1; i += gridDim.x) {
    int64_t o0, n0, o1, n1;
    deep_rows(a, deep_list(a)[i], o0, n0, o1, n1);
    const int64_t tiles0 = deep_tiles(n0), tiles1 = deep_tiles(n1);
    for (int g = 0; g < 2; ++g) {
      const int64_t b = a.ptile[i] + (g ? tiles0 : 0), nt = g ? tiles1 : tiles0;
      double s = 0.0;
      for (int64_t k = threadIdx.x; k < nt; k += kDeepThreads) s += a.tile_sum[b + k];
      s = big_block_sum(s, red);
      if (threadIdx.x == 0) a.acc[i].sum[g] = s;
    }
  }
}

template <int DTYPE>
__global__ __launch_bounds__(kDeepThreads) void deep_q_kernel(DeepArgs a) {
  typedef typename BigKey<DTYPE>::type K;
  __shared__ double red[kDeepThreads / 64];
  const int64_t t0 = a.roundtab[a.round], t1 = a.roundtab[a.round + 1];
  const K* src = reinterpret_cast<const K*>(a.src);
  for (int64_t t = t0 + blockIdx.x; t < t1; t += gridDim.x) {
    const DeepSeg s = deep_seg(a, t);
    const double mu = a.acc[s.i].sum[s.g] / (double)s.n;
    const int64_t first = (t - s.tile0) << kDeepTileShift;
    const K* in = src + ((t - t0) << kDeepTileShift);
    const int valid = (int)min((int64_t)kDeepTile, s.n - first);   // the tile's valid keys sort first (the pads are +inf)
    double q = 0.0;
    for (int k = threadIdx.x; k < valid; k += kDeepThreads) { const double d = (double)in[k] - mu; q += d * d; }
    q = big_block_sum(q, red);
    if (threadIdx.x == 0) a.tile_q[t] = q;
  }
}

// ---------------------------------------------------------------- 3. merge-path passes
// i = how many of the first d outputs of merge(A, B) come from A (A first on ties)
template <typename K>
__device__ __forceinline__ int64_t deep_merge_path(const K* A, int64_t la, const K* B, int64_t lb, int64_t d) {
  int64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (A[mid] <= B[d - 1 - mid]) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <int DTYPE>
__global__ __launch_bounds__(kDeepThreads) void deep_merge_kernel(DeepArgs a) {
  typedef typename BigKey<DTYPE>::type K;
  __shared__ K stage[kDeepChunk];
  __shared__ int64_t split[2];
  const int tid = threadIdx.x;
  const int64_t t0 = a.roundtab[a.round], t1 = a.roundtab[a.round + 1];
  const int64_t nchunks = ((t1 - t0) << kDeepTileShift) / kDeepChunk;
  const K* src = reinterpret_cast<const K*>(a.src);
  K* dst = reinterpret_cast<K*>(a.dst);
  const int64_t W = a.width;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t k0 = c * kDeepChunk;                          // round-local index of the chunk's first output
    const DeepSeg s = deep_seg(a, t0 + (k0 >> kDeepTileShift));
    const int64_t seg = (s.tile0 - t0) << kDeepTileShift;     // round-local start of the segment
    const int64_t len = deep_tiles(s.n) << kDeepTileShift;    // padded length
    const int64_t l0 = k0 - seg;
    const int64_t b = l0 / (2 * W) * (2 * W);                  // the pair of runs this chunk's outputs come from
    const int64_t la = min(W, len - b), lb = max((int64_t)0, min(W, len - b - W));
    const K* A = src + seg + b;
    const K* B = A + la;
    const int64_t d0 = l0 - b;
    if (tid < 2) split[tid] = deep_merge_path(A, la, B, lb, d0 + tid * kDeepChunk);
    __syncthreads();
    const int64_t ia = split[0], ja = d0 - ia;                  // the chunk takes A[ia, ib) and B[ja, jb)
    const int na = (int)(split[1] - ia), nb = kDeepChunk - na;
    for (int k = tid; k < kDeepChunk; k += kDeepThreads) stage[k] = k < na ? A[ia + k] : B[ja + (k - na)];
    __syncthreads();
    const K* sa = stage; const K* sb = stage + na;
    const int d = tid * kDeepMergePer;
    int i = (int)deep_merge_path(sa, (int64_t)na, sb, (int64_t)nb, (int64_t)d), j = d - i;
    K* out = dst + k0 + d;
#pragma unroll
    for (int e = 0; e < kDeepMergePer; ++e) {
      const bool take_a = j >= nb || (i < na && sa[i] <= sb[j]);
      out[e] = take_a ? sa[i] : sb[j];
      if (take_a) ++i; else ++j;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- 4. ranks, ties, KS candidates
template <typename K>
__device__ __forceinline__ int64_t deep_lower(const K* s, int64_t lo, int64_t hi, K x) {    // first index in [lo, hi) with s >= x
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (s[mid] < x) lo = mid + 1; else hi = mid; }
  return lo;
}
template <typename K>
__device__ __forceinline__ int64_t deep_upper(const K* s, int64_t lo, int64_t hi, K x) {    // first index in [lo, hi) with s > x
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (s[mid] <= x) lo = mid + 1; else hi = mid; }
  return lo;
}
__device__ __forceinline__ unsigned long long deep_wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const unsigned long long o = __shfl_xor(v, m); v = o > v ? o : v; }
  return v;
}

template <int DTYPE>
__global__ __launch_bounds__(kDeepThreads) void deep_rank_kernel(DeepArgs a) {
  typedef typename BigKey<DTYPE>::type K;
  const int tid = threadIdx.x;
  const int64_t t0 = a.roundtab[a.round], t1 = a.roundtab[a.round + 1];
  const K* src = reinterpret_cast<const K*>(a.src);
  for (int64_t t = t0 + blockIdx.x; t < t1; t += gridDim.x) {
    const DeepSeg s = deep_seg(a, t);
    const K* A = src + ((s.pos_tile0 - t0) << kDeepTileShift);   // group 1, sorted (m keys)
    const K* B = A + (s.tiles0 << kDeepTileShift);              // group 2, sorted (q keys)
    const int64_t m = s.g ? s.n_other : s.n, q = s.g ? s.n : s.n_other;
    const int64_t first = (t - s.tile0) << kDeepTileShift;
    const int64_t last = min(first + kDeepTile, s.n);
    const double dm = (double)m, dq = (double)q;
    unsigned long long s_acc = 0ull, best = 0ull;
    DeepU128 t_acc = {0ull, 0ull};
    double dmax = 0.0;
    if (s.g == 1) {
      // every run end of group 2: its run [js, je) and its ranks [L, U) in group 1 (formulas: big_rank_kernel)
      for (int64_t j = first + tid; j < last; j += kDeepThreads) {
        const K x = B[j];
        if (j + 1 < q && B[j + 1] == x) continue;
        const int64_t js = (j > 0 && B[j - 1] == x) ? deep_lower(B, (int64_t)0, j, x) : j, je = j + 1;
        const int64_t L = deep_lower(A, (int64_t)0, m, x);
        const int64_t U = (L < m && A[L] == x) ? deep_upper(A, L, m, x) : L;
        const unsigned long long ta = (unsigned long long)(U - L), tb = (unsigned long long)(je - js);
        s_acc += tb * (unsigned long long)(2 * m - U - L);
        if (tb > 1ull) u128_add(t_acc, t3_minus_t(tb));
        if (ta > 0ull) u128_add(t_acc, u128_mul(ta * tb, 3ull * (ta + tb)));
        const double d_at = (double)U / dm - (double)je / dq;       // ks_2samp's float form: fl(c0/n0) - fl(c1/n1)
        const double d_before = (double)L / dm - (double)js / dq;
        dmax = fmax(dmax, fmax(fabs(d_at), fabs(d_before)));
        const long long n_at = (long long)U * q - (long long)je * m, n_before = (long long)L * q - (long long)js * m;
        const unsigned long long m_at = (unsigned long long)(n_at < 0 ? -n_at : n_at);
        const unsigned long long m_before = (unsigned long long)(n_before < 0 ? -n_before : n_before);
        best = max(best, max(m_at, m_before));
      }
    } else if (a.all) {
      // runs of group 1: a^3 - a each
      for (int64_t i = first + tid; i < last; i += kDeepThreads) {
        const K x = A[i];
        if (i + 1 < m && A[i + 1] == x) continue;
        if (i == 0 || A[i - 1] != x) continue;
        const unsigned long long ta = (unsigned long long)(i + 1 - deep_lower(A, (int64_t)0, i, x));
        u128_add(t_acc, t3_minus_t(ta));
      }
    }
    DeepAcc& acc = a.acc[s.i];
    if (t_acc.lo | t_acc.hi) {                                   // (run ends with ties: rare on continuous data)
      const unsigned long long old = atomicAdd(&acc.tie_lo, t_acc.lo);
      const unsigned long long hi = t_acc.hi + (old + t_acc.lo < old ? 1ull : 0ull);
      if (hi) atomicAdd(&acc.tie_hi, hi);
    }
    if (s.g == 1) {
      const unsigned long long ws = wave_sum_u64(s_acc), wb = deep_wave_max_u64(best);
      const double wd = wave_max_f64(dmax);
      if ((tid & 63) == 0) {
        if (ws) atomicAdd(&acc.s, ws);
        atomicMax(&acc.ks_num, wb);
        atomicMax(&acc.dmax_bits, (unsigned long long)__double_as_longlong(wd));
      }
    }
  }
}

// ---------------------------------------------------------------- 5. outputs
struct DeepFacts {
  double d_float; unsigned long long num; int rational; double s, tie_v; double mo[4]; bool nf;
  __device__ __forceinline__ double ks_d(double prod) const { return rational ? (double)num / prod : d_float; }
  __device__ __forceinline__ double mwu_s() const { return s; }
  __device__ __forceinline__ double tie() const { return tie_v; }
  __device__ __forceinline__ const double* moments() const { return mo; }
  __device__ __forceinline__ bool nonfinite() const { return nf; }
};

template <int DTYPE>
__global__ __launch_bounds__(256) void deep_finalize_kernel(DeepArgs a, FinalizeArgs fa, int32_t ks_rational, int32_t check_finite) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.ndeep) return;
  const int64_t pos = deep_list(a)[i];
  int64_t o0, n0, o1, n1;
  deep_rows(a, pos, o0, n0, o1, n1);
  const DeepAcc& acc = a.acc[i];
  DeepFacts f;
  f.d_float = __longlong_as_double((long long)acc.dmax_bits);
  f.num = acc.ks_num; f.rational = ks_rational;
  f.s = (double)acc.s;                                         // < 2^49: exact
  const DeepU128 tie = {acc.tie_lo, acc.tie_hi};
  const int64_t size_i = n0 + n1;
  const DeepU128 full = t3_minus_t((unsigned long long)size_i);
  const double size = (double)(n0 + n1);
  // one run over the whole pool (every sample identical): the same fp64 expression K2 divides by, so that T is exactly 0
  f.tie_v = (tie.lo == full.lo && tie.hi == full.hi) ? size * size * size - size : u128_to_double(tie);
  const int64_t tiles0 = deep_tiles(n0);
  for (int g = 0; g < 2; ++g) {
    const int64_t n = g ? n1 : n0, b = a.ptile[i] + (g ? tiles0 : 0), nt = deep_tiles(n);
    double q = 0.0;
    if (a.all) for (int64_t k = 0; k < nt; ++k) q += a.tile_q[b + k];
    if constexpr (DTYPE == 1) { f.mo[2 * g] = acc.sum[g] / 1000.0 / (double)n; f.mo[2 * g + 1] = q * 1e-6; }
    else { f.mo[2 * g] = acc.sum[g] / (double)n; f.mo[2 * g + 1] = q; }
  }
  f.nf = check_finite && acc.nonfinite != 0u;
  finalize_position(fa, pos, n0, n1, false, f);
}

}  // namespace nmod
