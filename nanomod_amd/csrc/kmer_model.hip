// nmod_kmer_model — pool the events of a control run into per-k-mer level models on the device (K10).  The
// reference project has no such step; the definition is the one in include/nanomod_hip.h (tests/kmer_ref.py restates it with
// Python integers and math.fsum).  All on the caller's stream.
//
// int16 (the hot path: events are int16-exact and the library narrows to it), one streaming pass:
//   km_bounds_kernel      (with keep bounds) a thread per code: the bounds as the exact integer range of k that k / 1000.0 keeps
//   km_i16_kernel         persistent waves, a tile of 64 consecutive positions per wave.  The rows of a tile are one contiguous
//                         run of the sample vector, so the wave walks that run in aligned 16-byte pieces, a piece per lane,
//                         whatever the row lengths are: a 3-sample row costs 3 samples of a load, not a wave.  A lane finds the
//                         row of its first sample by a search over the tile's 64 row ends (LDS).  Without bounds a piece is
//                         reduced by masked dot products, split at the first row end in it; a piece that touches more than two
//                         rows, and every piece under bounds, goes a sample at a time.  Rows that end inside a lane's piece go
//                         to the table at once; the open partial of every lane is summed over the lanes of its row by a
//                         segmented DPP scan, and the last lane of each row adds it.
//                         The table (N, S1, S2, clipped, positions per code) is integer: privatised in LDS up to 4 096 codes
//                         and flushed with 64-bit global atomics (non-zero entries only), in global memory beyond.
//   km_finish_i16_kernel  a thread per code: mean and sd from (N, S1, S2) in 128-bit integers
// Integer sums do not depend on their order: the int16 outputs are the same bits for any order of the positions.
//
// float32 / float64 (not the hot path):
//   km_moments_kernel     a wave per position: kept count, mean, M2 (corrected two-pass in fp64), the sort key (its code)
//   rs_sort_pairs         stable grouping of the position indices by code (one to three one-byte passes)
//   km_combine_kernel     a wave per code: lane l chains the code's positions l, l + 64, ... in their order with the pairwise
//                         update, then a fixed tree over the lanes.  No float atomics: a code's bits depend on its positions
//                         and their relative order only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "entry_device.hpp"
#include "radix_sort.hpp"
#include "special_math.hpp"

namespace nmod {

constexpr int kKmThreads = 1024;                  // km_i16_kernel: sixteen waves
constexpr int kKmWaves = kKmThreads / 64;
constexpr int kKmTile = 64;                       // positions per wave tile: one per lane
constexpr int kKmVec = 8;                         // int16 samples per lane and step: one aligned 16-byte load
constexpr int kKmStep = 64 * kKmVec;              // samples per wave and step
constexpr int kKmLdsCodes = 4096;                 // the table lives in LDS up to here: 28 bytes per code = 112 KiB
constexpr int kKmLdsBytesPerCode = 28;            // S1, S2 (64-bit), N, positions, clipped (32-bit)

struct KmArgs {
  const void* sig; const int64_t* off; int64_t stride; const int32_t* code;
  int64_t npos; int32_t ncodes;
  const double* keep_lo; const double* keep_hi;   // device; both or neither
  const int2* kbound;                             // int16: per code the kept range of k, .x <= k <= .y
  unsigned long long* acc;                        // int16: 5 x ncodes words: N, S1, S2, positions, clipped
  uint8_t* pos_status;
  // float path
  double* pmean; double* pm2; int32_t* pn; int32_t* pcl; uint64_t* key; uint32_t* val;
  nmod_kmer_out out;
};

__device__ __forceinline__ void km_row(const KmArgs& a, int64_t i, int64_t& begin, int64_t& end) {
  if (a.off) { begin = a.off[i]; end = a.off[i + 1]; } else { begin = i * a.stride; end = begin + a.stride; }
}

// the position's code (-1: takes no part) and its status from code and size
__device__ __forceinline__ unsigned km_classify(const KmArgs& a, int64_t p, int64_t n, int& c) {
  unsigned st = 0;
  c = a.code[p];
  if (c < 0 || c >= a.ncodes) st |= NMOD_STATUS_NO_CODE;
  if (n <= 0) st |= NMOD_STATUS_EMPTY;
  if (n > (int64_t)NMOD_MAX_DEEP) st |= NMOD_STATUS_TOO_LARGE;
  if (st) c = -1;
  return st;
}

__device__ __forceinline__ void km_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------------------------------------------------------- int16

// keep_lo <= k / 1000.0 <= keep_hi as lo_k <= k <= hi_k: the predicate is monotone in k, so a search over the 65 536 values of
// k gives the exact range (a NaN bound: an empty one)
__global__ __launch_bounds__(256) void km_bounds_kernel(const double* keep_lo, const double* keep_hi, int ncodes, int2* kbound) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncodes) return;
  const double lo = keep_lo[c], hi = keep_hi[c];
  int first_ge = -32768, first_gt = -32768;        // first k with k / 1000.0 >= lo; first k with !(k / 1000.0 <= hi)
  for (int step = 65536; step; step >>= 1) {
    const int k = first_ge + step - 1;
    if (k <= 32767 && !((double)k / 1000.0 >= lo)) first_ge = k + 1;
  }
  for (int step = 65536; step; step >>= 1) {
    const int k = first_gt + step - 1;
    if (k <= 32767 && ((double)k / 1000.0 <= hi)) first_gt = k + 1;
  }
  kbound[c] = make_int2(first_ge, first_gt - 1);
}

template <bool LDS_TABLE>
struct KmTable {
  unsigned long long* s1; unsigned long long* s2;             // LDS_TABLE: LDS words, else the global words
  unsigned* n; unsigned* pos; unsigned* cl;                   // LDS_TABLE only
  unsigned long long* gn; unsigned long long* gpos; unsigned long long* gcl;
  __device__ __forceinline__ void add(int c, unsigned n_, unsigned cl_, long long s1_, unsigned long long s2_) const {
    if constexpr (LDS_TABLE) {
      if (n_) { atomicAdd(&n[c], n_); atomicAdd(&s1[c], (unsigned long long)s1_); atomicAdd(&s2[c], s2_); }
      if (cl_) atomicAdd(&cl[c], cl_);
    } else {
      if (n_) { atomicAdd(&gn[c], (unsigned long long)n_); atomicAdd(&s1[c], (unsigned long long)s1_); atomicAdd(&s2[c], s2_); }
      if (cl_) atomicAdd(&gcl[c], (unsigned long long)cl_);
    }
  }
  __device__ __forceinline__ void add_position(int c) const {
    if constexpr (LDS_TABLE) atomicAdd(&pos[c], 1u); else atomicAdd(&gpos[c], 1ull);
  }
};

struct KmPart { unsigned n; int s1; unsigned long long s2; };

typedef short km_short2 __attribute__((ext_vector_type(2)));

// n, sum and sum of squares of the int16 samples of four words whose 16-bit field in `m` is set.  A pair of squares is at most
// 2^31: exact in the 32 bits of the dot product read as unsigned
__device__ __forceinline__ KmPart km_masked_sums(const int (&w)[4], const uint4& m) {
  const unsigned mm[4] = {m.x, m.y, m.z, m.w};
  KmPart r = {0u, 0, 0ull};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int v = w[d] & (int)mm[d];
    const km_short2 pv = __builtin_bit_cast(km_short2, v);
    r.n += (unsigned)__popc(mm[d]);
    r.s1 = __builtin_amdgcn_sdot2(pv, __builtin_bit_cast(km_short2, 0x00010001), r.s1, false);
    r.s2 += (unsigned long long)(unsigned)__builtin_amdgcn_sdot2(pv, pv, 0, false);
  }
  r.n >>= 4;
  return r;
}

// Inclusive scan of (s1, px) over the lanes of equal key.  Equal keys are neighbours, so a source lane of the same key means
// every lane between has it too.  Four steps inside the rows of 16 lanes, then lane 15 of rows 0 and 2 into rows 1 and 3, then
// lane 31 into rows 2 and 3 (ks_rank.hpp: seg_exscan_add_u32).  A lane without a source reads the key -2, which no lane has
__device__ __forceinline__ void km_seg_scan(int key, int& s1, unsigned long long& px, int lane) {
  auto step = [&](auto tag, auto rows) {
    constexpr int C = decltype(tag)::value;
    constexpr int RM = decltype(rows)::value;
    const int ok = dpp_i<C, RM>(-2, key);
    const int o1 = dpp_i<C, RM>(0, s1);
    const unsigned lo = (unsigned)dpp_i<C, RM>(0, (int)(unsigned)px), hi = (unsigned)dpp_i<C, RM>(0, (int)(unsigned)(px >> 32));
    const bool take = ok == key;
    s1 += take ? o1 : 0;
    px += take ? (((unsigned long long)hi << 32) | lo) : 0ull;
  };
  using All = std::integral_constant<int, 0xf>;
  step(std::integral_constant<int, kDppRowShr + 1>{}, All{});
  step(std::integral_constant<int, kDppRowShr + 2>{}, All{});
  step(std::integral_constant<int, kDppRowShr + 4>{}, All{});
  step(std::integral_constant<int, kDppRowShr + 8>{}, All{});
  step(std::integral_constant<int, kDppRowBcast15>{}, std::integral_constant<int, 0xA>{});
  step(std::integral_constant<int, kDppRowBcast31>{}, std::integral_constant<int, 0xC>{});
}

template <bool LDS_TABLE, bool CLIP>
__global__ __launch_bounds__(kKmThreads) void km_i16_kernel(KmArgs a) {
  extern __shared__ unsigned long long km_lds[];
  __shared__ long long w_end[kKmWaves][kKmTile];              // per wave: the row ends of its tile,
  __shared__ int w_code[kKmWaves][kKmTile];                   // their codes (-1: the row takes no part),
  __shared__ int2 w_bound[kKmWaves][kKmTile];                 // kept ranges
  __shared__ unsigned w_kept[kKmWaves][kKmTile];              // and whether a sample of the row was kept
  __shared__ uint4 prefix[kKmVec + 1];                        // [k]: the 16-bit fields of the samples 0 .. k - 1 of a piece set
  if (threadIdx.x <= kKmVec) {
    const int k = threadIdx.x;
    auto word = [k](int d) { const int t = k - 2 * d; return t <= 0 ? 0u : (t == 1 ? 0xFFFFu : 0xFFFFFFFFu); };
    prefix[k] = make_uint4(word(0), word(1), word(2), word(3));
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nc = a.ncodes;
  KmTable<LDS_TABLE> tab;
  tab.gn = a.acc; tab.gpos = a.acc + 3 * (size_t)nc; tab.gcl = a.acc + 4 * (size_t)nc;
  if constexpr (LDS_TABLE) {
    tab.s1 = km_lds; tab.s2 = km_lds + nc;
    tab.n = reinterpret_cast<unsigned*>(km_lds + 2 * (size_t)nc); tab.pos = tab.n + nc; tab.cl = tab.pos + nc;
    for (int c = threadIdx.x; c < nc; c += kKmThreads) { tab.s1[c] = 0; tab.s2[c] = 0; tab.n[c] = 0; tab.pos[c] = 0; tab.cl[c] = 0; }
    __syncthreads();
  } else {
    tab.s1 = a.acc + (size_t)nc; tab.s2 = a.acc + 2 * (size_t)nc;
    tab.n = tab.pos = tab.cl = nullptr;
  }
  long long* ends = w_end[wave];
  int* codes = w_code[wave];
  int2* bounds = w_bound[wave];
  unsigned* kept = w_kept[wave];
  const int16_t* sg = static_cast<const int16_t*>(a.sig);
  const int64_t ntiles = (a.npos + kKmTile - 1) / kKmTile;

  for (int64_t t = (int64_t)blockIdx.x * kKmWaves + wave; t < ntiles; t += (int64_t)gridDim.x * kKmWaves) {
    const int64_t p0 = t * kKmTile;
    const int cnt = (int)(a.npos - p0 < kKmTile ? a.npos - p0 : kKmTile);
    const int64_t p = p0 + lane;
    const bool have = lane < cnt;
    int64_t b = 0, e = 0;
    int c = -1;
    if (have) {
      km_row(a, p, b, e);
      const unsigned st = km_classify(a, p, e - b, c);
      if (a.pos_status) a.pos_status[p] = (uint8_t)st;
    }
    ends[lane] = have ? e : INT64_MAX;
    codes[lane] = c;
    if constexpr (CLIP) bounds[lane] = c >= 0 ? a.kbound[c] : make_int2(0, 0);
    kept[lane] = 0;
    km_wave_sync();
    const int64_t B = __shfl(b, 0), E = __shfl(e, cnt - 1);

    // the tile's samples [B, E) in aligned pieces of kKmVec: the first piece starts at or below B
    const int64_t mis = (int64_t)(((reinterpret_cast<uintptr_t>(sg) >> 1) + (uint64_t)B) & (uint64_t)(kKmVec - 1));
    for (int64_t s0 = B - mis; s0 < E; s0 += kKmStep) {
      const int64_t s = s0 + (int64_t)lane * kKmVec;
      const int64_t lo = s > B ? s : B, hi = s + kKmVec < E ? s + kKmVec : E;
      int key = -1;                                             // the lane's open partial: its row,
      unsigned pn = 0, pcl = 0;
      int ps1 = 0;
      unsigned long long ps2 = 0;
      int w[4] = {0, 0, 0, 0};
      int j = 0;
      bool slow = false;
      if (lo < hi) {
        // the 16 bytes hold at least one sample of [B, E) and are aligned: they lie in a page the vector has
        const int4 raw = *reinterpret_cast<const int4*>(sg + s);
        w[0] = raw.x; w[1] = raw.y; w[2] = raw.z; w[3] = raw.w;
#pragma unroll
        for (int step = 32; step; step >>= 1) if (ends[j + step - 1] <= lo) j += step;   // rows ending at or below lo: lo's row
        slow = CLIP;
        if constexpr (!CLIP) {
          // without bounds: the piece as [lo, min(end of row j, hi)) and the rest, by masked dot products; a piece that
          // touches more than two rows goes the slow way
          const long long ej = ends[j];
          const int ke = (int)((ej < hi ? ej : hi) - s);
          const uint4 plo = prefix[(int)(lo - s)], phi = prefix[(int)(hi - s)], pe = prefix[ke];
          const uint4 in = make_uint4(phi.x & ~plo.x, phi.y & ~plo.y, phi.z & ~plo.z, phi.w & ~plo.w);
          const KmPart all = km_masked_sums(w, in);
          key = j;
          pn = all.n; ps1 = all.s1; ps2 = all.s2;
          if (ej < hi) {
            const int jn = j + 1 < kKmTile ? j + 1 : kKmTile - 1;
            const long long en = ends[jn];
            if (en >= hi && en > ej) {
              const KmPart head = km_masked_sums(w, make_uint4(in.x & pe.x, in.y & pe.y, in.z & pe.z, in.w & pe.w));
              const int cj = codes[j];
              if (cj >= 0) { tab.add(cj, head.n, 0u, (long long)head.s1, head.s2); if (head.n) kept[j] = 1; }
              key = jn;
              pn -= head.n; ps1 -= head.s1; ps2 -= head.s2;
            } else {
              slow = true;
            }
          }
        }
      }
      if (__ballot(slow) != 0ull) {
        if (slow) {                                             // a sample at a time
          long long ej = ends[j];
          int cj = codes[j];
          int2 bj = make_int2(0, 0);
          if constexpr (CLIP) bj = bounds[j];
          pn = pcl = 0; ps1 = 0; ps2 = 0;
#pragma unroll
          for (int k = 0; k < kKmVec; ++k) {
            const int64_t idx = s + k;
            if (idx >= lo && idx < hi) {
              while (idx >= ej) {                               // row j ends inside this piece: its partial goes to the table
                if (cj >= 0) { tab.add(cj, pn, pcl, (long long)ps1, ps2); if (pn) kept[j] = 1; }
                pn = pcl = 0; ps1 = 0; ps2 = 0;
                ++j;
                if (j < kKmTile) { ej = ends[j]; cj = codes[j]; if constexpr (CLIP) bj = bounds[j]; }
                else { j = kKmTile - 1; ej = INT64_MAX; cj = -1; }   // (offsets that decrease: nothing of this is counted)
              }
              const int x = (k & 1) ? (w[k >> 1] >> 16) : (int)(short)(w[k >> 1] & 0xFFFF);
              const bool in = !CLIP || (x >= bj.x && x <= bj.y);
              pn += in ? 1u : 0u;
              pcl += in ? 0u : 1u;
              ps1 += in ? x : 0;
              ps2 += in ? (unsigned long long)(unsigned)(x * x) : 0ull;
            }
          }
          key = j;
        }
      }
      if (key >= 0 && codes[key] < 0) key = -1;
      if (key < 0) { pn = pcl = 0; ps1 = 0; ps2 = 0; }
      // the open partials of the lanes of one row are neighbours: a segmented inclusive scan, then the row's last lane adds.
      // At most 512 samples a step: S1 fits 32 bits, and n (bits 40 up) and clipped (bits 50 up) ride on S2 (below 2^39)
      unsigned long long px = ps2 | ((unsigned long long)pn << 40) | ((unsigned long long)pcl << 50);
      km_seg_scan(key, ps1, px, lane);
      const int nk = lane_next_i(key, -2);
      if (key >= 0 && nk != key) {
        const unsigned n = (unsigned)(px >> 40) & 0x3FFu;
        tab.add(codes[key], n, (unsigned)(px >> 50), (long long)ps1, px & 0xFFFFFFFFFFull);
        if (n) kept[key] = 1;
      }
    }
    km_wave_sync();
    if (c >= 0 && kept[lane]) tab.add_position(c);
    km_wave_sync();                                             // the tile's words are read before the next tile's are stored
  }

  if constexpr (LDS_TABLE) {
    __syncthreads();
    for (int c = threadIdx.x; c < nc; c += kKmThreads) {
      const unsigned n = tab.n[c], cl = tab.cl[c], ps = tab.pos[c];
      if (n) {
        atomicAdd(&a.acc[c], (unsigned long long)n);
        atomicAdd(&a.acc[(size_t)nc + c], tab.s1[c]);
        atomicAdd(&a.acc[2 * (size_t)nc + c], tab.s2[c]);
      }
      if (ps) atomicAdd(&a.acc[3 * (size_t)nc + c], (unsigned long long)ps);
      if (cl) atomicAdd(&a.acc[4 * (size_t)nc + c], (unsigned long long)cl);
    }
  }
}

// correctly rounded (double)v
__device__ __forceinline__ double km_u128_to_double(unsigned __int128 v) {
  const unsigned long long hi = (unsigned long long)(v >> 64);
  if (!hi) return (double)(unsigned long long)v;
  const int sh = 64 - __clzll((long long)hi);
  unsigned long long m = (unsigned long long)(v >> sh);
  if ((v & ((((unsigned __int128)1) << sh) - 1)) != 0) m |= 1ull;     // sticky: far below the rounding position
  return ldexp((double)m, sh);
}

__device__ __forceinline__ void km_write_counts(const nmod_kmer_out& o, int c, long long n, long long pos, long long cl) {
  if (o.n_samples) o.n_samples[c] = n;
  if (o.n_positions) o.n_positions[c] = pos;
  if (o.n_clipped) o.n_clipped[c] = cl;
}

__global__ __launch_bounds__(256) void km_finish_i16_kernel(KmArgs a) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int nc = a.ncodes;
  if (c >= nc) return;
  const unsigned long long n = a.acc[c], s2 = a.acc[2 * (size_t)nc + c];
  const long long s1 = (long long)a.acc[(size_t)nc + c];
  km_write_counts(a.out, c, (long long)n, (long long)a.acc[3 * (size_t)nc + c], (long long)a.acc[4 * (size_t)nc + c]);
  double mean = nan_f64(), sd = nan_f64();
  if (n) {
    const unsigned long long m1 = (unsigned long long)(s1 < 0 ? -s1 : s1);
    const unsigned __int128 v = (unsigned __int128)n * s2 - (unsigned __int128)m1 * m1;   // >= 0 (Cauchy-Schwarz)
    mean = ((double)s1 / (double)n) / 1000.0;
    sd = sqrt(km_u128_to_double(v)) / (double)n / 1000.0;
  }
  if (a.out.mean) a.out.mean[c] = mean;
  if (a.out.sd) a.out.sd[c] = sd;
}

// ------------------------------------------------------------------------------------------------------ float32 / float64

template <int DT>
__device__ __forceinline__ double km_load(const void* p, int64_t i) {
  if constexpr (DT == NMOD_DTYPE_F32) return (double)static_cast<const float*>(p)[i];
  else return static_cast<const double*>(p)[i];
}

template <int DT>
__global__ __launch_bounds__(256) void km_moments_kernel(KmArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const bool clip = a.keep_lo != nullptr;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.npos; p += nwaves) {
    int64_t b, e;
    km_row(a, p, b, e);
    const int64_t n = e - b;
    int c;
    unsigned st = km_classify(a, p, n, c);
    double mean = 0.0, m2 = 0.0;
    unsigned long long nk = 0, ncl = 0;
    if (!st) {
      const double lo = clip ? a.keep_lo[c] : 0.0, hi = clip ? a.keep_hi[c] : 0.0;
      bool bad = false;
      double sum = 0.0;
      for (int64_t k = lane; k < n; k += 64) {
        const double x = km_load<DT>(a.sig, b + k);
        bad |= !(fabs(x) <= kDblMax);
        const bool in = !clip || (lo <= x && x <= hi);
        sum += in ? x : 0.0;
        nk += in ? 1u : 0u;
      }
      nk = wave_sum_u64(nk);
      ncl = (unsigned long long)n - nk;
      if (__ballot(bad) != 0ull) { st = NMOD_STATUS_NONFINITE; c = -1; nk = ncl = 0; }
      else if (nk) {
        const double dn = (double)nk;
        const double m0 = wave_sum_f64(sum) / dn;
        double sd1 = 0.0, sd2 = 0.0;                            // corrected two-pass
        for (int64_t k = lane; k < n; k += 64) {
          const double x = km_load<DT>(a.sig, b + k);
          const bool in = !clip || (lo <= x && x <= hi);
          const double d = x - m0;
          sd1 += in ? d : 0.0;
          sd2 += in ? d * d : 0.0;
        }
        const double r = wave_sum_f64(sd1) / dn;
        mean = m0 + r;
        m2 = wave_sum_f64(sd2) - r * r * dn;
        if (m2 < 0.0) m2 = 0.0;
      }
    }
    if (lane == 0) {
      if (a.pos_status) a.pos_status[p] = (uint8_t)st;
      a.pmean[p] = mean; a.pm2[p] = m2;
      a.pn[p] = (int32_t)nk; a.pcl[p] = (int32_t)ncl;
      a.key[p] = (uint64_t)(c >= 0 ? c : a.ncodes);             // the positions that take no part sort behind every code
      a.val[p] = (uint32_t)p;
    }
  }
}

struct KmMoments { double n, mean, m2; };

// (a) then (b), the pairwise update of Chan, Golub and LeVeque
__device__ __forceinline__ KmMoments km_chan(const KmMoments& x, const KmMoments& y) {
#pragma clang fp contract(off)
  if (y.n == 0.0) return x;
  if (x.n == 0.0) return y;
  KmMoments r;
  r.n = x.n + y.n;
  const double d = y.mean - x.mean;
  r.mean = x.mean + d * (y.n / r.n);
  r.m2 = x.m2 + y.m2 + d * d * (x.n * y.n / r.n);
  return r;
}

__device__ __forceinline__ int64_t km_lower_bound(const uint64_t* keys, int64_t n, uint64_t k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (keys[mid] < k) lo = mid + 1; else hi = mid; }
  return lo;
}

// skey / sval: the positions sorted by code, equal codes in index order
__global__ __launch_bounds__(256) void km_combine_kernel(KmArgs a, const uint64_t* skey, const uint32_t* sval) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < a.ncodes; c += gridDim.x * 4) {
    const int64_t begin = km_lower_bound(skey, a.npos, (uint64_t)c), end = km_lower_bound(skey, a.npos, (uint64_t)c + 1);
    KmMoments m = {0.0, 0.0, 0.0};
    unsigned long long ns = 0, ncl = 0, npo = 0;
    for (int64_t r = begin + lane; r < end; r += 64) {
      const uint32_t p = sval[r];
      const int32_t pn = a.pn[p];
      ns += (unsigned long long)pn; ncl += (unsigned long long)a.pcl[p]; npo += pn > 0 ? 1u : 0u;
      const KmMoments y = {(double)pn, a.pmean[p], a.pm2[p]};
      m = km_chan(m, y);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                          // lanes (l, l + d) -> l: the ranks stay in order
      KmMoments y;
      y.n = __shfl_down(m.n, d); y.mean = __shfl_down(m.mean, d); y.m2 = __shfl_down(m.m2, d);
      m = km_chan(m, y);
    }
    ns = wave_sum_u64(ns); ncl = wave_sum_u64(ncl); npo = wave_sum_u64(npo);
    if (lane == 0) {
      km_write_counts(a.out, c, (long long)ns, (long long)npo, (long long)ncl);
      if (a.out.mean) a.out.mean[c] = ns ? m.mean : nan_f64();
      if (a.out.sd) a.out.sd[c] = ns ? sqrt(m.m2 / m.n) : nan_f64();
    }
  }
}

template <bool LDS_TABLE>
static void km_launch_i16(const KmArgs& a, int num_cus, hipStream_t stream) {
  const int64_t ntiles = (a.npos + kKmTile - 1) / kKmTile;
  const dim3 grid(persistent_grid(ntiles, kKmWaves, (int64_t)num_cus * (LDS_TABLE ? 1 : 2)));
  const size_t lds = LDS_TABLE ? (size_t)a.ncodes * kKmLdsBytesPerCode : 0;
  // (above 64 KiB of dynamic LDS some runtimes want to be told; where there is no such limit the call is a no-op or an error to drop)
  const void* fn = a.kbound ? (const void*)km_i16_kernel<LDS_TABLE, true> : (const void*)km_i16_kernel<LDS_TABLE, false>;
  if (lds > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) (void)hipGetLastError();
  if (a.kbound) hipLaunchKernelGGL((km_i16_kernel<LDS_TABLE, true>), grid, dim3(kKmThreads), lds, stream, a);
  else hipLaunchKernelGGL((km_i16_kernel<LDS_TABLE, false>), grid, dim3(kKmThreads), lds, stream, a);
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_kmer_model(const nmod_params* prm, int64_t npos, const void* sig, const int64_t* off, const int32_t* code,
                               int32_t ncodes, const double* keep_lo, const double* keep_hi, const nmod_kmer_out* out) {
  if (check_prm_common(prm) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > (int64_t)INT32_MAX - 1 || ncodes < 1 || ncodes > NMOD_MAX_KMER_CODES) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_kmer_out)) return NMOD_ERR_INVALID_ARG;
  if ((keep_lo == nullptr) != (keep_hi == nullptr)) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && (!sig || !code)) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && !off && prm->stride0 <= 0) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && npos > 0) {
    if (off && !csr_offsets_ok(off, npos)) return NMOD_ERR_INVALID_ARG;
    for (int64_t i = 0; i < npos; ++i) if (code[i] < -1 || code[i] >= ncodes) return NMOD_ERR_INVALID_ARG;
  }
  const size_t nc = (size_t)ncodes, np = (size_t)npos;
  if (npos == 0 && host) {                                        // nothing to reduce: no device is needed
    for (size_t c = 0; c < nc; ++c) {
      if (out->n_positions) out->n_positions[c] = 0;
      if (out->n_samples) out->n_samples[c] = 0;
      if (out->n_clipped) out->n_clipped[c] = 0;
      if (out->mean) out->mean[c] = NAN;
      if (out->sd) out->sd[c] = NAN;
    }
    return NMOD_OK;
  }
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const bool i16 = prm->dtype == NMOD_DTYPE_I16_MILLI, clip = keep_lo != nullptr;
  const size_t esz = elem_bytes(prm->dtype);
  const size_t tot = host ? (size_t)(off ? off[npos] : npos * prm->stride0) : 0;

  KmArgs a;
  memset(&a, 0, sizeof(a));
  a.sig = sig; a.off = off; a.stride = off ? 0 : prm->stride0; a.code = code;
  a.npos = npos; a.ncodes = ncodes;
  a.keep_lo = keep_lo; a.keep_hi = keep_hi;
  a.out = *out;

  // one slab: the table (int16) or the per-position moments and the sort's buffers (floats); for the host entry the inputs
  // (the samples with 16 spare bytes: km_i16_kernel reads whole aligned pieces) and outputs as well
  Slab slab(host);
  const size_t o_acc = slab.take(i16 ? nc * 8 * 5 : 0), o_kb = slab.take(i16 && clip ? nc * 8 : 0);
  const size_t o_pm = slab.take(i16 ? 0 : np * 16), o_pn = slab.take(i16 ? 0 : np * 8);
  const size_t o_key = slab.take(i16 ? 0 : np * 16), o_val = slab.take(i16 ? 0 : np * 8), o_rs = slab.take(i16 ? 0 : rs_scratch_bytes(npos));
  slab.in(a.sig, tot * esz, 16); slab.in(a.off, (np + 1) * 8); slab.in(a.code, np * 4);
  slab.in(a.keep_lo, nc * 8); slab.in(a.keep_hi, nc * 8);
  slab.out(a.out.n_positions, nc * 8); slab.out(a.out.n_samples, nc * 8); slab.out(a.out.n_clipped, nc * 8);
  slab.out(a.out.mean, nc * 8); slab.out(a.out.sd, nc * 8); slab.out(a.out.pos_status, np);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.pos_status = a.out.pos_status;
  const unsigned code_blocks = (unsigned)((nc + 255) / 256);
  if (i16) {
    a.acc = slab.at<unsigned long long>(o_acc);
    NMOD_HIP(hipMemsetAsync(a.acc, 0, nc * 8 * 5, stream));
    if (clip) {
      hipLaunchKernelGGL(km_bounds_kernel, dim3(code_blocks), dim3(256), 0, stream, a.keep_lo, a.keep_hi, ncodes, slab.at<int2>(o_kb));
      a.kbound = slab.at<int2>(o_kb);
    }
    if (npos > 0) {
      if (ncodes <= kKmLdsCodes) km_launch_i16<true>(a, num_cus, stream); else km_launch_i16<false>(a, num_cus, stream);
    }
    hipLaunchKernelGGL(km_finish_i16_kernel, dim3(code_blocks), dim3(256), 0, stream, a);
  } else {
    a.pmean = slab.at<double>(o_pm); a.pm2 = a.pmean + np;
    a.pn = slab.at<int32_t>(o_pn); a.pcl = a.pn + np;
    a.key = slab.at<uint64_t>(o_key); a.val = slab.at<uint32_t>(o_val);
    uint64_t* key_tmp = a.key + np; uint32_t* val_tmp = a.val + np;
    const int passes = ncodes < 256 ? 1 : (ncodes < 65536 ? 2 : 3);         // the largest key is ncodes
    if (npos > 0) {
      const int64_t mb = (npos + 3) / 4, mcap = (int64_t)num_cus * 8;
      const dim3 mgrid((unsigned)(mb < mcap ? mb : mcap));
      if (prm->dtype == NMOD_DTYPE_F32) hipLaunchKernelGGL(km_moments_kernel<NMOD_DTYPE_F32>, mgrid, dim3(256), 0, stream, a);
      else hipLaunchKernelGGL(km_moments_kernel<NMOD_DTYPE_F64>, mgrid, dim3(256), 0, stream, a);
      NMOD_HIP(rs_sort_pairs(a.key, a.val, key_tmp, val_tmp, npos, slab.at<char>(o_rs), stream, passes));
    }
    const bool in_tmp = (passes & 1) != 0;
    const int64_t cb = ((int64_t)ncodes + 3) / 4, ccap = (int64_t)num_cus * 8;
    hipLaunchKernelGGL(km_combine_kernel, dim3((unsigned)(cb < ccap ? cb : ccap)), dim3(256), 0, stream, a,
                       (const uint64_t*)(in_tmp ? key_tmp : a.key), (const uint32_t*)(in_tmp ? val_tmp : a.val));
  }
  return launches_end(slab, stream);
}
