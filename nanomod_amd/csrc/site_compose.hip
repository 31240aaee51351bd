// nmod_site_compose — the shares of all states at a site by maximum likelihood (EM on the simplex) from the pivoted window sums of
// nmod_read_llr_multi, with a likelihood-ratio test per state and the responsibilities per read, on the device (K26).  The
// reference project has no such step; the definition is the one in include/nanomod_hip.h (tests/compose_ref.py restates it in numpy).
// K14's shape on pos_walk.hpp's walk, all on the caller's stream:
//   pos_classify_kernel<CoRule>  a thread per row: the row's class by its length
//   co_reg_kernel<NALT, 16>  rows <= NMOD_STOICH_SMALL: 16 lanes x 16 reads, four rows per wave; a finished row freezes while the others of
//                            its wave go on
//   co_reg_kernel<NALT, 64>  rows <= NMOD_STOICH_WAVE: the whole wave x 16 reads
//   co_block_kernel<NALT>    beyond: a workgroup of 256 threads per row (a row beyond NMOD_MAX_DEEP gets its NaN outputs here)
// Where the weights of a row live is decided by the row's length n and n_alt alone:
//   n <= NMOD_STOICH_WAVE                  registers: n_alt + 1 doubles per read, 16 reads per lane (32 .. 80 doubles a lane)
//   n <= kCoStageWords / (n_alt + 1)       LDS: 60 KiB of the workgroup, planes of n_alt + 1 x that many reads (3 840, 2 560, 1 920, 1 536 reads
//                                          for n_alt = 1 .. 4); two such workgroups fit the 160 KiB of a CU
//   beyond                                 a pool slab of n_alt + 1 planes in the score layout, streamed once per iteration (each thread reads
//                                          back the words it wrote itself: no barrier, no fence)
// The weights are computed once per valid read (n_alt + 1 exp); an iteration is one reciprocal and 2 (n_alt + 1) multiplications per read
// and no exp; the final evaluation reads the scores again for mx_i and takes one log per read.  A per-state test is one more fit per open
// state over the same resident weights.  Sums: a fixed-order chain per lane (the lane's reads in ascending index), then the fixed-order
// lane, wave and LDS reductions of wave_ops.hpp / entry_device.hpp; no float atomics; a row's bits depend on the row alone.
// p_m is the 1/2 chi2_0 + 1/2 chi2_1 boundary law of the likelihood-ratio test of pi_m = 0: asymptotic, and right only when the remaining
// shares are interior (a second share on the boundary makes the law a different mixture); tests/test_site_compose.py simulates the null:
// rows of 20 reads rejected 4.1 %, rows of 200 reads 4.2 % at the 5 % level (profiles/site_compose.txt): conservative, as K14's.
// Throughput (profiles/site_compose.txt §3, MI355X, the per-state test on): 37 M, 6.7 M and 1.7 M rows / s for rows of 40, 600 and 2 000 reads
// at n_alt = 2; 3.5 M, 2.2 M and 0.28 M at n_alt = 4.  Not tuned: the register forms run at one or two waves per SIMD.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "pos_walk.hpp"
#include "special_math.hpp"

namespace nmod {

constexpr int kCoPer = 16;                        // reads a lane keeps
constexpr int kCoThreads = 256;
constexpr int kCoWaves = kCoThreads / 64;
constexpr int kCoStageWords = 7680;               // doubles of weights the workgroup form keeps in LDS (60 KiB)
static_assert(16 * kCoPer == NMOD_STOICH_SMALL && 64 * kCoPer == NMOD_STOICH_WAVE, "K14's class steps");

__host__ __device__ constexpr int64_t co_stage_reads(int nalt) { return kCoStageWords / (nalt + 1); }

struct CoArgs {
  const double* score[NMOD_MULTI_MAX]; const int64_t* off; int64_t stride, npos, total;
  int n_alt, max_iter, min_valid; double tol;
  nmod_compose_out out;
  double* wsc;                                    // n_alt + 1 planes of `total`: the weights of the rows beyond the LDS stage (or null: no such row)
  PosLists<3> pl;
};

__device__ __forceinline__ bool co_valid(double s) { return fabs(s) <= kDblMax; }

struct CoRule {
  static constexpr int NC = 3;
  using Track = void;
  static __device__ __forceinline__ int cls(const CoArgs& a, int64_t i, int64_t& yb, int64_t& yn) {
    csr_row(a.off, a.stride, i, yb, yn);
    return yn <= NMOD_STOICH_SMALL ? 0 : (yn <= NMOD_STOICH_WAVE ? 1 : 2);      // (a row beyond NMOD_MAX_DEEP: the workgroup form refuses it)
  }
};

template <int NALT>
struct CoFit { double pi[NALT + 1]; double ll; int iters; bool nc, degen; };

// the weights of one read from its scores: mx = the largest of 0 and the open scores, w_0 = exp(-mx), w_m = exp(s_m - mx), 0 for a closed m
template <int NALT>
__device__ __forceinline__ void co_weights(const double (&s)[NALT], unsigned om, double (&w)[NALT + 1]) {
  double mx = 0.0;
#pragma unroll
  for (int m = 0; m < NALT; ++m) if ((om >> m & 1u) && s[m] > mx) mx = s[m];
  w[0] = exp(-mx);
#pragma unroll
  for (int m = 0; m < NALT; ++m) w[m + 1] = (om >> m & 1u) ? exp(s[m] - mx) : 0.0;
}

// den and the terms pi_m w_m of one read, in ascending m
template <int NALT>
__device__ __forceinline__ double co_den(const double (&pi)[NALT + 1], const double (&w)[NALT + 1], double (&t)[NALT + 1]) {
  t[0] = pi[0] * w[0];
  double den = t[0];
#pragma unroll
  for (int m = 1; m <= NALT; ++m) { t[m] = pi[m] * w[m]; den += t[m]; }
  return den;
}

// A row in the registers of a group of G lanes: lane g of it keeps the reads g + G j, j < 16; vm: which of them are valid
template <int NALT, int G>
struct CoRegRow {
  double w[kCoPer][NALT + 1];
  unsigned vm;
  const CoArgs* a; int64_t yb; int gl, lane;
  template <class F> __device__ __forceinline__ void each(F&& f) const {
#pragma unroll
    for (int j = 0; j < kCoPer; ++j) if (vm >> j & 1u) f(w[j], (int64_t)(gl + G * j));
  }
  __device__ __forceinline__ double sum(double v) const { return group_sum_f64<G>(v); }
  __device__ __forceinline__ bool any(bool b) const { return group_any<G>(b, lane); }
  __device__ __forceinline__ bool all_done(bool done) const { return __ballot(!done) == 0ull; }
};

// A row of the workgroup: thread t keeps the reads t + 256 j in planes of `ws` words at wp (LDS or the pool slab); w_0 = -1 marks a read that
// is not valid
template <int NALT>
struct CoBlockRow {
  const double* wp; int64_t ws, n; double* sh;
  const CoArgs* a; int64_t yb;
  template <class F> __device__ __forceinline__ void each(F&& f) const {
    for (int64_t i = threadIdx.x; i < n; i += kCoThreads) {
      double w[NALT + 1];
      w[0] = wp[i];
      if (w[0] >= 0.0) {
#pragma unroll
        for (int m = 1; m <= NALT; ++m) w[m] = wp[m * ws + i];
        f(w, i);
      }
    }
  }
  __device__ __forceinline__ double sum(double v) const { return block_sum_f64<kCoWaves>(v, sh); }
  __device__ __forceinline__ bool any(bool b) const { return __syncthreads_or(b ? 1 : 0) != 0; }
  __device__ __forceinline__ bool all_done(bool done) const { return done; }       // (the same in every thread: the sums are)
};

// mx of read idx of a row, from its scores again (no exp)
template <int NALT>
__device__ __forceinline__ double co_mx(const CoArgs& a, int64_t at, unsigned om) {
  double mx = 0.0;
#pragma unroll
  for (int m = 0; m < NALT; ++m)
    if (om >> m & 1u) { const double s = a.score[m][at]; if (s > mx) mx = s; }
  return mx;
}

// EM over the states of `active` (bit 0: canonical, always on; bit m: state m) from the uniform start, then the evaluation of ll at the
// result; om: the open states (bit m - 1), which fixed the weights.  Reached by whole waves / the whole workgroup; run false: computes along
template <int NALT, class Row>
__device__ __forceinline__ void co_fit(const Row& row, bool run, unsigned active, unsigned om, double nv, int max_iter, double tol, CoFit<NALT>& f) {
  const double share = 1.0 / (double)__popc(active);
#pragma unroll
  for (int m = 0; m <= NALT; ++m) f.pi[m] = (active >> m & 1u) ? share : 0.0;
  f.iters = 0; f.degen = false;
  bool done = !run;
  for (int it = 0; it < max_iter; ++it) {
    if (row.all_done(done)) break;
    double R[NALT + 1];
#pragma unroll
    for (int m = 0; m <= NALT; ++m) R[m] = 0.0;
    bool bad = false;
    row.each([&](const double (&w)[NALT + 1], int64_t) {
      double t[NALT + 1];
      const double den = co_den<NALT>(f.pi, w, t);
      if (den > 0.0) {
        const double q = 1.0 / den;
#pragma unroll
        for (int m = 0; m <= NALT; ++m) R[m] += t[m] * q;
      } else {
        bad = true;
      }
    });
#pragma unroll
    for (int m = 0; m <= NALT; ++m) R[m] = row.sum(R[m]);
    bad = row.any(bad);
    if (!done) {
      if (bad) {
        f.degen = true; done = true;
      } else {
        double step = 0.0;
#pragma unroll
        for (int m = 0; m <= NALT; ++m) {
          const double p = R[m] / nv;
          step = fmax(step, fabs(p - f.pi[m]));
          f.pi[m] = p;
        }
        ++f.iters;
        if (tol > 0.0 && step <= tol) done = true;
      }
    }
  }
  f.nc = run && !done;
  double l = 0.0;
  bool bad = false;
  row.each([&](const double (&w)[NALT + 1], int64_t idx) {
    double t[NALT + 1];
    const double den = co_den<NALT>(f.pi, w, t);
    if (den > 0.0) l += log(den) + co_mx<NALT>(*row.a, row.yb + idx, om); else bad = true;
  });
  f.ll = row.sum(l);
  if (row.any(bad)) f.degen = true;
}

template <int NALT>
__device__ __forceinline__ void co_write_nan(const CoArgs& a, int64_t pos, int n_valid, int n_partial, unsigned om, unsigned status) {
  const nmod_compose_out& o = a.out;
  const double nan = nan_f64();
#pragma unroll
  for (int m = 0; m <= NALT; ++m) if (o.pi) o.pi[m * a.npos + pos] = nan;
#pragma unroll
  for (int m = 0; m < NALT; ++m) {
    if (o.stat_m) o.stat_m[m * a.npos + pos] = nan;
    if (o.p_m) o.p_m[m * a.npos + pos] = nan;
  }
  if (o.ll) o.ll[pos] = nan;
  if (o.stat) o.stat[pos] = nan;
  if (o.n_valid) o.n_valid[pos] = n_valid;
  if (o.n_partial) o.n_partial[pos] = n_partial;
  if (o.iters) o.iters[pos] = 0;
  if (o.open_mask) o.open_mask[pos] = (uint8_t)om;
  if (o.status) o.status[pos] = (uint8_t)status;
}

// Everything between a row's counts and its outputs; `lead`: the thread that writes them.  Returns whether the row has an estimate, the
// fit with it
template <int NALT, class Row>
__device__ __forceinline__ bool co_estimate(const CoArgs& a, const Row& row, bool have, bool lead, int64_t pos, unsigned om, double cv, double cp,
                                            CoFit<NALT>& f) {
  const int nv = (int)cv, np = (int)cp;
  const bool no_state = om == 0u, too_few = !no_state && nv < a.min_valid;
  const bool run = have && !no_state && !too_few;
  const unsigned all = 1u | (om << 1);
  co_fit<NALT>(row, run, all, om, cv, a.max_iter, a.tol, f);
  const bool est = run && !f.degen;
  const nmod_compose_out& o = a.out;
  unsigned status = f.nc ? NMOD_COMPOSE_NOT_CONVERGED : 0u;
  if (have && lead) {
    if (!est) {
      co_write_nan<NALT>(a, pos, nv, np, om, no_state ? NMOD_COMPOSE_NO_STATE : (too_few ? NMOD_COMPOSE_TOO_FEW : NMOD_COMPOSE_DEGENERATE));
    } else {
#pragma unroll
      for (int m = 0; m <= NALT; ++m) if (o.pi) o.pi[m * a.npos + pos] = f.pi[m];
      if (o.ll) o.ll[pos] = f.ll;
      if (o.stat) o.stat[pos] = 2.0 * fmax(f.ll, 0.0);
      if (o.n_valid) o.n_valid[pos] = nv;
      if (o.n_partial) o.n_partial[pos] = np;
      if (o.iters) o.iters[pos] = f.iters;
      if (o.open_mask) o.open_mask[pos] = (uint8_t)om;
    }
  }
  if (o.stat_m || o.p_m) {                                     // the per-state tests: one more fit per open state, the state closed
#pragma unroll 1
    for (int m = 1; m <= NALT; ++m) {
      const bool open = (om >> (m - 1) & 1u) != 0u;
      CoFit<NALT> g;
      co_fit<NALT>(row, est && open, all & ~(1u << m), om, cv, a.max_iter, a.tol, g);
      if (est) {
        double sm = nan_f64(), pm = nan_f64();
        if (open) {
          if (g.nc) status |= NMOD_COMPOSE_NOT_CONVERGED;
          if (g.degen) {
            status |= NMOD_COMPOSE_DEGENERATE;
          } else {
            sm = 2.0 * fmax(f.ll - g.ll, 0.0);
            pm = sm == 0.0 ? 1.0 : fmax(0.5 * erfc(sqrt(sm / 2.0)), kDblMin);
          }
        }
        if (have && lead) {
          if (o.stat_m) o.stat_m[(m - 1) * a.npos + pos] = sm;
          if (o.p_m) o.p_m[(m - 1) * a.npos + pos] = pm;
        }
      }
    }
  }
  if (have && lead && est && o.status) o.status[pos] = (uint8_t)status;
  return est;
}

// the responsibilities of one valid read at the fit, or NaN
template <int NALT>
__device__ __forceinline__ void co_resp(const CoArgs& a, int64_t at, bool use, const CoFit<NALT>& f, const double (&w)[NALT + 1]) {
  double t[NALT + 1];
  double q = nan_f64();
  if (use) q = 1.0 / co_den<NALT>(f.pi, w, t);
#pragma unroll
  for (int m = 0; m <= NALT; ++m) a.out.resp[m * a.total + at] = use ? t[m] * q : q;
}

template <int NALT, int G>
__global__ __launch_bounds__(kCoThreads) void co_reg_kernel(CoArgs a) {
  const int lane = threadIdx.x & 63, gl = threadIdx.x & (G - 1);
  for (GroupWalk<G == 16 ? 0 : 1, G, kCoThreads> it(a.pl); it.more(); it.next()) {
    const bool have = it.have();
    int64_t pos = 0, yb = 0, yn = 0;
    if (have) {
      pos = it.pos();
      csr_row(a.off, a.stride, pos, yb, yn);
    }
    const int ny = (int)yn;
    CoRegRow<NALT, G> row;
    row.a = &a; row.yb = yb; row.gl = gl; row.lane = lane;
    unsigned long long fin = 0ull;                             // four bits per read: which of its scores are finite
    unsigned o = 0u;
#pragma unroll
    for (int j = 0; j < kCoPer; ++j) {
      const int idx = gl + G * j;
#pragma unroll
      for (int m = 0; m < NALT; ++m) {
        const double s = idx < ny ? a.score[m][yb + idx] : nan_f64();
        row.w[j][m + 1] = s;
        if (co_valid(s)) { fin |= 1ull << (4 * j + m); o |= 1u << m; }
      }
    }
    unsigned om = 0u;                                          // the open states, bit m - 1
#pragma unroll
    for (int m = 0; m < NALT; ++m) if (group_any<G>((o >> m & 1u) != 0u, lane)) om |= 1u << m;
    double cv = 0.0, cp = 0.0;
    row.vm = 0u;
#pragma unroll
    for (int j = 0; j < kCoPer; ++j) {
      const unsigned f = (unsigned)(fin >> (4 * j)) & 15u;
      const bool valid = om != 0u && f == om;
      double s[NALT];
#pragma unroll
      for (int m = 0; m < NALT; ++m) s[m] = row.w[j][m + 1];
      if (valid) {
        co_weights<NALT>(s, om, row.w[j]);
        row.vm |= 1u << j;
      } else {
#pragma unroll
        for (int m = 0; m <= NALT; ++m) row.w[j][m] = 0.0;
      }
      cv += valid ? 1.0 : 0.0;
      cp += f != 0u && !valid ? 1.0 : 0.0;
    }
    cv = group_sum_f64<G>(cv);                                 // (counts of up to 1 024 ones: exact)
    cp = group_sum_f64<G>(cp);
    CoFit<NALT> f;
    const bool est = co_estimate<NALT>(a, row, have, gl == 0, pos, om, cv, cp, f);
    if (a.out.resp && have) {
#pragma unroll
      for (int j = 0; j < kCoPer; ++j) {
        const int idx = gl + G * j;
        if (idx < ny) co_resp<NALT>(a, yb + idx, est && (row.vm >> j & 1u), f, row.w[j]);
      }
    }
  }
}

template <int NALT>
__global__ __launch_bounds__(kCoThreads) void co_block_kernel(CoArgs a) {
  __shared__ double stage[kCoStageWords];
  __shared__ double sh[kCoWaves];
  const int tid = threadIdx.x;
  constexpr int64_t cap = co_stage_reads(NALT);
  for (BlockWalk<2> it(a.pl); it.more(); it.next()) {
    const int64_t pos = it.pos();
    int64_t yb, yn;
    csr_row(a.off, a.stride, pos, yb, yn);
    const bool staged = yn <= cap;
    if (yn > NMOD_MAX_DEEP || (!staged && !a.wsc)) {           // (no slab: the caller's total_scores did not cover this row; refused likewise)
      if (tid == 0) co_write_nan<NALT>(a, pos, 0, 0, 0u, NMOD_COMPOSE_TOO_LARGE);
      if (a.out.resp)
        for (int64_t i = tid; i < yn; i += kCoThreads) {
#pragma unroll
          for (int m = 0; m <= NALT; ++m) a.out.resp[m * a.total + yb + i] = nan_f64();
        }
      continue;
    }
    unsigned o = 0u;
    for (int64_t i = tid; i < yn; i += kCoThreads) {
#pragma unroll
      for (int m = 0; m < NALT; ++m) if (co_valid(a.score[m][yb + i])) o |= 1u << m;
    }
    unsigned om = 0u;
#pragma unroll
    for (int m = 0; m < NALT; ++m) if (__syncthreads_or((int)(o >> m & 1u))) om |= 1u << m;
    double* wp = staged ? stage : a.wsc + yb;
    const int64_t ws = staged ? cap : a.total;
    double cv = 0.0, cp = 0.0;
    for (int64_t i = tid; i < yn; i += kCoThreads) {           // the weights: read back by this thread alone
      double s[NALT], w[NALT + 1];
      unsigned f = 0u;
#pragma unroll
      for (int m = 0; m < NALT; ++m) { s[m] = a.score[m][yb + i]; if (co_valid(s[m])) f |= 1u << m; }
      const bool valid = om != 0u && f == om;
      if (valid) {
        co_weights<NALT>(s, om, w);
#pragma unroll
        for (int m = 0; m <= NALT; ++m) wp[m * ws + i] = w[m];
      } else {
        wp[i] = -1.0;
      }
      cv += valid ? 1.0 : 0.0;
      cp += f != 0u && !valid ? 1.0 : 0.0;
    }
    cv = block_sum_f64<kCoWaves>(cv, sh);                      // (counts of up to 2^24 ones: exact)
    cp = block_sum_f64<kCoWaves>(cp, sh);
    CoBlockRow<NALT> row;
    row.wp = wp; row.ws = ws; row.n = yn; row.sh = sh; row.a = &a; row.yb = yb;
    CoFit<NALT> f;
    const bool est = co_estimate<NALT>(a, row, true, tid == 0, pos, om, cv, cp, f);
    if (a.out.resp)
      for (int64_t i = tid; i < yn; i += kCoThreads) {
        double w[NALT + 1];
        w[0] = wp[i];
        const bool use = est && w[0] >= 0.0;
#pragma unroll
        for (int m = 1; m <= NALT; ++m) w[m] = use ? wp[m * ws + i] : 0.0;
        co_resp<NALT>(a, yb + i, use, f, w);
      }
  }
}

template <int NALT>
static void co_launch(const CoArgs& a, int num_cus, hipStream_t stream) {
  launch_groups<16, kCoThreads>(co_reg_kernel<NALT, 16>, a, num_cus, stream);
  launch_groups<64, kCoThreads>(co_reg_kernel<NALT, 64>, a, num_cus, stream);
  launch_blocks<kCoThreads>(co_block_kernel<NALT>, a, num_cus, stream);
}

}  // namespace nmod

using namespace nmod;

extern "C" int64_t nmod_site_compose_stage_reads(int32_t n_alt) {
  return n_alt >= 1 && n_alt <= NMOD_MULTI_MAX ? co_stage_reads(n_alt) : -1;
}

extern "C" int nmod_site_compose(const nmod_params* prm, int64_t npos, int64_t total_scores, int32_t n_alt, const double* const* score,
                                 const int64_t* off, const nmod_compose_opts* opts, const nmod_compose_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_compose_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_compose_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->max_iter < 1 || opts->max_iter > NMOD_COMPOSE_MAX_ITER || opts->min_valid < 1) return NMOD_ERR_INVALID_ARG;
  if (!(opts->tol >= 0.0) || !(opts->tol <= kDblMax)) return NMOD_ERR_INVALID_ARG;
  if (n_alt < 1 || n_alt > NMOD_MULTI_MAX || !score) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > (int64_t)INT32_MAX - 1 || total_scores < 0) return NMOD_ERR_INVALID_ARG;
  if (!off && prm->stride0 <= 0) return NMOD_ERR_INVALID_ARG;
  for (int m = 0; m < n_alt; ++m) if (npos > 0 && !score[m]) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (!off && npos > 0 && total_scores / prm->stride0 < npos) return NMOD_ERR_INVALID_ARG;
  if (host && off && npos > 0 && (!csr_offsets_ok(off, npos) || off[npos] > total_scores)) return NMOD_ERR_INVALID_ARG;
  int num_cus = 0;
  const int rc = rows_begin(prm, npos, off, &num_cus);
  if (rc != NMOD_OK || npos == 0) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t np = (size_t)npos, na = (size_t)n_alt;
  const size_t tot = !host ? 0 : (off ? (size_t)off[npos] : np * (size_t)prm->stride0);   // scores the host call copies in
  const size_t plane = host ? (size_t)total_scores : 0;

  CoArgs a;
  memset(&a, 0, sizeof(a));
  for (int m = 0; m < n_alt; ++m) a.score[m] = score[m];
  a.off = off; a.stride = off ? 0 : prm->stride0; a.npos = npos; a.total = total_scores;
  a.n_alt = n_alt; a.max_iter = opts->max_iter; a.min_valid = opts->min_valid; a.tol = opts->tol;
  a.out = *out;

  // whether a row can lie beyond the LDS stage of the workgroup form: known from the offsets of a host call or the stride, else from
  // total_scores, which bounds every row
  const int64_t cap = co_stage_reads(n_alt);
  bool streamed = off ? total_scores > cap : prm->stride0 > cap;
  if (host && off) {
    streamed = false;
    for (int64_t i = 0; i < npos && !streamed; ++i) streamed = off[i + 1] - off[i] > cap;
  }

  // one slab: the three work lists and their count words, the streamed weights; for the host entry the inputs and outputs as well
  Slab slab(host);
  const PosListSpace<3> lists(slab, np);
  const size_t o_wsc = streamed ? slab.take((na + 1) * (size_t)total_scores * 8) : 0;
  slab.in(a.off, (np + 1) * 8);
  for (int m = 0; m < n_alt; ++m) slab.in(a.score[m], tot * 8);
  slab.out(a.out.pi, (na + 1) * np * 8); slab.out(a.out.ll, np * 8); slab.out(a.out.stat, np * 8);
  slab.out(a.out.stat_m, na * np * 8); slab.out(a.out.p_m, na * np * 8);
  slab.out(a.out.n_valid, np * 4); slab.out(a.out.n_partial, np * 4); slab.out(a.out.iters, np * 4);
  slab.out(a.out.open_mask, np); slab.out(a.out.status, np);
  slab.out(a.out.resp, (na + 1) * plane * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  if (streamed) a.wsc = slab.at<double>(o_wsc);
  NMOD_HIP(lists.fill<CoRule>(slab, a, num_cus, stream));
  switch (n_alt) {
    case 1: co_launch<1>(a, num_cus, stream); break;
    case 2: co_launch<2>(a, num_cus, stream); break;
    case 3: co_launch<3>(a, num_cus, stream); break;
    default: co_launch<4>(a, num_cus, stream); break;
  }
  return launches_end(slab, stream);
}
