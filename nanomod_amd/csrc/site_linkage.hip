// nmod_pair_linkage — soft same-read linkage of pairs of sites from window sums: per pair the two marginal modified shares by K14's
// maximum likelihood, the linkage D of the joint law of the two hidden states fitted with the margins fixed, its likelihood interval,
// the correlation r and the likelihood-ratio test of independence, on the device (K18).  The reference project has no
// such step; the definition is the one in include/nanomod_hip.h (tests/linkage_ref.py restates it).  The rows come from
// nmod_pair_rows_count / nmod_pair_rows_fill (site_pairs.hip): per pair the two scores of every read that is valid at both sites.
// K14's shape (site_stoich.hip) with two resident rows per pair; all on the caller's stream, one launch per class:
//   pos_classify_kernel<LkRule>  (pos_walk.hpp) a thread per pair: its class by the length of its row; a row beyond NMOD_MAX_DEEP gets
//                        its NaN outputs and status here
//   lk_reg_kernel<16>    rows <= 256: 16 lanes x (16 + 16) signed t values hold the two margins' rows in registers, four pairs per
//                        wave, DPP row sums only; then 16 products v take their place for the linkage and its interval
//   lk_reg_kernel<64>    rows <= 1 024: the whole wave
//   lk_block_kernel      beyond: a workgroup per pair, both rows' signed t staged in LDS while 2 n <= kLkStage, v in their place
//                        while n <= kLkStage (a thread reads back only the words it wrote itself), recomputed from the scores beyond
// Three passes over a row in one launch: both margins (K14's evaluation and bracketed iteration of stoich_rows.hpp on each row, the
// same operations in the same order: pa and pb have nmod_site_stoich's bits), then v = u_a u_b per read, then D and the interval by
// the same iteration over v.  Every sum is a fixed-order chain per lane followed by a fixed-order lane / wave / LDS reduction, no
// float atomics: a pair's bits depend on its row alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "pos_walk.hpp"
#include "special_math.hpp"
#include "stoich_rows.hpp"

namespace nmod {

constexpr int kLkSmall = 16 * kStPer;             // largest row of the 16-lane form: K14's classes, so that a margin has K14's bits
constexpr int kLkWave = 64 * kStPer;              // largest row of the whole-wave form
static_assert(kLkSmall == NMOD_LINK_SMALL && kLkWave == NMOD_LINK_WAVE, "the class steps the header names");
static_assert(NMOD_LINK_SMALL == NMOD_STOICH_SMALL && NMOD_LINK_WAVE == NMOD_STOICH_WAVE, "a margin is reduced in K14's order");
constexpr int kLkThreads = 256;
constexpr int kLkStage = 6144;                    // doubles of a row the workgroup form keeps in LDS (K14's 48 KiB)

struct LkArgs {
  const double* sa; const double* sb; const int64_t* off; int64_t npos;   // npos: the pairs (pos_walk.hpp's name for the rows)
  int max_iter, min_reads; double tol, drop;
  nmod_link_out out;
  PosLists<3> pl;
};

__device__ __forceinline__ void lk_write_nan(const nmod_link_out& o, int64_t i, int n_valid, unsigned status) {
  const double nan = nan_f64();
  if (o.pa) o.pa[i] = nan;
  if (o.pb) o.pb[i] = nan;
  if (o.d) o.d[i] = nan;
  if (o.d_lo) o.d_lo[i] = nan;
  if (o.d_hi) o.d_hi[i] = nan;
  if (o.r) o.r[i] = nan;
  if (o.stat) o.stat[i] = nan;
  if (o.p_indep) o.p_indep[i] = nan;
  if (o.n_valid) o.n_valid[i] = n_valid;
  if (o.iters) o.iters[i] = 0;
  if (o.status) o.status[i] = (uint8_t)status;
}

struct LkRule {
  static constexpr int NC = 3;
  using Track = void;
  static __device__ __forceinline__ int cls(const LkArgs& a, int64_t i, int64_t& yb, int64_t& yn) {
    csr_row(a.off, 0, i, yb, yn);
    if (yn > NMOD_MAX_DEEP) { lk_write_nan(a.out, i, 0, NMOD_LINK_TOO_LARGE); return -1; }
    return yn <= kLkSmall ? 0 : (yn <= kLkWave ? 1 : 2);
  }
};

// the signed t of one side of a read; a read that is not valid at both sites takes no part in either row
__device__ __forceinline__ double lk_signed_t(double s, double other) { return st_valid(other) ? st_signed_t(s) : 0.0; }

// K14's u of one score at the share p, with the sign of the side: + t / (1 - (1 - p) t), - t / (1 - p t)
__device__ __forceinline__ double lk_u(double w, double p) {
  const double t = fabs(w);
  const bool plus = w >= 0.0;
  const double qt = (plus ? 1.0 - p : p) * t;
  const double u = t / (1.0 - qt);
  return plus ? u : -u;
}

// one read's terms of an evaluation at D: x gathers log1p(dv) when WANT_G, else w^2
template <bool WANT_G>
__device__ __forceinline__ void lk_term(double v, double D, double& s, double& x) {
  const double dv = fmax(D * v, -1.0);
  const double w = v / (1.0 + dv);
  s += w;
  if constexpr (WANT_G) x += log1p(dv); else x += w * w;
}

// The products v of a row in the registers of a group of G lanes, in StRegRow's layout
template <int G>
struct LkRegV {
  double v[kStPer];
  static __device__ __forceinline__ bool any(bool f) { return __any(f); }
  template <bool WANT_G>
  __device__ __forceinline__ void eval(double D, double& S, double& X) const {
    double s = 0.0, x = 0.0;
#pragma unroll
    for (int j = 0; j < kStPer; ++j) lk_term<WANT_G>(v[j], D, s, x);
    S = group_sum_f64<G>(s);
    X = group_sum_f64<G>(x);
  }
};

// A pair in the registers of a group: the two margins' rows, then their products
template <int G>
struct LkRegPair {
  StRegRow<G> ra, rb;
  LkRegV<G> rv;
  __device__ __forceinline__ const StRegRow<G>& row_a() const { return ra; }
  __device__ __forceinline__ const StRegRow<G>& row_b() const { return rb; }
  __device__ __forceinline__ const LkRegV<G>& row_v() const { return rv; }
  __device__ __forceinline__ void make_v(double pa, double pb) {
#pragma unroll
    for (int j = 0; j < kStPer; ++j) rv.v[j] = lk_u(ra.w[j], pa) * lk_u(rb.w[j], pb);
  }
};

// A pair of a workgroup: thread t takes the reads t + 512 j.  Everything a decision rests on is a block sum, the same bits in every
// thread: the control flow is uniform over the workgroup.  (The loops are not unrolled, as in K15's workgroup form.)
struct LkBlockPair {
  const double* sa; const double* sb; int64_t n; double* stage; double* sh; bool staged_w, staged_v;
  double pa, pb;
  template <int SIDE>
  struct Margin {
    const LkBlockPair& p;
    static __device__ __forceinline__ bool any(bool f) { return f; }
    template <bool WANT_G>
    __device__ __forceinline__ void eval(double pi, double& S, double& X) const {
      const double qp = 1.0 - pi;
      double s = 0.0, x = 0.0;
#pragma unroll 1
      for (int64_t i = threadIdx.x; i < p.n; i += kStBlockThreads) st_term<WANT_G>(p.template w<SIDE>(i), qp, pi, s, x);
      S = block_sum_f64<kStBlockWaves>(s, p.sh);
      X = block_sum_f64<kStBlockWaves>(x, p.sh);
    }
  };
  struct Link {
    const LkBlockPair& p;
    static __device__ __forceinline__ bool any(bool f) { return f; }
    template <bool WANT_G>
    __device__ __forceinline__ void eval(double D, double& S, double& X) const {
      double s = 0.0, x = 0.0;
#pragma unroll 1
      for (int64_t i = threadIdx.x; i < p.n; i += kStBlockThreads) lk_term<WANT_G>(p.staged_v ? p.stage[i] : p.v_of(i), D, s, x);
      S = block_sum_f64<kStBlockWaves>(s, p.sh);
      X = block_sum_f64<kStBlockWaves>(x, p.sh);
    }
  };
  template <int SIDE>
  __device__ __forceinline__ double w(int64_t i) const {
    if (staged_w) return stage[SIDE * n + i];
    return SIDE == 0 ? lk_signed_t(sa[i], sb[i]) : lk_signed_t(sb[i], sa[i]);
  }
  __device__ __forceinline__ double v_of(int64_t i) const { return lk_u(w<0>(i), pa) * lk_u(w<1>(i), pb); }
  __device__ __forceinline__ Margin<0> row_a() const { return Margin<0>{*this}; }
  __device__ __forceinline__ Margin<1> row_b() const { return Margin<1>{*this}; }
  __device__ __forceinline__ Link row_v() const { return Link{*this}; }
  __device__ __forceinline__ void make_v(double a, double b) {
    pa = a; pb = b;
    if (staged_v)                                             // word i replaces this thread's own t of side a; side b's lie beyond n
      for (int64_t i = threadIdx.x; i < n; i += kStBlockThreads) stage[i] = v_of(i);
    staged_w = staged_w && !staged_v;                         // (2 n <= kLkStage implies n <= kLkStage: the t are gone)
  }
};

// K14's estimate of one row: 0 iff S(0) <= 0, else 1 iff S(1) >= 0, else the root of S by the bracketed iteration
template <class Row>
__device__ __forceinline__ double lk_margin(const LkArgs& a, const Row& row, bool run, bool& nc) {
  double S0, g0, S1, g1, x;
  int ev;
  row.template eval<true>(0.0, S0, g0);
  row.template eval<true>(1.0, S1, g1);
  const bool at0 = S0 <= 0.0, at1 = !at0 && S1 >= 0.0;
  st_solve<0>(row, run && !at0 && !at1, 0.0, 1.0, 0.0, 0.0, a.max_iter, a.tol, x, ev, nc);
  return at0 ? 0.0 : (at1 ? 1.0 : x);
}

// Everything between a pair's first sums (cnt: the reads valid at both sites, Ta, Tb: the sums of t of the two rows) and its outputs;
// `lead`: the thread that writes them
template <class Pair>
__device__ __forceinline__ void lk_estimate(const LkArgs& a, Pair& pair, bool have, bool lead, int64_t pos, double cnt, double Ta, double Tb) {
  const int n = (int)cnt;
  const bool too_few = n < a.min_reads, flat = !too_few && (!(Ta > 0.0) || !(Tb > 0.0));
  const bool run = have && !too_few && !flat;
  bool nca, ncb, ncd, nclo, nchi;
  const double pa = lk_margin(a, pair.row_a(), run, nca);
  const double pb = lk_margin(a, pair.row_b(), run, ncb);
  const double qa = 1.0 - pa, qb = 1.0 - pb;
  const bool degenerate = pa == 0.0 || pa == 1.0 || pb == 0.0 || pb == 1.0;
  const bool run_d = run && !degenerate;
  pair.make_v(pa, pb);
  const auto link = pair.row_v();
  const double d_min = -fmin(pa * pb, qa * qb), d_max = fmin(pa * qb, qa * pb);
  double Smin, gmin, Smax, gmax, x, xlo, xhi, Sh, gh;
  int iters, ev;
  link.template eval<true>(d_min, Smin, gmin);
  link.template eval<true>(d_max, Smax, gmax);
  const bool at_min = Smin <= 0.0, at_max = !at_min && Smax >= 0.0;
  st_solve<0>(link, run_d && !at_min && !at_max, d_min, d_max, 0.0, 0.0, a.max_iter, a.tol, x, iters, ncd);
  const double dhat = at_min ? d_min : (at_max ? d_max : x);
  link.template eval<true>(dhat, Sh, gh);
  const bool want_ci = a.out.d_lo || a.out.d_hi;
  const bool lo_end = 2.0 * (gh - gmin) <= a.drop, hi_end = 2.0 * (gh - gmax) <= a.drop;
  const bool run_lo = run_d && want_ci && !lo_end, run_hi = run_d && want_ci && !hi_end;
  st_solve<1>(link, run_lo, d_min, dhat, gh, a.drop, a.max_iter, a.tol, xlo, ev, nclo);
  st_solve<2>(link, run_hi, dhat, d_max, gh, a.drop, a.max_iter, a.tol, xhi, ev, nchi);
  if (have && lead) {
    const nmod_link_out& o = a.out;
    if (!run) {
      lk_write_nan(o, pos, n, too_few ? NMOD_LINK_TOO_FEW : NMOD_LINK_FLAT);
    } else {
      const unsigned nc_margin = nca || ncb ? NMOD_LINK_NOT_CONVERGED : 0;
      if (o.pa) o.pa[pos] = pa;
      if (o.pb) o.pb[pos] = pb;
      if (o.n_valid) o.n_valid[pos] = n;
      if (degenerate) {
        if (o.d) o.d[pos] = 0.0;
        if (o.d_lo) o.d_lo[pos] = 0.0;
        if (o.d_hi) o.d_hi[pos] = 0.0;
        if (o.r) o.r[pos] = nan_f64();
        if (o.stat) o.stat[pos] = 0.0;
        if (o.p_indep) o.p_indep[pos] = 1.0;
        if (o.iters) o.iters[pos] = 0;
        if (o.status) o.status[pos] = (uint8_t)(NMOD_LINK_DEGENERATE | nc_margin);
      } else {
        const double stat = fmax(2.0 * gh, 0.0);
        if (o.d) o.d[pos] = dhat;
        if (o.d_lo) o.d_lo[pos] = lo_end ? d_min : xlo;
        if (o.d_hi) o.d_hi[pos] = hi_end ? d_max : xhi;
        if (o.r) o.r[pos] = dhat / sqrt((pa * qa) * (pb * qb));
        if (o.stat) o.stat[pos] = stat;
        if (o.p_indep) o.p_indep[pos] = fmax(erfc(sqrt(stat / 2.0)), kDblMin);
        if (o.iters) o.iters[pos] = iters;
        if (o.status) o.status[pos] = (uint8_t)(nc_margin | (ncd || nclo || nchi ? NMOD_LINK_NOT_CONVERGED : 0) | (at_min ? NMOD_LINK_AT_MIN : 0) |
                                                (at_max ? NMOD_LINK_AT_MAX : 0));
      }
    }
  }
}

template <int G>
__global__ __launch_bounds__(kLkThreads) void lk_reg_kernel(LkArgs a) {
  const int gl = threadIdx.x & (G - 1);
  for (GroupWalk<G == 16 ? 0 : 1, G, kLkThreads> it(a.pl); it.more(); it.next()) {
    const bool have = it.have();
    int64_t pos = 0, yb = 0, yn = 0;
    if (have) {
      pos = it.pos();
      csr_row(a.off, 0, pos, yb, yn);
    }
    const int ny = (int)yn;
    LkRegPair<G> pair;
    double c = 0.0, Ta = 0.0, Tb = 0.0;
#pragma unroll
    for (int j = 0; j < kStPer; ++j) {
      const int idx = gl + G * j;
      const double s0 = idx < ny ? a.sa[yb + idx] : nan_f64(), s1 = idx < ny ? a.sb[yb + idx] : nan_f64();
      pair.ra.w[j] = lk_signed_t(s0, s1);
      pair.rb.w[j] = lk_signed_t(s1, s0);
      c += st_valid(s0) && st_valid(s1) ? 1.0 : 0.0;
      Ta += fabs(pair.ra.w[j]);
      Tb += fabs(pair.rb.w[j]);
    }
    c = group_sum_f64<G>(c);                                  // (a count of up to 1 024 ones: exact)
    Ta = group_sum_f64<G>(Ta);
    Tb = group_sum_f64<G>(Tb);
    lk_estimate(a, pair, have, gl == 0, pos, c, Ta, Tb);
  }
}

__global__ __launch_bounds__(kStBlockThreads) void lk_block_kernel(LkArgs a) {
  __shared__ double stage[kLkStage];
  __shared__ double sh[kStBlockWaves];
  const int tid = threadIdx.x;
  for (BlockWalk<2> it(a.pl); it.more(); it.next()) {
    const int64_t pos = it.pos();
    int64_t yb, yn;
    csr_row(a.off, 0, pos, yb, yn);
    const double* s0 = a.sa + yb;
    const double* s1 = a.sb + yb;
    const bool staged_w = 2 * yn <= kLkStage, staged_v = yn <= kLkStage;
    double c = 0.0, Ta = 0.0, Tb = 0.0;
    for (int64_t i = tid; i < yn; i += kStBlockThreads) {
      const double x0 = s0[i], x1 = s1[i];
      const double wa = lk_signed_t(x0, x1), wb = lk_signed_t(x1, x0);
      if (staged_w) { stage[i] = wa; stage[yn + i] = wb; }    // read back by this thread alone
      c += st_valid(x0) && st_valid(x1) ? 1.0 : 0.0;
      Ta += fabs(wa);
      Tb += fabs(wb);
    }
    c = block_sum_f64<kStBlockWaves>(c, sh);                  // (a count of up to 2^24 ones: exact)
    Ta = block_sum_f64<kStBlockWaves>(Ta, sh);
    Tb = block_sum_f64<kStBlockWaves>(Tb, sh);
    LkBlockPair pair{s0, s1, yn, stage, sh, staged_w, staged_v, 0.0, 0.0};
    lk_estimate(a, pair, true, tid == 0, pos, c, Ta, Tb);
  }
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_pair_linkage(const nmod_params* prm, int64_t npairs, const double* sa, const double* sb, const int64_t* prow_off,
                                 const nmod_link_opts* opts, const nmod_link_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_link_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_link_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->max_iter < 1 || opts->max_iter > 200 || opts->min_reads < 1) return NMOD_ERR_INVALID_ARG;
  if (!(opts->tol >= 0.0) || !(opts->tol <= kDblMax) || !(opts->ci_drop > 0.0) || !(opts->ci_drop <= kDblMax)) return NMOD_ERR_INVALID_ARG;
  if (npairs < 0 || npairs > (int64_t)INT32_MAX - 1) return NMOD_ERR_INVALID_ARG;
  if (npairs > 0 && !prow_off) return NMOD_ERR_INVALID_ARG;
  // (host rows that are all empty need no scores)
  if (npairs > 0 && (!sa || !sb) && (prm->memspace != NMOD_MEM_HOST || prow_off[npairs] > 0)) return NMOD_ERR_INVALID_ARG;
  int num_cus = 0;
  const int rc = rows_begin(prm, npairs, prow_off, &num_cus);
  if (rc != NMOD_OK || npairs == 0) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  const size_t np = (size_t)npairs;
  const size_t tot = host ? (size_t)prow_off[npairs] : 0;

  LkArgs a;
  memset(&a, 0, sizeof(a));
  a.sa = sa; a.sb = sb; a.off = prow_off; a.npos = npairs;
  a.max_iter = opts->max_iter; a.min_reads = opts->min_reads; a.tol = opts->tol; a.drop = opts->ci_drop;
  a.out = *out;

  // one slab: the three work lists and their count words; for the host entry the inputs and outputs as well
  Slab slab(host);
  const PosListSpace<3> lists(slab, np);
  slab.in(a.off, (np + 1) * 8); slab.in(a.sa, tot * 8); slab.in(a.sb, tot * 8);
  slab.out(a.out.pa, np * 8); slab.out(a.out.pb, np * 8); slab.out(a.out.d, np * 8); slab.out(a.out.d_lo, np * 8);
  slab.out(a.out.d_hi, np * 8); slab.out(a.out.r, np * 8); slab.out(a.out.stat, np * 8); slab.out(a.out.p_indep, np * 8);
  slab.out(a.out.n_valid, np * 4); slab.out(a.out.iters, np * 4); slab.out(a.out.status, np);
  NMOD_HIP(slab.commit(stream, prm->device));
  NMOD_HIP(lists.fill<LkRule>(slab, a, num_cus, stream));
  launch_groups<16, kLkThreads>(lk_reg_kernel<16>, a, num_cus, stream);
  launch_groups<64, kLkThreads>(lk_reg_kernel<64>, a, num_cus, stream);
  launch_blocks<kStBlockThreads>(lk_block_kernel, a, num_cus, stream);
  return launches_end(slab, stream);
}
