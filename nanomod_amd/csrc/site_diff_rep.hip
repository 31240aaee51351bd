// nmod_site_diff_rep — the modified shares of two replicated conditions compared per site from pivoted window sums: every replicate's
// estimate, K15's condition-level fit of the pooled reads, the heterogeneity of the replicates and the F(1, G - 2) test and interval
// of delta that carry it, on the device (K24).  The reference project has no such step; the definition is the one in
// include/nanomod_hip.h (tests/diff_rep_ref.py restates it in numpy).  K15's shape (site_diff.hip): the two condition super-rows of a
// site are its two resident rows, in K15's lane layout, reduction order and LDS stage, so that the condition level has K15's bits.
// All on the caller's stream:
//   pos_classify_kernel<DrRule>  (pos_walk.hpp) a thread per site: its class by the longer super-row; a site with a super-row beyond
//                        NMOD_MAX_DEEP gets its NaN outputs and status here
//   dr_reg_kernel<16>    both super-rows <= 128: 16 lanes x (8 + 8) signed t values in registers over all iterations
//   dr_reg_kernel<64>    both super-rows <= 512: the whole wave x (8 + 8)
//   dr_block_kernel      beyond: a workgroup per site, K15's stage
//   dr_tail_kernel       a thread per site: p_cond, p_het and p_rep from the statistics the kernels above left in their places
// nmod_site_diff_rep_mod (K25) is the same launches with the MOD instances of the three iterating kernels and dr_tail_mod_kernel: they
// read the record of nmod_rep_prior (rep_prior.hip) from device memory, take the posterior dispersion for phi_used and the record's
// quantile for the drop; the plain instances keep their code and their bytes.
// The saturated fit: a sample is an index range of its super-row, and a sample view hands st_solve the super-row with every element
// outside the range as w = 0, which adds exactly 0 to S, D and g (st_term).  The register forms mask the registers they hold; the
// workgroup form walks the range alone, a thread over the words t + 512 j of the super-row it staged itself.  The lane (thread)
// partials are rotated by the sample's offset before they are reduced, so that a sample's sums run in the sample's own order and
// its bits do not depend on where in the super-row it lies.  G roots, one after the other, no second read of the scores.  No float atomics: a site's bits depend on its rows, G and ncontrol alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "pos_walk.hpp"
#include "site_diff_views.hpp"
#include "special_math.hpp"
#include "stoich_rows.hpp"

namespace nmod {

static_assert(NMOD_REP_TOO_FEW == NMOD_DIFF_TOO_FEW && NMOD_REP_FLAT == NMOD_DIFF_FLAT && NMOD_REP_NOT_CONVERGED == NMOD_DIFF_NOT_CONVERGED &&
              NMOD_REP_POOL_AT_END == NMOD_DIFF_POOL_AT_END && NMOD_REP_TOO_LARGE == NMOD_DIFF_TOO_LARGE, "K15's status values");

struct DrArgs {
  const double* score; const int64_t* off;
  int64_t npos;
  int G, nc;                                      // samples per site; those of condition 0
  int max_iter, min_valid; double tol, ci_drop, phi_floor;
  nmod_rep_out out;
  PosLists<3> pl;
  const double* prior; double* phi_post;          // nmod_site_diff_rep_mod alone (the MOD instances): K25's record, the moderated dispersion
};

// the outputs of a site without an estimate; n_valid is the caller's
__device__ __forceinline__ void dr_write_nan(const DrArgs& a, int64_t i, unsigned status) {
  const nmod_rep_out& o = a.out;
  const double nan = nan_f64();
  if (o.pi_s) for (int g = 0; g < a.G; ++g) o.pi_s[i * a.G + g] = nan;
  if (o.pi0) o.pi0[i] = nan;
  if (o.pi1) o.pi1[i] = nan;
  if (o.pi_pool) o.pi_pool[i] = nan;
  if (o.delta) o.delta[i] = nan;
  if (o.delta_lo) o.delta_lo[i] = nan;
  if (o.delta_hi) o.delta_hi[i] = nan;
  if (o.stat_cond) o.stat_cond[i] = nan;
  if (o.p_cond) o.p_cond[i] = nan;
  if (o.stat_het) o.stat_het[i] = nan;
  if (o.p_het) o.p_het[i] = nan;
  if (o.phi) o.phi[i] = nan;
  if (o.p_rep) o.p_rep[i] = nan;
  if (a.phi_post) a.phi_post[i] = nan;
  if (o.iters) o.iters[i] = 0;
  if (o.status) o.status[i] = (uint8_t)status;
}

// the two super-rows of site i: their first scores and lengths (offsets that decrease: an empty row)
__device__ __forceinline__ void dr_rows(const DrArgs& a, int64_t i, int64_t& b0, int64_t& m0, int64_t& b1, int64_t& m1) {
  const int64_t* o = a.off + i * a.G;
  b0 = o[0]; b1 = o[a.nc];
  m0 = b1 - b0; m1 = o[a.G] - b1;
  if (m0 < 0) m0 = 0;
  if (m1 < 0) m1 = 0;
}

// sample g of site i as a range [lo, hi) of its super-row of m scores
__device__ __forceinline__ void dr_range(const DrArgs& a, int64_t i, int g, int64_t m, int64_t& lo, int64_t& hi) {
  const int64_t* o = a.off + i * a.G;
  const int64_t b = o[g < a.nc ? 0 : a.nc];
  lo = o[g] - b; hi = o[g + 1] - b;
  lo = lo < 0 ? 0 : (lo > m ? m : lo);
  hi = hi < lo ? lo : (hi > m ? m : hi);
}

// the class of site i by the longer of its super-rows, K15's steps; a site with a super-row beyond NMOD_MAX_DEEP is left out
struct DrRule {
  static constexpr int NC = 3;
  using Track = void;
  static __device__ __forceinline__ int cls(const DrArgs& a, int64_t i, int64_t& yb, int64_t& yn) {
    int64_t b1, n1;
    dr_rows(a, i, yb, yn, b1, n1);
    const int64_t m = yn > n1 ? yn : n1;
    if (m > NMOD_MAX_DEEP) {
      if (a.out.n_valid) for (int g = 0; g < a.G; ++g) a.out.n_valid[i * a.G + g] = 0;
      dr_write_nan(a, i, NMOD_REP_TOO_LARGE);
      return -1;
    }
    return m <= kDfSmall ? 0 : (m <= kDfWave ? 1 : 2);
  }
};

// A sample of a register pair: the super-row `second` with every element outside [lo, hi) as w = 0.  (Both rows are named with
// constant indices and chosen by a select: a pointer to one of them would send the registers to scratch.)
// The order of a sample's sums is the sample's own, whatever its offset in the super-row: element k of the sample sits in lane
// (lo + k) mod G, so the chain of lane L — its registers in ascending index, the masked ones adding exactly 0 — is the chain over
// the elements k = l + G j of the sample for l = (L - lo) mod G.  The lane partials are rotated by lo mod G before the lane
// reduction, which then sees them in the order of l: a sample's bits do not move with the samples before it.
template <int G>
struct DrRegSample {
  const DfRegPair<G>& p; bool second; int lo, hi, gl;
  static __device__ __forceinline__ bool any(bool f) { return __any(f); }
  __device__ __forceinline__ double w(int j) const {
    const int idx = gl + G * j;
    return idx >= lo && idx < hi ? (second ? p.w1[j] : p.w0[j]) : 0.0;
  }
  template <bool WANT_G>
  __device__ __forceinline__ void eval(double pi, double& S, double& X) const {
    const double qp = 1.0 - pi;
    double s = 0.0, x = 0.0;
#pragma unroll
    for (int j = 0; j < kDfPer; ++j) st_term<WANT_G>(w(j), qp, pi, s, x);
    const int src = (gl + lo) & (G - 1);                      // the lane that holds the partial of l = gl
    S = group_sum_f64<G>(__shfl(s, src, G));
    X = group_sum_f64<G>(__shfl(x, src, G));
  }
};

// A sample of a workgroup: the range [lo, hi) of a super-row whose staged words begin at `stage` and whose scores at `sc`; thread t
// takes the elements t + 512 j of the super-row that fall inside, the words it staged itself.  As in the register forms the thread
// partials are rotated by lo mod 512, through the 2 x 512 words of `rot`, before the workgroup reduction.  (block_sum_f64 waits
// twice after the partials are read back: the next evaluation's writes to `rot` cannot overtake a read.)
struct DrBlockSample {
  const double* sc; const double* stage; int64_t lo, hi; double* sh; double* rot; bool staged;
  static __device__ __forceinline__ bool any(bool f) { return f; }
  __device__ __forceinline__ int64_t first() const { return lo + (((int64_t)threadIdx.x - lo) & (kStBlockThreads - 1)); }
  template <bool WANT_G>
  __device__ __forceinline__ void eval(double pi, double& S, double& X) const {
    const double qp = 1.0 - pi;
    double s = 0.0, x = 0.0;
#pragma unroll 1
    for (int64_t i = first(); i < hi; i += kStBlockThreads) st_term<WANT_G>(staged ? stage[i] : st_signed_t(sc[i]), qp, pi, s, x);
    const int own = (int)(((int64_t)threadIdx.x - lo) & (kStBlockThreads - 1));   // the l whose partial this thread made
    rot[own] = s; rot[kStBlockThreads + own] = x;
    __syncthreads();
    S = block_sum_f64<kStBlockWaves>(rot[threadIdx.x], sh);
    X = block_sum_f64<kStBlockWaves>(rot[kStBlockThreads + threadIdx.x], sh);
  }
};

// A record no site can be moderated with: a NaN in d0 or df_tot, a NaN in s0^2 where it is used (d0 > 0), a negative word among the
// first four.  The one rule: the MOD instances below skip the interval under it, dr_tail_mod_kernel writes what follows from it.
__device__ __forceinline__ bool dr_prior_bad(const double* prior) {
  const double d0 = prior[0], s0 = prior[1], dft = prior[2], ci = prior[3];
  return d0 != d0 || dft != dft || (d0 > 0.0 && s0 != s0) || d0 < 0.0 || s0 < 0.0 || dft < 0.0 || ci < 0.0;
}

// Everything between a site's counts and its outputs.  sample(g): the view of sample g; `lead`: the thread that writes.  The condition
// level is df_estimate's (site_diff.hip), operation for operation, with the saturated fit between its test and its interval: the drop
// of the interval needs the dispersion.
// MOD (nmod_site_diff_rep_mod): the dispersion is the posterior one under the record a.prior and the drop is scaled by the record's quantile.
template <bool MOD, class Pair, class SampleOf>
__device__ __forceinline__ void dr_estimate(const DrArgs& a, const Pair& pair, const SampleOf& sample, bool have, bool lead, int64_t pos,
                                            bool too_few, bool flat) {
  const bool run = have && !too_few && !flat;
  const bool want_ci = a.out.delta_lo || a.out.delta_hi;
  double S00, g00, S10, g10, S01, g01, S11, g11;              // S<row><pi>, g<row><pi> at pi = 0 and 1
  pair.template eval2<true>(0.0, 0.0, S00, g00, S10, g10);
  pair.template eval2<true>(1.0, 1.0, S01, g01, S11, g11);
  const bool a0z = S00 <= 0.0, a0o = !a0z && S01 >= 0.0, a1z = S10 <= 0.0, a1o = !a1z && S11 >= 0.0;
  const bool apz = S00 + S10 <= 0.0, apo = !apz && S01 + S11 >= 0.0;
  double x0, x1, xp, xlo, xhi;
  int ev, iters;
  bool nc0, nc1, ncp, nclo, nchi;
  st_solve<0>(DfView<0, Pair>{pair, 0.0}, run && !a0z && !a0o, 0.0, 1.0, 0.0, 0.0, a.max_iter, a.tol, x0, ev, nc0);
  st_solve<0>(DfView<1, Pair>{pair, 0.0}, run && !a1z && !a1o, 0.0, 1.0, 0.0, 0.0, a.max_iter, a.tol, x1, ev, nc1);
  st_solve<0>(DfView<2, Pair>{pair, 0.0}, run && !apz && !apo, 0.0, 1.0, 0.0, 0.0, a.max_iter, a.tol, xp, iters, ncp);
  const double pi0 = a0z ? 0.0 : (a0o ? 1.0 : x0), pi1 = a1z ? 0.0 : (a1o ? 1.0 : x1), pip = apz ? 0.0 : (apo ? 1.0 : xp);
  double Sa, ga, Sb, gb, Sc, gc, Sd, gd;
  pair.template eval2<true>(pi0, pi1, Sa, ga, Sb, gb);
  pair.template eval2<true>(pip, pip, Sc, gc, Sd, gd);
  const double ghat = ga + gb, gpool = gc + gd;
  const double stat = fmax(2.0 * (ghat - gpool), 0.0);
  const double delta = pi1 - pi0;

  // the saturated fit: K14's estimate of every sample, its g summed in ascending g
  double gsat = 0.0;
  bool ncs = false;
#pragma unroll 1
  for (int g = 0; g < a.G; ++g) {
    const auto view = sample(g);
    double Sz, Xz, So, Xo, xs, Ss, gs;
    bool c;
    view.template eval<false>(0.0, Sz, Xz);
    view.template eval<false>(1.0, So, Xo);
    const bool az = Sz <= 0.0, ao = !az && So >= 0.0;
    st_solve<0>(view, run && !az && !ao, 0.0, 1.0, 0.0, 0.0, a.max_iter, a.tol, xs, ev, c);
    const double pis = az ? 0.0 : (ao ? 1.0 : xs);
    view.template eval<true>(pis, Ss, gs);
    gsat += gs;
    ncs = ncs || c;
    if (run && lead && a.out.pi_s) a.out.pi_s[pos * a.G + g] = pis;
  }
  const double df = (double)(a.G - 2);
  const double stat_het = fmax(2.0 * (gsat - ghat), 0.0);
  const double phi = stat_het / df;
  double phi_post = phi, ci_drop = a.ci_drop;
  bool bad = false;
  if constexpr (MOD) {
    const double d0 = a.prior[0], s0 = a.prior[1];
    bad = dr_prior_bad(a.prior);
    ci_drop = bad ? 0.0 : a.prior[3];                         // (a drop of 0: no interval root runs; the tail kernel writes the NaN)
    if (d0 == 0.0) phi_post = phi;
    else if (d0 > kDblMax) phi_post = s0;
    else phi_post = (d0 * s0 + df * phi) / (d0 + df);
  }
  const double phi_used = fmax(phi_post, a.phi_floor);
  const double F = stat == 0.0 ? 0.0 : stat / phi_used;       // (phi_used == 0: +inf, whose tail the clamp turns into DBL_MIN)
  const double drop = phi_used * ci_drop;

  double gm = g01 + g10, gp = g00 + g11;                      // h(-1) = g0(1) + g1(0), h(+1) = g0(0) + g1(1)
  if constexpr (Pair::kAgain) {                               // (the workgroup form evaluates them here again, the same bits, as K15 does)
    double Se, ge0, Sf, ge1;
    pair.template eval2<true>(1.0, 0.0, Se, ge0, Sf, ge1);
    gm = ge0 + ge1;
    pair.template eval2<true>(0.0, 1.0, Se, ge0, Sf, ge1);
    gp = ge0 + ge1;
  }
  const bool point = !(drop > 0.0);                           // no dispersion and no floor: the interval is delta itself
  const bool lo_end = 2.0 * (ghat - gm) <= drop, hi_end = 2.0 * (ghat - gp) <= drop;
  const bool run_lo = run && want_ci && !lo_end && !point, run_hi = run && want_ci && !hi_end && !point;
  const DfProfile<Pair> prof_lo{pair, run_lo, a.max_iter, a.tol, false}, prof_hi{pair, run_hi, a.max_iter, a.tol, false};
  st_solve<1>(prof_lo, run_lo, -1.0, delta, ghat, drop, a.max_iter, a.tol, xlo, ev, nclo);
  st_solve<2>(prof_hi, run_hi, delta, 1.0, ghat, drop, a.max_iter, a.tol, xhi, ev, nchi);
  if (have && lead) {
    const nmod_rep_out& o = a.out;
    if (!run) {
      dr_write_nan(a, pos, too_few ? NMOD_REP_TOO_FEW : NMOD_REP_FLAT);
    } else {
      if (o.pi0) o.pi0[pos] = pi0;
      if (o.pi1) o.pi1[pos] = pi1;
      if (o.pi_pool) o.pi_pool[pos] = pip;
      if (o.delta) o.delta[pos] = delta;
      if (o.delta_lo) o.delta_lo[pos] = point ? delta : (lo_end ? -1.0 : xlo);
      if (o.delta_hi) o.delta_hi[pos] = point ? delta : (hi_end ? 1.0 : xhi);
      if (o.stat_cond) o.stat_cond[pos] = stat;
      if (o.p_cond) o.p_cond[pos] = stat;                     // (dr_tail_kernel turns these three into the tails)
      if (o.stat_het) o.stat_het[pos] = stat_het;
      if (o.p_het) o.p_het[pos] = stat_het;
      if (o.phi) o.phi[pos] = phi;
      if (o.p_rep) o.p_rep[pos] = F;
      if constexpr (MOD) { if (a.phi_post) a.phi_post[pos] = phi_post; }
      if (o.iters) o.iters[pos] = iters;
      if (o.status) o.status[pos] = (uint8_t)((nc0 || nc1 || ncp || ncs || nclo || nchi || prof_lo.nc || prof_hi.nc ? NMOD_REP_NOT_CONVERGED : 0) |
                                              (pip == 0.0 || pip == 1.0 ? NMOD_REP_POOL_AT_END : 0) |
                                              (stat != 0.0 && phi_used == 0.0 && !bad ? NMOD_REP_PHI_ZERO : 0));
    }
  }
}

// two waves per SIMD: the register budget of K15's forms
template <int G, bool MOD>
__global__ __launch_bounds__(kDfThreads, 2) void dr_reg_kernel(DrArgs a) {
  const int gl = threadIdx.x & (G - 1);
  for (GroupWalk<G == 16 ? 0 : 1, G, kDfThreads> it(a.pl); it.more(); it.next()) {
    const bool have = it.have();
    int64_t pos = 0, b0 = 0, m0 = 0, b1 = 0, m1 = 0;
    if (have) {
      pos = it.pos();
      dr_rows(a, pos, b0, m0, b1, m1);
    }
    const int ny0 = (int)m0, ny1 = (int)m1;
    DfRegPair<G> pair;
    unsigned ok0 = 0u, ok1 = 0u;                              // bit j: whether the lane's score j of the row is valid
#pragma unroll
    for (int j = 0; j < kDfPer; ++j) {
      const int idx = gl + G * j;
      const double s0 = idx < ny0 ? a.score[b0 + idx] : nan_f64();
      const double s1 = idx < ny1 ? a.score[b1 + idx] : nan_f64();
      pair.w0[j] = st_signed_t(s0);
      pair.w1[j] = st_signed_t(s1);
      ok0 |= st_valid(s0) ? 1u << j : 0u;
      ok1 |= st_valid(s1) ? 1u << j : 0u;
    }
    // every sample's count and sum of t, over the same registers (counts of up to 512 ones: exact)
    bool too_few = false, any_flat = false;
#pragma unroll 1
    for (int g = 0; g < a.G; ++g) {
      const bool second = g >= a.nc;
      int64_t lo = 0, hi = 0;
      if (have) dr_range(a, pos, g, second ? m1 : m0, lo, hi);
      const DrRegSample<G> view{pair, second, (int)lo, (int)hi, gl};
      const unsigned ok = second ? ok1 : ok0;
      double c = 0.0, T = 0.0;
#pragma unroll
      for (int j = 0; j < kDfPer; ++j) {
        const int idx = gl + G * j;
        c += idx >= (int)lo && idx < (int)hi && (ok >> j & 1u) ? 1.0 : 0.0;
        T += fabs(view.w(j));
      }
      c = group_sum_f64<G>(c); T = group_sum_f64<G>(T);
      const int n = (int)c;
      too_few = too_few || n < a.min_valid;
      any_flat = any_flat || !(T > 0.0);
      if (have && gl == 0 && a.out.n_valid) a.out.n_valid[pos * a.G + g] = n;
    }
    const auto sample = [&](int g) {
      const bool second = g >= a.nc;
      int64_t lo = 0, hi = 0;
      if (have) dr_range(a, pos, g, second ? m1 : m0, lo, hi);
      return DrRegSample<G>{pair, second, (int)lo, (int)hi, gl};
    };
    dr_estimate<MOD>(a, pair, sample, have, gl == 0, pos, too_few, !too_few && any_flat);
  }
}

template <bool MOD>
__global__ __launch_bounds__(kStBlockThreads) void dr_block_kernel(DrArgs a) {
  __shared__ double stage[kDfStage];
  __shared__ double sh[kStBlockWaves];
  __shared__ double rot[2 * kStBlockThreads];
  const int tid = threadIdx.x;
  for (BlockWalk<2> it(a.pl); it.more(); it.next()) {
    const int64_t pos = it.pos();
    int64_t b0, m0, b1, m1;
    dr_rows(a, pos, b0, m0, b1, m1);
    const double *sc0 = a.score + b0, *sc1 = a.score + b1;
    const bool staged = m0 + m1 <= kDfStage;
    // K15's staging (thread t: the words t + 512 j of each row, row 1 behind row 0), a sample at a time for its count and sum of t
    // (counts of up to 2^24 ones: exact)
    bool too_few = false, any_flat = false;
#pragma unroll 1
    for (int g = 0; g < a.G; ++g) {
      const bool second = g >= a.nc;
      int64_t lo, hi;
      dr_range(a, pos, g, second ? m1 : m0, lo, hi);
      const double* sc = second ? sc1 : sc0;
      double* st = stage + (second ? m0 : 0);
      double c = 0.0, T = 0.0;
#pragma unroll 1
      for (int64_t i = lo + (((int64_t)tid - lo) & (kStBlockThreads - 1)); i < hi; i += kStBlockThreads) {
        const double s = sc[i], wt = st_signed_t(s);
        if (staged) st[i] = wt;                               // read back by this thread alone
        c += st_valid(s) ? 1.0 : 0.0;
        T += fabs(wt);
      }
      c = block_sum_f64<kStBlockWaves>(c, sh); T = block_sum_f64<kStBlockWaves>(T, sh);
      const int n = (int)c;
      too_few = too_few || n < a.min_valid;
      any_flat = any_flat || !(T > 0.0);
      if (tid == 0 && a.out.n_valid) a.out.n_valid[pos * a.G + g] = n;
    }
    const DfBlockPair pair{sc0, m0, sc1, m1, stage, sh, staged};
    const auto sample = [&](int g) {
      const bool second = g >= a.nc;
      int64_t lo, hi;
      dr_range(a, pos, g, second ? m1 : m0, lo, hi);
      return DrBlockSample{second ? sc1 : sc0, stage + (second ? m0 : 0), lo, hi, sh, rot, staged};
    };
    dr_estimate<MOD>(a, pair, sample, true, tid == 0, pos, too_few, !too_few && any_flat);
  }
}

// p_cond, p_het and p_rep from the statistics the kernels above left in their places (NaN stays NaN): the tail functions stay out of
// the iterating kernels.  df = G - 2.
__global__ __launch_bounds__(256) void dr_tail_kernel(double* p_cond, double* p_het, double* p_rep, int df, int64_t npos) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npos; i += (int64_t)gridDim.x * 256) {
    if (p_cond) {
      const double stat = p_cond[i];
      if (stat == stat) p_cond[i] = fmax(erfc(sqrt(0.5 * stat)), kDblMin);
    }
    if (p_het) {
      const double stat = p_het[i];
      if (stat == stat) p_het[i] = fmax(df & 1 ? chi2_sf_odd(stat, df >> 1) : chi2_sf_even(stat, df >> 1), kDblMin);
    }
    if (p_rep) {
      const double F = p_rep[i];
      const double p = student_t_two_sided(sqrt(F), (double)df);   // (reached by every lane of the loop's trip: it votes)
      if (F == F) p_rep[i] = fmax(p, kDblMin);
    }
  }
}

// nmod_site_diff_rep_mod's tail: p_cond and p_het as above; p_rep on the record's df_tot degrees of freedom (+inf: the normal tail of
// sqrt(F), erfc(sqrt(F / 2))); and, decided here once for every site, with or without an estimate, what a record that cannot be used
// does: NaN p_rep, phi_post and interval, and NMOD_REP_BAD_PRIOR.
__global__ __launch_bounds__(256) void dr_tail_mod_kernel(DrArgs a) {
  const nmod_rep_out& o = a.out;
  const int df = a.G - 2;
  const bool bad = dr_prior_bad(a.prior);
  const double dft = a.prior[2];
  const bool normal = dft > kDblMax;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.npos; i += (int64_t)gridDim.x * 256) {
    if (o.p_cond) {
      const double stat = o.p_cond[i];
      if (stat == stat) o.p_cond[i] = fmax(erfc(sqrt(0.5 * stat)), kDblMin);
    }
    if (o.p_het) {
      const double stat = o.p_het[i];
      if (stat == stat) o.p_het[i] = fmax(df & 1 ? chi2_sf_odd(stat, df >> 1) : chi2_sf_even(stat, df >> 1), kDblMin);
    }
    if (o.p_rep) {
      const double F = o.p_rep[i];
      const double p = normal ? erfc(sqrt(0.5 * F)) : student_t_two_sided(sqrt(F), bad ? 1.0 : dft);   // (every lane of the trip votes)
      if (F == F) o.p_rep[i] = fmax(p, kDblMin);
    }
    if (bad) {
      const double nan = nan_f64();
      if (o.p_rep) o.p_rep[i] = nan;
      if (a.phi_post) a.phi_post[i] = nan;
      if (o.delta_lo) o.delta_lo[i] = nan;
      if (o.delta_hi) o.delta_hi[i] = nan;
      if (o.status) o.status[i] = (uint8_t)(o.status[i] | NMOD_REP_BAD_PRIOR);
    }
  }
}

}  // namespace nmod

using namespace nmod;

// both entries; MOD: nmod_site_diff_rep_mod, with the record `prior` and the output `phi_post` (or NULL)
template <bool MOD>
static int dr_entry(const nmod_params* prm, int64_t npos, int32_t nsamples, int32_t ncontrol, const double* score, const int64_t* off,
                    const nmod_rep_opts* opts, const nmod_rep_out* out, const double* prior, double* phi_post) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_rep_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_rep_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->max_iter < 1 || opts->max_iter > 200 || opts->min_valid < 1) return NMOD_ERR_INVALID_ARG;
  if (!(opts->tol >= 0.0) || !(opts->tol <= kDblMax) || !(opts->ci_drop > 0.0) || !(opts->ci_drop <= kDblMax)) return NMOD_ERR_INVALID_ARG;
  if (!(opts->phi_floor >= 0.0) || !(opts->phi_floor <= kDblMax)) return NMOD_ERR_INVALID_ARG;
  if (nsamples < 3 || nsamples > NMOD_REP_MAX_SAMPLES || ncontrol < 1 || ncontrol > nsamples - 1) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > ((int64_t)INT32_MAX - 1) / nsamples) return NMOD_ERR_INVALID_ARG;
  if (!off || (npos > 0 && !score) || (MOD && !prior)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  const int64_t nrows = npos * nsamples;
  int num_cus = 0;
  const int rc = rows_begin(prm, nrows, off, &num_cus);
  if (rc != NMOD_OK || npos == 0) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t np = (size_t)npos, nr = (size_t)nrows;
  const size_t tot = host ? (size_t)off[nrows] : 0;

  DrArgs a;
  memset(&a, 0, sizeof(a));
  a.score = score; a.off = off;
  a.npos = npos;
  a.G = nsamples; a.nc = ncontrol;
  a.max_iter = opts->max_iter; a.min_valid = opts->min_valid; a.tol = opts->tol; a.ci_drop = opts->ci_drop; a.phi_floor = opts->phi_floor;
  a.out = *out;
  a.prior = prior; a.phi_post = phi_post;

  // one slab: the three work lists and their count words; for the host entry the inputs and outputs as well
  Slab slab(host);
  const PosListSpace<3> lists(slab, np);
  slab.in(a.off, (nr + 1) * 8); slab.in(a.score, tot * 8);
  slab.out(a.out.pi_s, nr * 8); slab.out(a.out.pi0, np * 8); slab.out(a.out.pi1, np * 8); slab.out(a.out.pi_pool, np * 8);
  slab.out(a.out.delta, np * 8); slab.out(a.out.delta_lo, np * 8); slab.out(a.out.delta_hi, np * 8);
  slab.out(a.out.stat_cond, np * 8); slab.out(a.out.p_cond, np * 8); slab.out(a.out.stat_het, np * 8); slab.out(a.out.p_het, np * 8);
  slab.out(a.out.phi, np * 8); slab.out(a.out.p_rep, np * 8);
  slab.out(a.out.n_valid, nr * 4); slab.out(a.out.iters, np * 4); slab.out(a.out.status, np);
  if (MOD) { slab.in(a.prior, NMOD_REP_PRIOR_WORDS * 8); slab.out(a.phi_post, np * 8); }
  NMOD_HIP(slab.commit(stream, prm->device));
  NMOD_HIP(lists.fill<DrRule>(slab, a, num_cus, stream));
  launch_groups<16, kDfThreads>(dr_reg_kernel<16, MOD>, a, num_cus, stream);
  launch_groups<64, kDfThreads>(dr_reg_kernel<64, MOD>, a, num_cus, stream);
  launch_blocks<kStBlockThreads>(dr_block_kernel<MOD>, a, num_cus, stream);
  const dim3 tail_grid(persistent_grid(npos, 256, (int64_t)num_cus * 16));
  if (MOD)
    hipLaunchKernelGGL(dr_tail_mod_kernel, tail_grid, dim3(256), 0, stream, a);
  else if (a.out.p_cond || a.out.p_het || a.out.p_rep)
    hipLaunchKernelGGL(dr_tail_kernel, tail_grid, dim3(256), 0, stream, a.out.p_cond, a.out.p_het, a.out.p_rep, nsamples - 2, npos);
  return launches_end(slab, stream);
}

extern "C" int nmod_site_diff_rep(const nmod_params* prm, int64_t npos, int32_t nsamples, int32_t ncontrol, const double* score,
                                  const int64_t* off, const nmod_rep_opts* opts, const nmod_rep_out* out) {
  return dr_entry<false>(prm, npos, nsamples, ncontrol, score, off, opts, out, nullptr, nullptr);
}

extern "C" int nmod_site_diff_rep_mod(const nmod_params* prm, int64_t npos, int32_t nsamples, int32_t ncontrol, const double* score,
                                      const int64_t* off, const nmod_rep_opts* opts, const nmod_rep_out* out, const double* prior,
                                      double* phi_post) {
  return dr_entry<true>(prm, npos, nsamples, ncontrol, score, off, opts, out, prior, phi_post);
}
