// nmod_site_diff — the modified shares of two samples compared per site from pivoted window sums: each sample's estimate, the pooled
// one, the likelihood-ratio test of pi0 = pi1 and the profile-likelihood interval of delta = pi1 - pi0, on the device (K15, DESIGN.md
// §3).  The reference project has no such step; the definition is the one in include/nanomod_hip.h (tests/diff_ref.py restates it in
// numpy).  K14's shape (site_stoich.hip) with two resident rows per site.  All on the caller's stream:
//   pos_classify_kernel<DfRule>  (pos_walk.hpp) a thread per site: its class by the longer of its two rows; a site with a row beyond
//                        NMOD_MAX_DEEP gets its NaN outputs and status here
//   df_reg_kernel<16>    both rows <= 128: 16 lanes x (8 + 8) signed t values hold the two rows in registers over all iterations, four
//                        sites per wave, DPP row sums only
//   df_reg_kernel<64>    both rows <= 512: the whole wave x (8 + 8)
//   df_tail_kernel       a thread per site: p_diff from stat
//   df_block_kernel      beyond: a workgroup per site, both rows' signed t staged in LDS up to kDfStage words in all (a thread reads back
//                        only the words it wrote itself), re-read and recomputed per evaluation beyond
// A pair policy evaluates both rows at (pi0, pi1), each row's sums reduced on their own; the views (site_diff_views.hpp, shared with
// K24) hand one row, or the sum of the two at (x, x + delta), or the profile over delta to K14's st_solve (stoich_rows.hpp).  Every
// sum is a fixed-order chain per lane followed by a fixed-order lane / wave / LDS reduction, no float atomics: a site's bits depend on
// its two rows alone.
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

struct DfArgs {
  const double* score0; const int64_t* off0; int64_t stride0;
  const double* score1; const int64_t* off1; int64_t stride1;
  int64_t npos;
  int max_iter, min_valid; double tol, drop;
  nmod_diff_out out;
  PosLists<3> pl;
};

__device__ __forceinline__ void df_write_nan(const nmod_diff_out& o, int64_t i, int n0, int n1, unsigned status) {
  const double nan = nan_f64();
  if (o.pi0) o.pi0[i] = nan;
  if (o.pi1) o.pi1[i] = nan;
  if (o.pi_pool) o.pi_pool[i] = nan;
  if (o.delta) o.delta[i] = nan;
  if (o.delta_lo) o.delta_lo[i] = nan;
  if (o.delta_hi) o.delta_hi[i] = nan;
  if (o.stat) o.stat[i] = nan;
  if (o.p_diff) o.p_diff[i] = nan;
  if (o.n_valid0) o.n_valid0[i] = n0;
  if (o.n_valid1) o.n_valid1[i] = n1;
  if (o.iters) o.iters[i] = 0;
  if (o.status) o.status[i] = (uint8_t)status;
}

// the class of site i by the longer of its rows; a site with a row beyond NMOD_MAX_DEEP is left out
struct DfRule {
  static constexpr int NC = 3;
  using Track = void;
  static __device__ __forceinline__ int cls(const DfArgs& a, int64_t i, int64_t& yb, int64_t& yn) {
    int64_t b1, n1;
    csr_row(a.off0, a.stride0, i, yb, yn);
    csr_row(a.off1, a.stride1, i, b1, n1);
    const int64_t m = yn > n1 ? yn : n1;
    if (m > NMOD_MAX_DEEP) { df_write_nan(a.out, i, 0, 0, NMOD_DIFF_TOO_LARGE); return -1; }
    return m <= kDfSmall ? 0 : (m <= kDfWave ? 1 : 2);
  }
};

// Everything between a site's first sums (c: valid scores, T: the sum of t, per row) and its outputs; `lead`: the thread that writes.
template <class Pair>
__device__ __forceinline__ void df_estimate(const DfArgs& a, const Pair& pair, bool have, bool lead, int64_t pos, double c0, double T0,
                                            double c1, double T1) {
  const int n0 = (int)c0, n1 = (int)c1;
  const bool too_few = n0 < a.min_valid || n1 < a.min_valid, flat = !too_few && (!(T0 > 0.0) || !(T1 > 0.0));
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
  double gm = g01 + g10, gp = g00 + g11;                      // h(-1) = g0(1) + g1(0), h(+1) = g0(0) + g1(1)
  if constexpr (Pair::kAgain) {                               // (the workgroup form evaluates them here again, the same bits, and does
    double Se, ge0, Sf, ge1;                                  // not keep four sums in registers across three roots)
    pair.template eval2<true>(1.0, 0.0, Se, ge0, Sf, ge1);
    gm = ge0 + ge1;
    pair.template eval2<true>(0.0, 1.0, Se, ge0, Sf, ge1);
    gp = ge0 + ge1;
  }
  const bool lo_end = 2.0 * (ghat - gm) <= a.drop, hi_end = 2.0 * (ghat - gp) <= a.drop;
  // a profile view per end: a site whose end is fixed computes along with its wave and must not take a status from roots it never wanted
  const bool run_lo = run && want_ci && !lo_end, run_hi = run && want_ci && !hi_end;
  const DfProfile<Pair> prof_lo{pair, run_lo, a.max_iter, a.tol, false}, prof_hi{pair, run_hi, a.max_iter, a.tol, false};
  st_solve<1>(prof_lo, run_lo, -1.0, delta, ghat, a.drop, a.max_iter, a.tol, xlo, ev, nclo);
  st_solve<2>(prof_hi, run_hi, delta, 1.0, ghat, a.drop, a.max_iter, a.tol, xhi, ev, nchi);
  if (have && lead) {
    const nmod_diff_out& o = a.out;
    if (!run) {
      df_write_nan(o, pos, n0, n1, too_few ? NMOD_DIFF_TOO_FEW : NMOD_DIFF_FLAT);
    } else {
      if (o.pi0) o.pi0[pos] = pi0;
      if (o.pi1) o.pi1[pos] = pi1;
      if (o.pi_pool) o.pi_pool[pos] = pip;
      if (o.delta) o.delta[pos] = delta;
      if (o.delta_lo) o.delta_lo[pos] = lo_end ? -1.0 : xlo;
      if (o.delta_hi) o.delta_hi[pos] = hi_end ? 1.0 : xhi;
      if (o.stat) o.stat[pos] = stat;
      if (o.p_diff) o.p_diff[pos] = stat;                     // (df_tail_kernel turns it into the tail)
      if (o.n_valid0) o.n_valid0[pos] = n0;
      if (o.n_valid1) o.n_valid1[pos] = n1;
      if (o.iters) o.iters[pos] = iters;
      if (o.status) o.status[pos] = (uint8_t)((nc0 || nc1 || ncp || nclo || nchi || prof_lo.nc || prof_hi.nc ? NMOD_DIFF_NOT_CONVERGED : 0) |
                                              (pip == 0.0 || pip == 1.0 ? NMOD_DIFF_POOL_AT_END : 0));
    }
  }
}

// two waves per SIMD: the register budget of K14's forms
template <int G>
__global__ __launch_bounds__(kDfThreads, 2) void df_reg_kernel(DfArgs a) {
  const int gl = threadIdx.x & (G - 1);
  for (GroupWalk<G == 16 ? 0 : 1, G, kDfThreads> it(a.pl); it.more(); it.next()) {
    const bool have = it.have();
    int64_t pos = 0, b0 = 0, m0 = 0, b1 = 0, m1 = 0;
    if (have) {
      pos = it.pos();
      csr_row(a.off0, a.stride0, pos, b0, m0);
      csr_row(a.off1, a.stride1, pos, b1, m1);
    }
    const int ny0 = (int)m0, ny1 = (int)m1;
    DfRegPair<G> pair;
    double c0 = 0.0, T0 = 0.0, c1 = 0.0, T1 = 0.0;
#pragma unroll
    for (int j = 0; j < kDfPer; ++j) {
      const int idx = gl + G * j;
      const double s0 = idx < ny0 ? a.score0[b0 + idx] : nan_f64();
      const double s1 = idx < ny1 ? a.score1[b1 + idx] : nan_f64();
      pair.w0[j] = st_signed_t(s0);
      pair.w1[j] = st_signed_t(s1);
      c0 += st_valid(s0) ? 1.0 : 0.0;
      c1 += st_valid(s1) ? 1.0 : 0.0;
      T0 += fabs(pair.w0[j]);
      T1 += fabs(pair.w1[j]);
    }
    c0 = group_sum_f64<G>(c0); T0 = group_sum_f64<G>(T0);   // (counts of up to 512 ones: exact)
    c1 = group_sum_f64<G>(c1); T1 = group_sum_f64<G>(T1);
    df_estimate(a, pair, have, gl == 0, pos, c0, T0, c1, T1);
  }
}

__global__ __launch_bounds__(kStBlockThreads) void df_block_kernel(DfArgs a) {
  __shared__ double stage[kDfStage];
  __shared__ double sh[kStBlockWaves];
  const int tid = threadIdx.x;
  for (BlockWalk<2> it(a.pl); it.more(); it.next()) {
    const int64_t pos = it.pos();
    int64_t b0, m0, b1, m1;
    csr_row(a.off0, a.stride0, pos, b0, m0);
    csr_row(a.off1, a.stride1, pos, b1, m1);
    const double *sc0 = a.score0 + b0, *sc1 = a.score1 + b1;
    const bool staged = m0 + m1 <= kDfStage;
    double c0 = 0.0, T0 = 0.0, c1 = 0.0, T1 = 0.0;
#pragma unroll 1
    for (int64_t i = tid; i < m0; i += kStBlockThreads) {
      const double s = sc0[i], wt = st_signed_t(s);
      if (staged) stage[i] = wt;                            // read back by this thread alone
      c0 += st_valid(s) ? 1.0 : 0.0;
      T0 += fabs(wt);
    }
#pragma unroll 1
    for (int64_t i = tid; i < m1; i += kStBlockThreads) {
      const double s = sc1[i], wt = st_signed_t(s);
      if (staged) stage[m0 + i] = wt;
      c1 += st_valid(s) ? 1.0 : 0.0;
      T1 += fabs(wt);
    }
    c0 = block_sum_f64<kStBlockWaves>(c0, sh); T0 = block_sum_f64<kStBlockWaves>(T0, sh);   // (counts of up to 2^24 ones: exact)
    c1 = block_sum_f64<kStBlockWaves>(c1, sh); T1 = block_sum_f64<kStBlockWaves>(T1, sh);
    const DfBlockPair pair{sc0, m0, sc1, m1, stage, sh, staged};
    df_estimate(a, pair, true, tid == 0, pos, c0, T0, c1, T1);
  }
}

// p_diff from the stat the kernels above left in its place (NaN stays NaN): the tail functions stay out of the iterating kernels
__global__ __launch_bounds__(256) void df_tail_kernel(double* p_diff, int64_t npos) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npos; i += (int64_t)gridDim.x * 256) {
    const double stat = p_diff[i];
    if (stat == stat) p_diff[i] = fmax(erfc(sqrt(0.5 * stat)), kDblMin);
  }
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_site_diff(const nmod_params* prm, int64_t npos, const double* score0, const int64_t* off0, const double* score1,
                              const int64_t* off1, const nmod_diff_opts* opts, const nmod_diff_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_diff_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_diff_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->max_iter < 1 || opts->max_iter > 200 || opts->min_valid < 1) return NMOD_ERR_INVALID_ARG;
  if (!(opts->tol >= 0.0) || !(opts->tol <= kDblMax) || !(opts->ci_drop > 0.0) || !(opts->ci_drop <= kDblMax)) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > (int64_t)INT32_MAX - 1) return NMOD_ERR_INVALID_ARG;
  if ((!off0 && prm->stride0 <= 0) || (!off1 && prm->stride1 <= 0)) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && (!score0 || !score1)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && off1 && npos > 0 && !csr_offsets_ok(off1, npos)) return NMOD_ERR_INVALID_ARG;
  int num_cus = 0;
  const int rc = rows_begin(prm, npos, off0, &num_cus);
  if (rc != NMOD_OK || npos == 0) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t np = (size_t)npos;
  const size_t tot0 = !host ? 0 : (off0 ? (size_t)off0[npos] : np * (size_t)prm->stride0);
  const size_t tot1 = !host ? 0 : (off1 ? (size_t)off1[npos] : np * (size_t)prm->stride1);

  DfArgs a;
  memset(&a, 0, sizeof(a));
  a.score0 = score0; a.off0 = off0; a.stride0 = off0 ? 0 : prm->stride0;
  a.score1 = score1; a.off1 = off1; a.stride1 = off1 ? 0 : prm->stride1;
  a.npos = npos;
  a.max_iter = opts->max_iter; a.min_valid = opts->min_valid; a.tol = opts->tol; a.drop = opts->ci_drop;
  a.out = *out;

  // one slab: the three work lists and their count words; for the host entry the inputs and outputs as well
  Slab slab(host);
  const PosListSpace<3> lists(slab, np);
  slab.in(a.off0, (np + 1) * 8); slab.in(a.score0, tot0 * 8);
  slab.in(a.off1, (np + 1) * 8); slab.in(a.score1, tot1 * 8);
  slab.out(a.out.pi0, np * 8); slab.out(a.out.pi1, np * 8); slab.out(a.out.pi_pool, np * 8); slab.out(a.out.delta, np * 8);
  slab.out(a.out.delta_lo, np * 8); slab.out(a.out.delta_hi, np * 8); slab.out(a.out.stat, np * 8); slab.out(a.out.p_diff, np * 8);
  slab.out(a.out.n_valid0, np * 4); slab.out(a.out.n_valid1, np * 4); slab.out(a.out.iters, np * 4); slab.out(a.out.status, np);
  NMOD_HIP(slab.commit(stream, prm->device));
  NMOD_HIP(lists.fill<DfRule>(slab, a, num_cus, stream));
  launch_groups<16, kDfThreads>(df_reg_kernel<16>, a, num_cus, stream);
  launch_groups<64, kDfThreads>(df_reg_kernel<64>, a, num_cus, stream);
  launch_blocks<kStBlockThreads>(df_block_kernel, a, num_cus, stream);
  if (a.out.p_diff)
    hipLaunchKernelGGL(df_tail_kernel, dim3(persistent_grid(npos, 256, (int64_t)num_cus * 16)), dim3(256), 0, stream, a.out.p_diff, npos);
  return launches_end(slab, stream);
}
