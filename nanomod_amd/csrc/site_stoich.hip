// nmod_site_stoich — per-position modified fraction by maximum likelihood from pivoted window sums, with a likelihood interval, the
// likelihood-ratio test of pi = 0 and a posterior per read, on the device (K14).  The reference project has no such step;
// the definition is the one in include/nanomod_hip.h (tests/stoich_ref.py restates it in numpy).  K8's shape (mix_fraction.hip): a few
// fixed-point iterations over a row that stays on chip.  All on the caller's stream:
//   pos_classify_kernel<StRule>  (pos_walk.hpp) a thread per row: the row's class by its length, ballot-compacted into one list per
//                        class; a row beyond NMOD_MAX_DEEP gets its NaN outputs, status and NaN resp here
//   st_reg_kernel<16>    rows <= 256: 16 lanes x 16 signed t values hold a row in registers over all iterations, four rows per wave,
//                        DPP row sums only; a finished row freezes while the others of its wave go on
//   st_reg_kernel<64>    rows <= 1 024: the whole wave x 16 doubles
//   st_block_kernel      beyond: a workgroup per row, the signed t staged in LDS up to kStStage scores (a thread reads back only the words
//                        it wrote itself), re-read and recomputed per evaluation beyond; wave sums through LDS in index order
// t = -expm1(-|s|) is computed once at load with the side of s as its sign, so an evaluation is one fp64 division and a few adds per
// score (a log1p in their place for the interval roots).  The three roots of a row (pi^, pi_lo, pi_hi) run one after the other on the
// resident t; resp is one final pass over the scores.  The grids are persistent and read their list's length from the device: no host
// read anywhere.  Every sum is a fixed-order chain per lane followed by a fixed-order lane / wave / LDS reduction, no float atomics: a
// row's bits depend on the row alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "pos_walk.hpp"
#include "special_math.hpp"
#include "stoich_rows.hpp"

namespace nmod {

// (kStPer, the signed t values a lane keeps, and the workgroup's size: stoich_rows.hpp, with the row policies and st_solve)
constexpr int kStSmall = 16 * kStPer;             // largest row of the 16-lane form
constexpr int kStWave = 64 * kStPer;              // largest row of the whole-wave form
static_assert(kStSmall == NMOD_STOICH_SMALL && kStWave == NMOD_STOICH_WAVE, "the class steps the header names");
constexpr int kStThreads = 256;
constexpr int kStStage = 6144;                    // scores of a row the workgroup form keeps in LDS (48 KiB; tests/stoich_ref.py names it)

struct StArgs {
  const double* score; const int64_t* off; int64_t stride; int64_t npos;
  int max_iter, min_valid; double tol, drop;
  nmod_stoich_out out;
  PosLists<3> pl;                                 // per class: indices of the rows, their number
};

__device__ __forceinline__ void st_write_nan(const nmod_stoich_out& o, int64_t i, int n_valid, unsigned status) {
  const double nan = nan_f64();
  if (o.pi) o.pi[i] = nan;
  if (o.pi_lo) o.pi_lo[i] = nan;
  if (o.pi_hi) o.pi_hi[i] = nan;
  if (o.stat) o.stat[i] = nan;
  if (o.p_null) o.p_null[i] = nan;
  if (o.n_valid) o.n_valid[i] = n_valid;
  if (o.iters) o.iters[i] = 0;
  if (o.status) o.status[i] = (uint8_t)status;
}

// the class of row i by its length; a row beyond NMOD_MAX_DEEP is left out (its scores' resp: NaN, by the classify kernel)
struct StRule {
  static constexpr int NC = 3;
  using Track = double;
  static __device__ __forceinline__ double* track(const StArgs& a) { return a.out.resp; }
  static __device__ __forceinline__ int cls(const StArgs& a, int64_t i, int64_t& yb, int64_t& yn) {
    csr_row(a.off, a.stride, i, yb, yn);
    if (yn > NMOD_MAX_DEEP) { st_write_nan(a.out, i, 0, NMOD_STOICH_TOO_LARGE); return -1; }
    return yn <= kStSmall ? 0 : (yn <= kStWave ? 1 : 2);
  }
};

// Everything between a row's first sums (cnt valid scores, P = the sum of those >= 0, T = the sum of t) and its outputs; `lead`: the
// thread that writes them.  Returns whether the row has an estimate, pihat with it.
template <class Row>
__device__ __forceinline__ bool st_estimate(const StArgs& a, const Row& row, bool have, bool lead, int64_t pos, double cnt, double P, double T,
                                            double& pihat) {
  const int n = (int)cnt;
  const bool too_few = n < a.min_valid, flat = !too_few && !(T > 0.0);
  const bool run = have && !too_few && !flat;
  double S0, g0, S1, g1;
  row.template eval<true>(0.0, S0, g0);
  row.template eval<true>(1.0, S1, g1);
  const bool at0 = S0 <= 0.0, at1 = !at0 && S1 >= 0.0;
  double x, xlo, xhi;
  int iters, ev;
  bool nc0, nc1, nc2;
  st_solve<0>(row, run && !at0 && !at1, 0.0, 1.0, 0.0, 0.0, a.max_iter, a.tol, x, iters, nc0);
  pihat = at0 ? 0.0 : (at1 ? 1.0 : x);
  double Sh, gh;
  row.template eval<true>(pihat, Sh, gh);
  const double lhat = at0 ? 0.0 : fmax(gh + P, 0.0);
  const bool lo0 = 2.0 * (gh - g0) <= a.drop, hi1 = 2.0 * (gh - g1) <= a.drop;
  st_solve<1>(row, run && !lo0, 0.0, pihat, gh, a.drop, a.max_iter, a.tol, xlo, ev, nc1);
  st_solve<2>(row, run && !hi1, pihat, 1.0, gh, a.drop, a.max_iter, a.tol, xhi, ev, nc2);
  if (have && lead) {
    const nmod_stoich_out& o = a.out;
    if (!run) {
      st_write_nan(o, pos, n, too_few ? NMOD_STOICH_TOO_FEW : NMOD_STOICH_FLAT);
    } else {
      if (o.pi) o.pi[pos] = pihat;
      if (o.pi_lo) o.pi_lo[pos] = lo0 ? 0.0 : xlo;
      if (o.pi_hi) o.pi_hi[pos] = hi1 ? 1.0 : xhi;
      if (o.stat) o.stat[pos] = 2.0 * lhat;
      if (o.p_null) o.p_null[pos] = at0 ? 1.0 : fmax(0.5 * erfc(sqrt(lhat)), kDblMin);
      if (o.n_valid) o.n_valid[pos] = n;
      if (o.iters) o.iters[pos] = iters;
      if (o.status) o.status[pos] = (uint8_t)((nc0 || nc1 || nc2 ? NMOD_STOICH_NOT_CONVERGED : 0) | (at0 ? NMOD_STOICH_AT_ZERO : 0) |
                                              (at1 ? NMOD_STOICH_AT_ONE : 0));
    }
  }
  return run;
}

// the posterior of one read at pihat; est: whether its row has an estimate
__device__ __forceinline__ double st_resp(double s, double pihat, bool est) {
  if (!est || !st_valid(s)) return nan_f64();
  if (pihat == 0.0) return 0.0;
  if (pihat == 1.0) return 1.0;
  const double e = exp(-fabs(s));
  return s >= 0.0 ? pihat / (pihat + (1.0 - pihat) * e) : (pihat * e) / ((1.0 - pihat) + pihat * e);
}

template <int G>
__global__ __launch_bounds__(kStThreads) void st_reg_kernel(StArgs a) {
  const int gl = threadIdx.x & (G - 1);
  for (GroupWalk<G == 16 ? 0 : 1, G, kStThreads> it(a.pl); it.more(); it.next()) {
    const bool have = it.have();
    int64_t pos = 0, yb = 0, yn = 0;
    if (have) {
      pos = it.pos();
      csr_row(a.off, a.stride, pos, yb, yn);
    }
    const int ny = (int)yn;
    StRegRow<G> row;
    double c = 0.0, P = 0.0, T = 0.0;
#pragma unroll
    for (int j = 0; j < kStPer; ++j) {
      const int idx = gl + G * j;
      const double s = idx < ny ? a.score[yb + idx] : nan_f64();
      const bool valid = st_valid(s);
      row.w[j] = st_signed_t(s);
      c += valid ? 1.0 : 0.0;
      P += valid && s >= 0.0 ? s : 0.0;
      T += fabs(row.w[j]);
    }
    c = group_sum_f64<G>(c);                                // (a count of up to 1 024 ones: exact)
    P = group_sum_f64<G>(P);
    T = group_sum_f64<G>(T);
    double pihat;
    const bool est = st_estimate(a, row, have, gl == 0, pos, c, P, T, pihat);
    if (a.out.resp && have) {
#pragma unroll
      for (int j = 0; j < kStPer; ++j) {
        const int idx = gl + G * j;
        if (idx < ny) a.out.resp[yb + idx] = st_resp(a.score[yb + idx], pihat, est);
      }
    }
  }
}

__global__ __launch_bounds__(kStBlockThreads) void st_block_kernel(StArgs a) {
  __shared__ double stage[kStStage];
  __shared__ double sh[kStBlockWaves];
  const int tid = threadIdx.x;
  for (BlockWalk<2> it(a.pl); it.more(); it.next()) {
    const int64_t pos = it.pos();
    int64_t yb, yn;
    csr_row(a.off, a.stride, pos, yb, yn);
    const double* sc = a.score + yb;
    const bool staged = yn <= kStStage;
    double c = 0.0, P = 0.0, T = 0.0;
    for (int64_t i = tid; i < yn; i += kStBlockThreads) {
      const double s = sc[i];
      const bool valid = st_valid(s);
      const double wt = st_signed_t(s);
      if (staged) stage[i] = wt;                            // read back by this thread alone
      c += valid ? 1.0 : 0.0;
      P += valid && s >= 0.0 ? s : 0.0;
      T += fabs(wt);
    }
    c = block_sum_f64<kStBlockWaves>(c, sh);                // (a count of up to 2^24 ones: exact)
    P = block_sum_f64<kStBlockWaves>(P, sh);
    T = block_sum_f64<kStBlockWaves>(T, sh);
    const StBlockRow row{sc, yn, stage, sh, staged};
    double pihat;
    const bool est = st_estimate(a, row, true, tid == 0, pos, c, P, T, pihat);
    if (a.out.resp)
      for (int64_t i = tid; i < yn; i += kStBlockThreads) a.out.resp[yb + i] = st_resp(sc[i], pihat, est);
  }
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_site_stoich(const nmod_params* prm, int64_t npos, const double* score, const int64_t* off,
                                const nmod_stoich_opts* opts, const nmod_stoich_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_stoich_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_stoich_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->max_iter < 1 || opts->max_iter > 200 || opts->min_valid < 1) return NMOD_ERR_INVALID_ARG;
  if (!(opts->tol >= 0.0) || !(opts->tol <= kDblMax) || !(opts->ci_drop > 0.0) || !(opts->ci_drop <= kDblMax)) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > (int64_t)INT32_MAX - 1) return NMOD_ERR_INVALID_ARG;
  if (!off && prm->stride0 <= 0) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && !score) return NMOD_ERR_INVALID_ARG;
  int num_cus = 0;
  const int rc = rows_begin(prm, npos, off, &num_cus);
  if (rc != NMOD_OK || npos == 0) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  const size_t np = (size_t)npos;
  const size_t tot = !host ? 0 : (off ? (size_t)off[npos] : np * (size_t)prm->stride0);

  StArgs a;
  memset(&a, 0, sizeof(a));
  a.score = score; a.off = off; a.stride = off ? 0 : prm->stride0; a.npos = npos;
  a.max_iter = opts->max_iter; a.min_valid = opts->min_valid; a.tol = opts->tol; a.drop = opts->ci_drop;
  a.out = *out;

  // one slab: the three work lists and their count words; for the host entry the inputs and outputs as well
  Slab slab(host);
  const PosListSpace<3> lists(slab, np);
  slab.in(a.off, (np + 1) * 8); slab.in(a.score, tot * 8);
  slab.out(a.out.pi, np * 8); slab.out(a.out.pi_lo, np * 8); slab.out(a.out.pi_hi, np * 8); slab.out(a.out.stat, np * 8);
  slab.out(a.out.p_null, np * 8); slab.out(a.out.n_valid, np * 4); slab.out(a.out.iters, np * 4); slab.out(a.out.status, np);
  slab.out(a.out.resp, tot * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  NMOD_HIP(lists.fill<StRule>(slab, a, num_cus, stream));
  launch_groups<16, kStThreads>(st_reg_kernel<16>, a, num_cus, stream);
  launch_groups<64, kStThreads>(st_reg_kernel<64>, a, num_cus, stream);
  launch_blocks<kStBlockThreads>(st_block_kernel, a, num_cus, stream);
  return launches_end(slab, stream);
}
