// What the kernels over rows of window sums share (K14 nmod_site_stoich, K15 nmod_site_diff, K18 nmod_pair_linkage): whether a score is
// valid, its signed t, one score's terms of an evaluation, K14's two row policies and the bracketed iteration of include/nanomod_hip.h.  The units are
// compiled with contraction off; every operation here is the header's, in its order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "entry_device.hpp"
#include "special_math.hpp"

namespace nmod {

constexpr int kStPer = 16;                        // signed t values a lane keeps
constexpr int kStBlockThreads = 512;
constexpr int kStBlockWaves = kStBlockThreads / 64;

__device__ __forceinline__ bool st_valid(double s) { return fabs(s) <= kDblMax; }

// t = -expm1(-|s|) with the side of s as its sign; 0 for an invalid score, which then adds nothing to any sum
__device__ __forceinline__ double st_signed_t(double s) {
  if (!st_valid(s)) return 0.0;
  const double t = -expm1(-fabs(s));
  return s >= 0.0 ? t : -t;
}

// one score's terms of an evaluation at pi (qp = 1 - pi, qn = pi): x gathers log1p(-qt) when WANT_G, else u^2
template <bool WANT_G>
__device__ __forceinline__ void st_term(double w, double qp, double qn, double& s, double& x) {
  const double t = fabs(w);
  const bool plus = w >= 0.0;
  const double qt = (plus ? qp : qn) * t;
  const double u = t / (1.0 - qt);
  s += plus ? u : -u;
  if constexpr (WANT_G) x += log1p(-qt); else x += u * u;
}

// A row in the registers of a group of G lanes, lane g of it keeps the scores g + G j, j < 16.  Reached with all lanes on (a group
// without a row, or a finished one, computes and does not commit), so the DPP sums always see a full row.
template <int G>
struct StRegRow {
  double w[kStPer];
  static __device__ __forceinline__ bool any(bool f) { return __any(f); }
  template <bool WANT_G>
  __device__ __forceinline__ void eval(double pi, double& S, double& X) const {
    const double qp = 1.0 - pi;
    double s = 0.0, x = 0.0;
#pragma unroll
    for (int j = 0; j < kStPer; ++j) st_term<WANT_G>(w[j], qp, pi, s, x);
    S = group_sum_f64<G>(s);
    X = group_sum_f64<G>(x);
  }
};

// A row of a workgroup: thread t takes the scores t + 512 j, from the stage in LDS or, for a row beyond it, from the scores again.
// Everything a decision rests on is a block sum, the same bits in every thread: the control flow is uniform over the workgroup.
struct StBlockRow {
  const double* score; int64_t n; const double* stage; double* sh; bool staged;
  static __device__ __forceinline__ bool any(bool f) { return f; }
  template <bool WANT_G>
  __device__ __forceinline__ void eval(double pi, double& S, double& X) const {
    const double qp = 1.0 - pi;
    double s = 0.0, x = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kStBlockThreads) st_term<WANT_G>(staged ? stage[i] : st_signed_t(score[i]), qp, pi, s, x);
    S = block_sum_f64<kStBlockWaves>(s, sh);
    X = block_sum_f64<kStBlockWaves>(x, sh);
  }
};

// The bracketed iteration of the header on (a, b).  MODE 0: the root of S; 1: the lower end of the interval; 2: the upper end.
// run: whether the caller's row wants this root at all; a row that does not, or has stopped, computes along and keeps its state.
template <int MODE, class Row>
__device__ __forceinline__ void st_solve(const Row& row, bool run, double a, double b, double ghat, double drop, int max_iter, double tol,
                                         double& root, int& evals, bool& not_converged) {
  double x = a + 0.5 * (b - a);
  bool active = run;
  evals = 0;
  for (int k = 1; k <= max_iter; ++k) {
    if (!Row::any(active)) break;
    double S, X;
    row.template eval<MODE != 0>(x, S, X);
    bool right;
    double xn;
    if constexpr (MODE == 0) {
      right = S > 0.0;
      xn = x + S / X;
    } else {
      const double h = 2.0 * (ghat - X);
      right = MODE == 1 ? h > drop : h <= drop;
      xn = x + (h - drop) / (2.0 * S);
    }
    const double na = right ? x : a, nb = right ? b : x;
    if (xn != x && !(xn > na && xn < nb)) xn = na + 0.5 * (nb - na);   // (xn == x: a step below the spacing of doubles at x; x stays)
    if (active) {
      const double step = fabs(xn - x);
      a = na; b = nb; x = xn; evals = k;
      if (tol > 0.0 && (b - a <= tol || step <= tol)) active = false;
    }
  }
  root = x;
  not_converged = active;                                   // still running when max_iter was reached
}

}  // namespace nmod
