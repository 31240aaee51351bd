// What the kernels over two resident rows of window sums per site share (K15 nmod_site_diff, K24 nmod_site_diff_rep): the class steps,
// the pair policies of the register and the workgroup forms, and the views that hand one row, the sum of the two at (x, x + delta)
// or the profile over delta to K14's st_solve (stoich_rows.hpp).  A pair policy evaluates both rows at (pi0, pi1), each row's sums
// reduced on their own.  Every sum is a fixed-order chain per lane followed by a fixed-order lane / wave / LDS reduction, no float
// atomics.  The units are compiled with contraction off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nanomod_hip.h"
#include "special_math.hpp"
#include "stoich_rows.hpp"

namespace nmod {

constexpr int kDfPer = 8;                         // signed t values of each row a lane keeps
constexpr int kDfSmall = 16 * kDfPer;             // longest row of the 16-lane form
constexpr int kDfWave = 64 * kDfPer;              // longest row of the whole-wave form
static_assert(kDfSmall == NMOD_DIFF_SMALL && kDfWave == NMOD_DIFF_WAVE, "the class steps the header names");
constexpr int kDfThreads = 256;
constexpr int kDfStage = 6144;                    // signed t values of both rows together the workgroup form keeps in LDS (K14's 48 KiB)

// pi1 of the pair at (x, x + delta): inside [0, 1] whatever the last bit of the sum
__device__ __forceinline__ double df_shift(double x, double delta) { return fmin(fmax(x + delta, 0.0), 1.0); }

// Two rows in the registers of a group of G lanes: lane g keeps the scores g + G j, j < 8, of each.
template <int G>
struct DfRegPair {
  double w0[kDfPer], w1[kDfPer];
  static constexpr bool kAgain = false;
  static __device__ __forceinline__ bool any(bool f) { return __any(f); }
  template <bool WANT_G>
  __device__ __forceinline__ void eval2(double p0, double p1, double& S0, double& X0, double& S1, double& X1) const {
    const double q0 = 1.0 - p0, q1 = 1.0 - p1;
    double s0 = 0.0, x0 = 0.0, s1 = 0.0, x1 = 0.0;
#pragma unroll
    for (int j = 0; j < kDfPer; ++j) st_term<WANT_G>(w0[j], q0, p0, s0, x0);
#pragma unroll
    for (int j = 0; j < kDfPer; ++j) st_term<WANT_G>(w1[j], q1, p1, s1, x1);
    S0 = group_sum_f64<G>(s0); X0 = group_sum_f64<G>(x0);
    S1 = group_sum_f64<G>(s1); X1 = group_sum_f64<G>(x1);
  }
};

// Two rows of a workgroup: thread t takes the scores t + 512 j of each, from the stage (row 1 behind row 0) or from the scores again.
// (The loops are not unrolled: the nested iterations around them keep enough alive that an unrolled body spills.)
struct DfBlockPair {
  const double* sc0; int64_t n0; const double* sc1; int64_t n1; const double* stage; double* sh; bool staged;
  static constexpr bool kAgain = true;
  static __device__ __forceinline__ bool any(bool f) { return f; }
  template <bool WANT_G>
  __device__ __forceinline__ void eval2(double p0, double p1, double& S0, double& X0, double& S1, double& X1) const {
    const double q0 = 1.0 - p0, q1 = 1.0 - p1;
    double s0 = 0.0, x0 = 0.0, s1 = 0.0, x1 = 0.0;
#pragma unroll 1
    for (int64_t i = threadIdx.x; i < n0; i += kStBlockThreads) st_term<WANT_G>(staged ? stage[i] : st_signed_t(sc0[i]), q0, p0, s0, x0);
#pragma unroll 1
    for (int64_t i = threadIdx.x; i < n1; i += kStBlockThreads) st_term<WANT_G>(staged ? stage[n0 + i] : st_signed_t(sc1[i]), q1, p1, s1, x1);
    S0 = block_sum_f64<kStBlockWaves>(s0, sh); X0 = block_sum_f64<kStBlockWaves>(x0, sh);
    S1 = block_sum_f64<kStBlockWaves>(s1, sh); X1 = block_sum_f64<kStBlockWaves>(x1, sh);
  }
};

// What st_solve iterates over.  ROW 0 / 1: that row alone; 2: the sum of both at (x, x + delta) — delta = 0: the pooled problem.
template <int ROW, class Pair>
struct DfView {
  const Pair& p; double delta;
  static __device__ __forceinline__ bool any(bool f) { return Pair::any(f); }
  template <bool WANT_G>
  __device__ __forceinline__ void eval(double x, double& S, double& X) const {
    double S0, X0, S1, X1;
    p.template eval2<WANT_G>(x, ROW == 2 ? df_shift(x, delta) : x, S0, X0, S1, X1);
    if constexpr (ROW == 0) { S = S0; X = X0; }
    else if constexpr (ROW == 1) { S = S1; X = X1; }
    else { S = S0 + S1; X = X0 + X1; }
  }
};

// The profile h(delta) = max over pi in I(delta) of g0(pi) + g1(pi + delta) as st_solve's "g", its envelope slope S1(pi* + delta) as
// "S" (NaN where pi* is an end of I(delta): st_solve's Newton point is then no point of the bracket and it bisects).
template <class Pair>
struct DfProfile {
  const Pair& p; bool run; int max_iter; double tol; mutable bool nc;
  static __device__ __forceinline__ bool any(bool f) { return Pair::any(f); }
  template <bool WANT_G>
  __device__ __forceinline__ void eval(double d, double& S, double& X) const {
    const double lo = fmax(0.0, -d), hi = fmin(1.0, 1.0 - d);
    const DfView<2, Pair> joint{p, d};
    double Sl, Dl, Sh, Dh;
    joint.template eval<false>(lo, Sl, Dl);
    joint.template eval<false>(hi, Sh, Dh);
    const bool atlo = Sl <= 0.0, athi = !atlo && Sh >= 0.0;
    double x; int ev; bool c;
    st_solve<0>(joint, run && !atlo && !athi, lo, hi, 0.0, 0.0, max_iter, tol, x, ev, c);
    nc = nc || c;
    const double ps = atlo ? lo : (athi ? hi : x);
    double S0, g0, S1, g1;
    p.template eval2<true>(ps, df_shift(ps, d), S0, g0, S1, g1);
    X = g0 + g1;
    S = atlo || athi ? nan_f64() : S1;
  }
};

}  // namespace nmod
