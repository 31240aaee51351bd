// K2 (finalize) and K3 (window combine): one thread per genomic position, fp64.
//
// K2 turns K1's exact integers / moments into the (stat, p) pairs getKStest
// returns (myDetect.py:327-343,363) following the scipy 1.2.1 formulas
// (SURVEY.md §8a rows A1-A3).  K3 restates get_combin_pvalue
// (myDetect.py:379-414) over the whole KS track.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "special_math.hpp"
#include "../../include/nanomod_hip.h"

namespace nmod {

struct FinalizeArgs {
  int64_t npos;
  const int64_t* off0; const int64_t* off1;
  int64_t stride0, stride1;
  const uint32_t* ks_num; const uint64_t* mwu_s; const uint64_t* tie; const double* moments;
  const double* ks_d_ref;               // non-null in all-tests mode: the reference's float form of D
  int32_t tests; int32_t want_mstd;
  int64_t max_n0, max_n1;               // per-group limits of this launch
  int64_t min_cap;                      // KS-only: capacity limit of the smaller (sorted) group, else 0
  const uint8_t* nonfinite;             // [npos] or null: 1 where nonfinite_scan_kernel found a NaN / infinite sample (NMOD_FLAG_CHECK_FINITE)
  int64_t deep_lim0, deep_lim1;         // NMOD_FLAG_DEEP: a position with a group beyond NMOD_MAX_RANKED and both within these limits is
                                        // the deep form's (deep_rank.hpp writes its outputs): skipped here.  0: no deep form in this batch
  double ks_scale;                      // fixed strides: en + 0.12 + 0.11/en of ks_2samp, the same for every position (ks_size_scale on the
                                        // host); 0 where a group is CSR and the sizes differ per position
  nmod_out out;
};

// ks_2samp's size term: en = sqrt(n0 n1 / (n0 + n1)); D is scaled by en + 0.12 + 0.11/en.  Host and device evaluate this one
// expression: a square root, two divisions and two additions, each correctly rounded on both sides and none of them next to a
// multiplication that could be contracted, so a fixed-stride batch (the host's value in FinalizeArgs) and the same rows as CSR
// (per position) agree bit for bit.
__host__ __device__ __forceinline__ double ks_size_scale(int64_t n0, int64_t n1) {
  const double prod = (double)n0 * (double)n1;
  const double en = sqrt(prod / (double)(n0 + n1));
  return en + 0.12 + 0.11 / en;
}

// K1's facts of position p in the workspace (the wave-resident, counting and large-position forms)
struct K1Facts {
  const FinalizeArgs& a; int64_t p;
  __device__ __forceinline__ double ks_d(double prod) const { return a.ks_d_ref ? a.ks_d_ref[p] : (double)a.ks_num[p] / prod; }
  __device__ __forceinline__ double mwu_s() const { return (double)a.mwu_s[p]; }
  __device__ __forceinline__ double tie() const { return (double)a.tie[p]; }
  __device__ __forceinline__ const double* moments() const { return a.moments + p * 4; }
  __device__ __forceinline__ bool nonfinite() const { return a.nonfinite && a.nonfinite[p]; }
};

// The outputs and status of one position from K1's facts (src: K1Facts, or the deep form's DeepFacts)
template <class Src>
__device__ __forceinline__ void finalize_position(const FinalizeArgs& a, int64_t p, int64_t n0, int64_t n1, bool too_large, const Src& src) {
  const double nan = __builtin_nan("");
  unsigned status = 0;
  const bool empty = (n0 <= 0 || n1 <= 0) || too_large;    // "empty": nothing was computed by K1
  if (n0 <= 0 || n1 <= 0) status |= NMOD_STATUS_EMPTY;
  if (too_large) status |= NMOD_STATUS_TOO_LARGE;
  const double dn0 = (double)n0, dn1 = (double)n1;
  const double prod = dn0 * dn1;

  if (a.tests & NMOD_TEST_KS) {
    double d = nan, pv = nan;
    if (!empty) {
      // ks_2samp (scipy 1.2.1): d = max|cdf1 - cdf2|; en = sqrt(n1*n2/float(n1+n2));
      // prob = kstwobign.sf((en + 0.12 + 0.11/en) * d)
      // KS-only mode: the exact rational, correctly rounded (<= 1 ulp from the float-CDF form)
      d = src.ks_d(prod);
      // (fixed strides: every position that is not empty has the strides for sizes, and the term is a launch constant)
      const double scale = a.ks_scale > 0.0 ? a.ks_scale : ks_size_scale(n0, n1);
      pv = kolmogorov_sf(scale * d);
    }
    if (a.out.ks_d) a.out.ks_d[p] = clamp_stat(d);
    if (a.out.ks_p) a.out.ks_p[p] = clamp_p(pv);
  }

  if (a.tests & NMOD_TEST_MWU) {
    double u = nan, pv = nan;
    if (!empty) {
      // mannwhitneyu(x, y, use_continuity=True, alternative=None) of scipy 1.2.1
      double u1 = prod - 0.5 * src.mwu_s();      // n1*n2 + n1(n1+1)/2 - sum(rank x)
      double u2 = prod - u1;
      double size = (double)(n0 + n1);
      double T = (size < 2.0) ? 1.0 : 1.0 - src.tie() / (size * size * size - size);
      if (T == 0.0) {
        status |= NMOD_STATUS_MWU_ALL_IDENTICAL;          // the reference raises here
      } else {
        double sd = sqrt(T * dn0 * dn1 * (double)(n0 + n1 + 1) / 12.0);
        double meanrank = prod / 2.0 + 0.5;
        double bigu = fmax(u1, u2);
        double z = (bigu - meanrank) / sd;
        pv = norm_sf(fabs(z));
        u = fmin(u1, u2);
      }
    }
    if (a.out.mwu_u) a.out.mwu_u[p] = clamp_stat(u);
    if (a.out.mwu_p) a.out.mwu_p[p] = clamp_p(pv);
  }

  if ((a.tests & NMOD_TEST_WELCH) || a.want_mstd) {
    const double* mo = src.moments();
    double mean0 = nan, m20 = nan, mean1 = nan, m21 = nan;
    if (!empty) { mean0 = mo[0]; m20 = mo[1]; mean1 = mo[2]; m21 = mo[3]; }
    // finite samples have finite moments: a NaN or an infinity here is one in the position's samples (NMOD_STATUS_NONFINITE)
    if (!empty && !(fabs(mean0) <= 1.7976931348623157e308 && fabs(mean1) <= 1.7976931348623157e308 &&
                    fabs(m20) <= 1.7976931348623157e308 && fabs(m21) <= 1.7976931348623157e308)) status |= NMOD_STATUS_NONFINITE;
    if (a.tests & NMOD_TEST_WELCH) {
      double t = nan, pv = nan;
      if (!empty) {
        // ttest_ind(equal_var=False): _unequal_var_ttest_denom + _ttest_finish
        // (vn = var / n with one division each, df with one: the products of the small integers are exact)
        const double e0 = dn0 - 1.0, e1 = dn1 - 1.0;
        double vn1 = m20 / (e0 * dn0), vn2 = m21 / (e1 * dn1);
        double df = (vn1 + vn2) * (vn1 + vn2) * (e0 * e1) / (vn1 * vn1 * e1 + vn2 * vn2 * e0);
        if (df != df) df = 1.0;
        double denom = sqrt(vn1 + vn2);
        t = (mean0 - mean1) / denom;
        pv = student_t_two_sided(t, df);
      }
      if (pv != pv) status |= NMOD_STATUS_T_NAN;
      if (a.out.t_t) a.out.t_t[p] = clamp_stat(t);
      if (a.out.t_p) a.out.t_p[p] = clamp_p(pv);
    }
    if (a.want_mstd) {
      if (a.out.mean0) a.out.mean0[p] = mean0;
      if (a.out.std0) a.out.std0[p] = sqrt(m20 / dn0);      // np.std, ddof = 0
      if (a.out.mean1) a.out.mean1[p] = mean1;
      if (a.out.std1) a.out.std1[p] = sqrt(m21 / dn1);
    }
  }
  if (!empty && src.nonfinite()) status |= NMOD_STATUS_NONFINITE;
  if (a.out.status) a.out.status[p] = (uint8_t)status;
}

__global__ __launch_bounds__(256) void finalize_kernel(FinalizeArgs a) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= a.npos) return;
  const int64_t n0 = a.stride0 > 0 ? a.stride0 : a.off0[p + 1] - a.off0[p];
  const int64_t n1 = a.stride1 > 0 ? a.stride1 : a.off1[p + 1] - a.off1[p];
  if (a.deep_lim0 > 0 && n0 > 0 && n1 > 0 && (n0 > NMOD_MAX_RANKED || n1 > NMOD_MAX_RANKED) && n0 <= a.deep_lim0 && n1 <= a.deep_lim1) return;
  const bool too_large = (n0 > a.max_n0 || n1 > a.max_n1) || (a.min_cap > 0 && (n0 < n1 ? n0 : n1) > a.min_cap);
  finalize_position(a, p, n0, n1, too_large, K1Facts{a, p});
}

// NMOD_FLAG_CHECK_FINITE: one wave per position reads both rows and flags a NaN / infinite sample (float32 or float64 rows)
struct NonfiniteArgs {
  const void* sig0; const void* sig1; const int64_t* off0; const int64_t* off1; int64_t stride0, stride1; int64_t npos; int32_t f64;
  int64_t lim0, lim1; uint8_t* flag;
};
__global__ __launch_bounds__(256) void nonfinite_scan_kernel(NonfiniteArgs a) {
  const int lane = threadIdx.x & 63;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < a.npos; p += (int64_t)gridDim.x * 4) {
    bool bad = false;
    for (int g = 0; g < 2; ++g) {
      const int64_t st = g ? a.stride1 : a.stride0;
      const int64_t* off = g ? a.off1 : a.off0;
      const int64_t o = st > 0 ? p * st : off[p];
      int64_t n = st > 0 ? st : off[p + 1] - o;
      if (n > (g ? a.lim1 : a.lim0)) n = 0;                       // (a position beyond the limits is skipped everywhere: NMOD_STATUS_TOO_LARGE)
      const void* sig = g ? a.sig1 : a.sig0;
      for (int64_t i = lane; i < n; i += 64) {
        if (a.f64) bad = bad || !(fabs(reinterpret_cast<const double*>(sig)[o + i]) <= 1.7976931348623157e308);
        else bad = bad || !(fabsf(reinterpret_cast<const float*>(sig)[o + i]) <= 3.4028234663852886e38f);
      }
    }
    const bool any = __ballot(bad) != 0ull;
    if (lane == 0) a.flag[p] = any ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------
constexpr int kCombineTile = 256;

struct CombineArgs {
  int64_t npos;
  const double* ks_d; const double* ks_p; const int32_t* run_id;
  double* comb_st; double* comb_p;
  int32_t nb; int32_t method;
  double wnorm;                         // ||w||_2
  double w[2 * NMOD_MAX_NB + 1];        // Stouffer weights, w[nb] = 100 (myDetect.py:396-400)
};

__global__ __launch_bounds__(kCombineTile) void combine_kernel(CombineArgs a) {
  // per-position transform of the KS p-value (z = isf(p) or ln p), tile + halo
  __shared__ double tr[kCombineTile + 2 * NMOD_MAX_NB];
  const int nb = a.nb;
  const int64_t tile0 = (int64_t)blockIdx.x * kCombineTile;
  const int t = threadIdx.x;
  const bool stouffer = a.method == NMOD_METHOD_STOUFFER;
  auto transform = [&](int64_t j) -> double {
    double pj = a.ks_p[j];
    return stouffer ? norm_isf(pj) : log(pj);
  };
  const int64_t p = tile0 + t;
  if (nb == 0) {                                  // myDetect.py:413: the KS tuple itself
    if (p < a.npos) { a.comb_st[p] = a.ks_d[p]; a.comb_p[p] = a.ks_p[p]; }
    return;
  }
  if (p < a.npos) tr[nb + t] = transform(p);
  if (t < 2 * nb) {
    int64_t j = (t < nb) ? tile0 - nb + t : tile0 + kCombineTile + (t - nb);
    int slot = (t < nb) ? t : kCombineTile + t;
    if (j >= 0 && j < a.npos) tr[slot] = transform(j);
  }
  __syncthreads();
  if (p >= a.npos) return;
  const int32_t rid = a.run_id[p];
  // window = [p_KS[j] if usable else 1.0]  (myDetect.py:383-389); isf(1) = -inf, ln(1) = 0
  const double pad = stouffer ? -__builtin_inf() : 0.0;
  double acc = 0.0;
  for (int k = -nb; k <= nb; ++k) {
    int64_t j = p + k;
    bool ok = (j >= 0) && (j < a.npos);
    if (ok) ok = (a.run_id[j] == rid);
    double v = ok ? tr[nb + t + k] : pad;
    acc += stouffer ? a.w[nb + k] * v : v;
  }
  double st, pv;
  if (stouffer) {
    st = acc / a.wnorm;                 // Z = dot(w, Zi) / ||w||
    pv = norm_sf(st);
  } else {
    st = -2.0 * acc;                    // Xsq = -2 sum(log p)
    pv = chi2_sf_even(st, 2 * nb + 1);
  }
  a.comb_p[p] = clamp_p(pv);
  a.comb_st[p] = clamp_stat(st);
}

}  // namespace nmod
