// fp64 tail functions for the p-values of the per-base tests (device side).
//
// Each function states the scipy 1.2.1 primitive it stands for (the reference
// reaches them through scipy.stats at myDetect.py:331,335,341,393,401).  They
// are written for gfx950 only (ocml exp/log/erfc/lgamma/log1p in fp64);
// relative accuracy target 1e-12 down to p = DBL_MIN.
#pragma once
#include <hip/hip_runtime.h>

namespace nmod {

constexpr double kDblMin = 2.2250738585072014e-308;
constexpr double kDblMax = 1.7976931348623157e+308;
constexpr double kSqrt2Pi = 2.5066282746310002;
constexpr double kInvSqrt2 = 0.70710678118654752;

// m_min_float / m_max_float (myDetect.py:317-325); NaN passes through both.
__device__ __forceinline__ double clamp_p(double p) { return (p < kDblMin) ? kDblMin : p; }
__device__ __forceinline__ double clamp_stat(double s) { return (s > kDblMax) ? kDblMax : s; }

// kstwobign.sf == scipy.special.kolmogorov: Q(x) = 2 sum_{k>=1} (-1)^(k-1) exp(-2 k^2 x^2).
// Small x uses the theta-function dual 1 - sqrt(2 pi)/x sum exp(-(2k-1)^2 pi^2/(8 x^2)),
// which is what keeps the value accurate where the alternating series cancels.
// Every term of either series is a power of one exponential, e^(1, 9, 25, 49) with e = exp(-pi^2/(8 x^2)) and
// e^(k^2) with e = exp(-2 x^2): one exp per branch, the powers by multiplication (a wave of positions on both sides
// of 0.82 runs both branches — twelve calls of exp before, two now).  A power e^n carries n times the rounding of e,
// against a term that is e^(n-1) times smaller than the first: 5.6e-14 against mpmath over 0.2 <= x <= 18, the same
// as with one exp per term (the rounding of x itself dominates both; tests/test_tail_math_host.py).
__device__ inline double kolmogorov_sf(double x) {
  if (!(x > 0.0)) return (x != x) ? x : 1.0;
  if (x < 0.82) {
    const double pi2_8 = 1.2337005501361697;  // pi^2/8
    double w = pi2_8 / (x * x);
    const double e = exp(-w);
    const double e2 = e * e, e4 = e2 * e2, e8 = e4 * e4, e9 = e8 * e;
    const double e16 = e8 * e8, e24 = e16 * e8, e25 = e24 * e;
    const double e48 = e24 * e24, e49 = e48 * e;
    double s = e + e9 + e25 + e49;
    return 1.0 - kSqrt2Pi / x * s;
  }
  const double e = exp(-2.0 * x * x), e2 = e * e;
  double t = e, r = e2 * e;                    // t_k = e^(k^2), r_k = e^(2k+1) = t_(k+1) / t_k
  double s = 0.0, sign = 1.0;
#pragma unroll 1
  for (int k = 1; k <= 8; ++k) {
    s += sign * t;
    sign = -sign;
    if (t < 1e-18 * s) break;
    t *= r;
    r *= e2;
  }
  return 2.0 * s;
}

// norm.sf(z) = ndtr(-z)
__device__ __forceinline__ double norm_sf(double z) { return 0.5 * erfc(z * kInvSqrt2); }

// norm.isf(p) = -ndtri(p).  Wichura's AS241, routine PPND16 (Applied Statistics 37 (1988) 477-484): three pairs of
// degree-7 polynomials, on 0.425^2 - (q - 1/2)^2 for 0.075 <= q <= 0.5 and on r = sqrt(-log q) below (r <= 5 and
// 5 < r <= 27; r = 26.62 at q = DBL_MIN), one division for all of them.  Against mpmath from DBL_MIN to 0.5: 8e-16
// relative in z (tests/test_tail_math_host.py).  (Acklam's approximation with a Newton step through erfcx stood
// here before: 7e-13, with two logarithms, erfcx, a square root and a division for every p.)
// Every coefficient is positive and so is every argument (0.5 - q, r, r - 1.6, r - 5): the unflipped half cannot
// come out negative, and z = +0 exactly at p = 0.5.
__device__ inline double norm_isf(double p) {
  if (p != p) return p;
  if (p <= 0.0) return __builtin_inf();
  if (p >= 1.0) return -__builtin_inf();
  const bool flip = p > 0.5;
  const double q = flip ? 1.0 - p : p;          // exact for p in (0.5, 1)
  double num, den;
  if (q >= 0.075) {
    const double c = 0.5 - q, r = 0.180625 - c * c;
    num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r
              + 4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r
              + 1.3314166789178437745e+2) * r + 3.387132872796366608) * c;
    den = ((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r
              + 2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r
              + 4.2313330701600911252e+1) * r + 1.0;
  } else {
    double r = sqrt(-log(q));
    if (r <= 5.0) {
      r -= 1.6;
      num = ((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r
               + 1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.76949722146069140550) * r
               + 4.63033784615654529590) * r + 1.42343711074968357734;
      den = ((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r
               + 1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940) * r
               + 2.05319162663775882187) * r + 1.0;
    } else {
      r -= 5.0;
      num = ((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r
               + 2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580) * r
               + 5.46378491116411436990) * r + 6.65790464350110377720;
      den = ((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r
               + 7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r
               + 5.99832206555887937690e-1) * r + 1.0;
    }
  }
  const double z = num / den;
  return flip ? -z : z;
}

// log B(a, 1/2) without the lgamma cancellation: shift a up to z >= 16 with the recurrence, then the asymptotic series
//   lgamma(z + 1/2) - lgamma(z) = 1/2 ln z + sum_{n even} (2^(1-n) - 2) B_n / (n (n - 1) z^(n-1))
//                               = 1/2 ln z - 1/(8 z) + 1/(192 z^3) - 1/(640 z^5) + 17/(14336 z^7) - 31/(18432 z^9) + 691/(180224 z^11)
// (next term 3e-18 at z = 16; against mpmath's log(beta(a, 1/2)) on 0.5 <= a <= 1e7: 7.3e-16 absolute).  One division
// and one logarithm; the Stirling-difference form before it took four divisions, log1p and two logarithms.
__device__ inline double lbeta_half(double a) {
  double ratio = 1.0;                     // prod (a+i)/(a+i+1/2)
  double z = a;
  bool shifted = false;
#pragma unroll 1
  while (z < 16.0) { ratio *= z / (z + 0.5); z += 1.0; shifted = true; }
  const double r = 1.0 / z, r2 = r * r;
  const double d = 0.5 * log(z) + r * (-1.0 / 8.0 + r2 * (1.0 / 192.0 + r2 * (-1.0 / 640.0 + r2 * (17.0 / 14336.0
                   + r2 * (-31.0 / 18432.0 + r2 * (691.0 / 180224.0))))));
  // lgamma(a+1/2) - lgamma(a) = d + log(ratio)
  double lr = 0.0;
  if (__ballot(shifted) != 0ull) lr = log(ratio);
  return 0.57236494292470009 /* log(pi)/2 */ - d - lr;
}

// Continued fraction of the regularised incomplete beta, 1/(1 + d_1/(1 + d_2/(1 + ...))) with
//   d_{2m+1} = -(a+m)(a+b+m) x / ((a+2m)(a+2m+1)),   d_{2m} = m (b-m) x / ((a+2m-1)(a+2m)).
// Evaluated by the forward (Wallis) recurrence on an equivalent fraction without divisions: with d_k = n_k/e_k
// and c_k = e_k rho_k, rho_k any approximation of 1/e_k (v_rcp_f64), the fraction with partial numerators
// rho_k c_{k-1} n_k and partial denominators c_k has the same convergents and stays O(1) in magnitude.
// (The modified-Lentz form costs six fp64 divisions per m; this one none: finalize_kernel 1.0 -> 0.4 ms.)
__device__ inline double betacf(double a, double b, double x) {
  const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
  double A0 = 0.0, B0 = 1.0, A1 = 1.0, B1 = 1.0, cprev = 1.0;
  auto step = [&](double n, double e) {
    const double rho = __builtin_amdgcn_rcp(e);
    const double c = e * rho;
    const double t = rho * cprev * n;
    const double A2 = c * A1 + t * A0, B2 = c * B1 + t * B0;
    A0 = A1; B0 = B1; A1 = A2; B1 = B2; cprev = c;
  };
  step(-qab * x, qap);                                            // d_1
#pragma unroll 1
  for (int m = 1; m <= 2000; ++m) {
    const double dm = (double)m, m2 = 2.0 * dm;
    step(dm * (b - dm) * x, (qam + m2) * (a + m2));               // d_{2m}
    step(-(a + dm) * (qab + dm) * x, (a + m2) * (qap + m2));      // d_{2m+1}
    const double u = A1 * B0, v = A0 * B1;                         // successive convergents agree to 2e-16 (relative)
    if (fabs(u - v) < 2e-16 * fabs(u)) break;
    // the convergents are ratios: rescale all four terms when they drift (x near 1 with large a shrinks them by
    // ~(1 - x) per m and the fraction needs hundreds of terms)
    const double mag = fabs(B1);
    if (mag < 1e-60 || mag > 1e60) {
      const double sc = __builtin_amdgcn_rcp(fmax(mag, 1e-300));
      A0 *= sc; B0 *= sc; A1 *= sc; B1 *= sc;
    }
  }
  const double tiny = 1e-300;
  if (fabs(B1) < tiny) B1 = tiny;
  return A1 / B1;
}

// 1 / (k + 3/2), k = 0 .. 127 (correctly rounded): the coefficient ratios of the series below
__device__ __constant__ double kInvKPlus15[128] = {
  0.66666666666666663, 0.40000000000000002, 0.2857142857142857, 0.22222222222222221,
  0.18181818181818182, 0.15384615384615385, 0.13333333333333333, 0.11764705882352941,
  0.10526315789473684, 0.095238095238095233, 0.086956521739130432, 0.080000000000000002,
  0.07407407407407407, 0.068965517241379309, 0.064516129032258063, 0.060606060606060608,
  0.057142857142857141, 0.054054054054054057, 0.05128205128205128, 0.04878048780487805,
  0.046511627906976744, 0.044444444444444446, 0.042553191489361701, 0.040816326530612242,
  0.039215686274509803, 0.037735849056603772, 0.036363636363636362, 0.035087719298245612,
  0.033898305084745763, 0.032786885245901641, 0.031746031746031744, 0.030769230769230771,
  0.029850746268656716, 0.028985507246376812, 0.028169014084507043, 0.027397260273972601,
  0.026666666666666668, 0.025974025974025976, 0.025316455696202531, 0.024691358024691357,
  0.024096385542168676, 0.023529411764705882, 0.022988505747126436, 0.02247191011235955,
  0.02197802197802198, 0.021505376344086023, 0.021052631578947368, 0.020618556701030927,
  0.020202020202020204, 0.019801980198019802, 0.019417475728155338, 0.019047619047619049,
  0.018691588785046728, 0.01834862385321101, 0.018018018018018018, 0.017699115044247787,
  0.017391304347826087, 0.017094017094017096, 0.01680672268907563, 0.016528925619834711,
  0.016260162601626018, 0.016, 0.015748031496062992, 0.015503875968992248,
  0.015267175572519083, 0.015037593984962405, 0.014814814814814815, 0.014598540145985401,
  0.014388489208633094, 0.014184397163120567, 0.013986013986013986, 0.013793103448275862,
  0.013605442176870748, 0.013422818791946308, 0.013245033112582781, 0.013071895424836602,
  0.012903225806451613, 0.012738853503184714, 0.012578616352201259, 0.012422360248447204,
  0.012269938650306749, 0.012121212121212121, 0.011976047904191617, 0.011834319526627219,
  0.011695906432748537, 0.011560693641618497, 0.011428571428571429, 0.011299435028248588,
  0.0111731843575419, 0.011049723756906077, 0.01092896174863388, 0.010810810810810811,
  0.0106951871657754, 0.010582010582010581, 0.010471204188481676, 0.010362694300518135,
  0.010256410256410256, 0.01015228426395939, 0.010050251256281407, 0.0099502487562189053,
  0.009852216748768473, 0.0097560975609756097, 0.0096618357487922701, 0.0095693779904306216,
  0.0094786729857819912, 0.0093896713615023476, 0.0093023255813953487, 0.0092165898617511521,
  0.0091324200913242004, 0.0090497737556561094, 0.0089686098654708519, 0.0088888888888888889,
  0.0088105726872246704, 0.0087336244541484712, 0.008658008658008658, 0.0085836909871244635,
  0.0085106382978723406, 0.0084388185654008432, 0.008368200836820083, 0.0082987551867219917,
  0.00823045267489712, 0.0081632653061224497, 0.0080971659919028341, 0.0080321285140562242,
  0.0079681274900398405, 0.0079051383399209481, 0.0078431372549019607, 0.0077821011673151752,
};

// 2 * t.sf(|t|, df) = I_{df/(df+t^2)}(df/2, 1/2)   (ttest_ind's _ttest_finish)
__device__ inline double student_t_two_sided(double t, double df) {
  if (t != t || df != df) return __builtin_nan("");
  double t2 = t * t;
  if (t2 == 0.0) return 1.0;
  if (isinf(t2)) return 0.0;
  double a = 0.5 * df, b = 0.5;
  const double inv = 1.0 / (df + t2);     // (one division for both)
  double x = df * inv;                    // df/(df+t^2)
  double y = t2 * inv;                    // 1 - x, without cancellation
  double lnx = log1p(-y);
  double front = sqrt(y) * exp(a * lnx - lbeta_half(a));       // x^a y^(1/2) / B(a, 1/2)
  // Moderate |t| (t^2 < 9: p > 2.7e-3, so 1 - v keeps 12 digits) and y < 0.3: the hypergeometric series
  //   I_y(1/2, a) = 2 front * sum_k [(a + 1/2)_k / (3/2)_k] y^k      (DLMF 8.17.8; all terms positive)
  // whose term ratio y (a + 1/2 + k) / (3/2 + k) falls below 1/2 within a few terms: 6 fp64 operations per term against
  // ~35 per step of the continued fraction, and nearly every position of a null-like batch is in this range.
  const bool fast = t2 < 9.0 && y < 0.3;
  double p_fast = 0.0;
  bool done = false;
  if (__ballot(fast) != 0ull) {
    double term = 1.0, sum = 1.0;
    const double ah = a + 0.5;
    bool conv = false;
#pragma unroll 1
    for (int k = 0; k < 128; k += 4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        term *= y * (ah + (double)(k + j)) * kInvKPlus15[k + j];
        sum += term;
      }
      conv = !(term > 1e-17 * sum);                      // (the ratio is decreasing in k: once below this, the tail is too)
      if (__ballot(fast && !conv) == 0ull) break;
    }
    p_fast = 1.0 - 2.0 * front * sum;
    done = fast && conv;
  }
  if (__ballot(!done) == 0ull) return p_fast;
  // one call for both regimes: a wave whose lanes fall on both sides would otherwise run the fraction twice
  const bool direct = x < (a + 1.0) / (a + b + 2.0);
  const double ca = direct ? a : b, cb = direct ? b : a, cx = direct ? x : y;
  const double v = front * betacf(ca, cb, cx) / ca;
  const double p_cf = direct ? v : 1.0 - v;
  return done ? p_fast : p_cf;
}

// chi2.sf(X, 2W) = exp(-x) sum_{m<W} x^m/m!,  x = X/2   (combine_pvalues, fisher)
__device__ inline double chi2_sf_even(double X, int W) {
  double x = 0.5 * X;
  if (x != x) return x;
  if (!(x > 0.0)) return 1.0;
  if (isinf(x)) return 0.0;
  int ms = W - 1;
  if ((double)ms > x) ms = (int)x;
  double lt = -x + (double)ms * log(x) - lgamma((double)ms + 1.0);
  double t = exp(lt);
  double sum = t, tm = t;
#pragma unroll 1
  for (int m = ms; m >= 1; --m) { tm *= (double)m / x; sum += tm; if (tm < 1e-18 * sum) break; }
  tm = t;
#pragma unroll 1
  for (int m = ms + 1; m <= W - 1; ++m) { tm *= x / (double)m; sum += tm; }
  return sum > 1.0 ? 1.0 : sum;
}

// chi2.sf(X, 2M + 1) = erfc(sqrt(x)) + exp(-x) sum_{j=1..M} x^(j - 1/2) / Gamma(j + 1/2),  x = X/2   (K24's heterogeneity test at
// an odd number of degrees of freedom; M = 0: the chi2_1 tail).  The terms run down from j = M, the first through its logarithm as
// above: exp(-x) alone underflows from x = 745 on, where the tail of 13 degrees of freedom is still above DBL_MIN.
__device__ inline double chi2_sf_odd(double X, int M) {
  double x = 0.5 * X;
  if (x != x) return x;
  if (!(x > 0.0)) return 1.0;
  if (isinf(x)) return 0.0;
  double sum = erfc(sqrt(x));
  if (M >= 1) {
    double tm = exp(-x + ((double)M - 0.5) * log(x) - lgamma((double)M + 0.5));
    sum += tm;
#pragma unroll 1
    for (int j = M; j >= 2; --j) { tm *= ((double)j - 0.5) / x; sum += tm; }
  }
  return sum > 1.0 ? 1.0 : sum;
}

// ---- the polygamma functions of K25's prior fit (nmod_rep_prior: one thread; x > 0).  All three by the same method: the recurrence
// f(x) = f(x + 1) -+ n! / x^(n+1) up to z >= 16, then the asymptotic (Bernoulli) series in 1 / z^2 through B14 (next term below 1e-19
// at z = 16).  The recurrence terms are summed on their own and joined to the series once.  Measured against 50-digit mpmath on 4 000
// log-uniform points of 1e-3 <= x <= 1e8 and the half-integers 1/2 .. 7 (tests/test_site_diff_mod.py, profiles/site_diff_mod.txt):
//   digamma    1.4e-15 relative to max(1, |psi|) (it crosses 0 at 1.4616), 5.3e-16 relative from x = 4 on
//   trigamma   6.7e-16 relative
//   tetragamma 7.2e-16 relative
// psi(x) = ln z - 1/(2z) - sum_n B_2n / (2n z^2n) - sum_{k < z - x} 1 / (x + k)
__device__ inline double digamma(double x) {
  double z = x, shift = 0.0;
#pragma unroll 1
  while (z < 16.0) { shift += 1.0 / z; z += 1.0; }
  const double r = 1.0 / z, r2 = r * r;
  const double tail = r2 * (1.0 / 12.0 - r2 * (1.0 / 120.0 - r2 * (1.0 / 252.0 - r2 * (1.0 / 240.0 - r2 * (1.0 / 132.0
                      - r2 * (691.0 / 32760.0 - r2 * (1.0 / 12.0)))))));
  return log(z) - 0.5 * r - tail - shift;
}

// psi'(x) = 1/z + 1/(2 z^2) + sum_n B_2n / z^(2n+1) + sum_{k < z - x} 1 / (x + k)^2
__device__ inline double trigamma(double x) {
  double z = x, shift = 0.0;
#pragma unroll 1
  while (z < 16.0) { shift += 1.0 / (z * z); z += 1.0; }
  const double r = 1.0 / z, r2 = r * r;
  const double tail = r * r2 * (1.0 / 6.0 - r2 * (1.0 / 30.0 - r2 * (1.0 / 42.0 - r2 * (1.0 / 30.0 - r2 * (5.0 / 66.0
                      - r2 * (691.0 / 2730.0 - r2 * (7.0 / 6.0)))))));
  return r + 0.5 * r2 + tail + shift;
}

// psi''(x) = -1/z^2 - 1/z^3 - sum_n (2n + 1) B_2n / z^(2n+2) - sum_{k < z - x} 2 / (x + k)^3   (the slope of the Newton step below)
__device__ inline double tetragamma(double x) {
  double z = x, shift = 0.0;
#pragma unroll 1
  while (z < 16.0) { shift += 2.0 / (z * z * z); z += 1.0; }
  const double r = 1.0 / z, r2 = r * r;
  const double tail = r2 * r2 * (0.5 - r2 * (1.0 / 6.0 - r2 * (1.0 / 6.0 - r2 * (0.3 - r2 * (5.0 / 6.0
                      - r2 * (691.0 / 210.0 - r2 * (17.5)))))));
  return -(r2 + r * r2 + tail + shift);
}

// The y > 0 with psi'(y) = x, x > 0: limma's trigammaInverse.  Newton on 1 / psi', which is convex and nearly linear in y, from
// y = 1/2 + 1/x, which lies below the root: the iterates rise to it.  The step is dif = psi'(y) (1 - psi'(y) / x) / psi''(y), and
// the iteration STOPS after the first step with -dif / y < 1e-8 (the step is applied; convergence is quadratic, so what is left
// is of the order 1e-16), or after 50 steps.  x > 1e7: 1 / sqrt(x), x < 1e-6: 1 / x (the leading terms; the next is 1e-7 relative
// at most, and the prior fit reaches neither: evar there means d0 below 1e-3 or above 1e6).  NaN for NaN; not for x <= 0.
// Against mpmath's root on 1e-6 <= x <= 1e7: 4.3e-16 relative (tests/test_site_diff_mod.py).
__device__ inline double trigamma_inverse(double x) {
  if (x != x) return x;
  if (x > 1e7) return 1.0 / sqrt(x);
  if (x < 1e-6) return 1.0 / x;
  double y = 0.5 + 1.0 / x;
#pragma unroll 1
  for (int it = 0; it < 50; ++it) {
    const double tri = trigamma(y);
    const double dif = tri * (1.0 - tri / x) / tetragamma(y);
    y += dif;
    if (-dif / y < 1e-8) break;
  }
  return y;
}

// The `level` quantile of F(1, nu) for real nu > 0, 0 < level < 1: the square of the t with student_t_two_sided(t, nu) = 1 - level,
// by bisection of that tail (decreasing in t) until the bracket is two neighbouring doubles; nu = +inf: norm_isf((1 - level) / 2)^2,
// the chi2_1 quantile.  One thread's work (the tail votes with __ballot: a lone thread's vote is its own).  Its error is the tail's:
// against mpmath over nu in {1 .. 14, 2.37, 14.6, 1e6, inf} and levels 0.9, 0.95, 0.999, compiled for the host: 2.6e-13 relative, but
// 1.9e-11 at nu = 1 and 0.999 (t = 637: the tail's log1p(-y) with y within 2.5e-6 of 1); on the device 4e-15 over the eleven fits
// of tests/test_site_diff_mod_gpu.py (tests/test_site_diff_mod.py; profiles/site_diff_mod.txt §3).
__device__ inline double f1_quantile(double level, double nu) {
  const double alpha = 1.0 - level;
  if (nu != nu || alpha != alpha) return __builtin_nan("");
  if (isinf(nu)) { const double z = norm_isf(0.5 * alpha); return z * z; }
  double lo = 0.0, hi = 1.0;
#pragma unroll 1
  while (student_t_two_sided(hi, nu) > alpha) {
    lo = hi; hi *= 2.0;
    if (hi > 1e150) return __builtin_inf();
  }
#pragma unroll 1
  for (int it = 0; it < 1100; ++it) {
    const double mid = lo + 0.5 * (hi - lo);
    if (mid <= lo || mid >= hi) break;
    if (student_t_two_sided(mid, nu) > alpha) lo = mid; else hi = mid;
  }
  const double t = lo + 0.5 * (hi - lo);
  return t * t;
}

}  // namespace nmod
