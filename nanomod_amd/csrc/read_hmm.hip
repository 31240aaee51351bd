// nmod_read_sites_count / nmod_read_hmm / nmod_read_hmm_grad — per read a two-state hidden Markov chain over the candidate sites it covers,
// emissions from the window sums (K13's llr_win), evaluated by forward-backward as a scan of 2 x 2 non-negative matrices (K19; K21 is the
// same chain's log-likelihood with its gradient in the two parameters).  The reference project has no such step; the
// definition is the one in include/nanomod_hip.h (tests/hmm_ref.py restates it).  The walk over the reads is read_walk.hpp's, the site
// search and the offsets' scan are site_search.hpp's (shared with K16 / K18); what the chain entries of K19 - K22 share is
// read_entries.hpp's (the refusals and ChainCall; ReadGeom, read_sum, and ReadDraw for the entries kernel).  All on the caller's stream:
//   read_classify_kernel     (read_walk.hpp) a thread per read: the read's class, by its events for the entries, by its entries for the chain
//   rh_entries_kernel<., 0>  the entries of a read counted: ballots over the sites it covers (nmod_read_sites_count)
//   sp_scan_kernel           (site_search.hpp) the counts' exclusive scan in place (hoff)
//   rh_entries_kernel<., 1>  the same walk: entry j of the read writes its site, its position and its score to row hoff[r] + j (every
//                            chain entry enqueues it through read_entries.hpp's ChainCall and rh_fill_entries)
//   rh_hmm_kernel<1>         a wave per read of up to NMOD_HMM_WAVE_MAX entries, four waves a workgroup
//   rh_hmm_kernel<4>         a workgroup of four waves per longer read
//   rh_grad_kernel<1>, <4>   nmod_read_hmm_grad (K21): the same two forms, the same forward pass; the backward pass forms the terms of the
//                            log-likelihood's gradient in logit(pi) and ln(length) instead of the posteriors
//   rh_grad_sums_kernel      its batch sums: one workgroup, a fixed order
//   rh_share_kernel          the prior entries (K23: nmod_read_hmm_prior, nmod_read_viterbi_prior, nmod_read_hmm_grad_prior) alone: behind
//                            the fill a thread per row resolves the share of the row's site once (the NaN rule, the clamp; for K20 its
//                            two logarithms); the chain kernels' <., true> instances read that word beside xs, the others never see it
// The chain of a read is two passes of one scan, rh_tile<., BWD>, over tiles of NMOD_HMM_CHUNK entries a thread: a thread forms the step
// matrices of its chunk and multiplies them in order, the lanes of a wave take the inclusive scan of those products (six shuffle steps on
// four doubles and an exponent), a workgroup hands the waves' totals on through LDS, and the thread replays its chunk as a row vector from
// the prefix in front of it.  The vector after a tile's last entry is carried into the next tile, so the entries of a read are bounded by
// the read alone.  The forward pass leaves the normalised forward vectors in the call's slab; the backward pass, the same scan over the
// reversed transposes, combines them into post and decides state, the runs and the site counts while it replays.  Every product is
// rescaled by a power of two (frexp of its largest entry, ldexp): scaling adds no rounding.  Integer atomics only (the site counts).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "read_entries.hpp"
#include "read_walk.hpp"
#include "site_search.hpp"

namespace nmod {

constexpr double kLn2 = 0.6931471805599453;

// the chain: the rows, the lists of the reads by their entries
struct RhArgs {
  int64_t nreads; const int64_t* hoff; int64_t nrows, nsites;
  ReadLists w;
  const int32_t* site; const double* xs;
  double* alpha;                                  // per row the forward vector, scaled (the backward pass reads it)
  double pi, q, length, call_post, call_lo;
  bool backward;                                  // an output that needs post was asked for
  nmod_hmm_out out;
  const double* share;                            // the prior entries: per row the clamped share of its site (unread by the other instances)
};

// ---------------------------------------------------------------------------------------------------------------- the entries

// FILL false: a read's count of entries; true: entry j goes to row hoff[read] + j, in ascending key
template <int WAVES, bool FILL>
__global__ __launch_bounds__(kRwThreads) void rh_entries_kernel(RhEntArgs a) {
  __shared__ unsigned sh_item;
  __shared__ int sh_tile[kRwWaves];
  const ReadGeom<WAVES> geo;
  const ReadDraw<WAVES> reads(a.w, sh_item);
  for (;;) {
    const ReadRows r = reads.draw();
    if (!r.more) break;
    const int64_t read = r.read;
    int64_t begin, n;
    csr_row(a.roff, 0, read, begin, n);
    const int64_t cs = a.cs[read], start = a.start[read];
    if (n <= 0 || cs < 0 || start < 0 || start > kSpPosMask) continue;   // (the counts are zeroed by the entry)
    const int64_t last_pos = start + n - 1 < kSpPosMask ? start + n - 1 : kSpPosMask;
    const int64_t c_lo = sp_bound<false>(a.key, 0, a.nsites, (cs << 40) | start);
    const int64_t c_hi = sp_bound<true>(a.key, c_lo, a.nsites, (cs << 40) | last_pos);
    const SpRead rd{read, start, n, (cs & 1) != 0, a.score + begin, a.key};
    int64_t base = 0, m = 0;
    if constexpr (FILL) {
      base = a.hoff[read]; m = a.hoff[read + 1] - base;
      if (m <= 0) continue;
    }
    int64_t done = 0;                                           // the entries in front of the tile
    for (int64_t s0 = c_lo; s0 < c_hi; s0 += geo.T) {
      const int64_t s = s0 + geo.t;
      double l = 0.0;
      const bool v = s < c_hi && rd.score_at(s, l) && fabs(l) <= kDblMax;
      const unsigned long long b = __ballot(v);
      int before = __popcll(b & ((1ull << geo.lane) - 1ull)), total = __popcll(b);
      if constexpr (WAVES > 1) {
        __syncthreads();                                        // the last tile's words are read
        if (geo.lane == 0) sh_tile[geo.wave] = total;
        __syncthreads();
        total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) { before += w < geo.wave ? sh_tile[w] : 0; total += sh_tile[w]; }
      }
      if constexpr (FILL) {
        const int64_t j = done + before, row = base + j;
        if (v && j < m && row >= 0 && row < a.nrows) {          // (offsets that are not this call's counts: outside the rows)
          a.site[row] = (int32_t)s;
          a.xs[2 * row] = (double)(a.key[s] & kSpPosMask);
          a.xs[2 * row + 1] = l;
        }
      }
      done += total;
    }
    if constexpr (!FILL) { if (geo.t == 0) a.cnt[read] = done; }
  }
}

void rh_fill_entries(const RhEntArgs& e, int num_cus, hipStream_t stream) {
  rh_launch(e, rh_entries_kernel<1, true>, rh_entries_kernel<kRwWaves, true>, num_cus, stream);
}

// The share of every row, once a call: pi_j = site_pi[site_j] clamped to 1e-9 .. 1 - 1e-9 (an infinity with the rest), pi where that word
// is a NaN (or the row has no site of this call's: a row no read owns).  stride 1: the share alone; 3: (pi_j, log q_j, log pi_j) with
// q_j = 1 - pi_j, what the chain kernels form it as
__global__ __launch_bounds__(256) void rh_share_kernel(int64_t nrows, const int32_t* site, int64_t nsites, const double* site_pi, double pi,
                                                       int stride, double* share) {
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < nrows; row += (int64_t)gridDim.x * 256) {
    const int64_t s = site[row];
    double v = s >= 0 && s < nsites ? site_pi[s] : pi;
    if (v != v) v = pi;
    v = v < kSharePiLo ? kSharePiLo : (v > kSharePiHi ? kSharePiHi : v);
    share[stride * row] = v;
    if (stride == 3) { share[3 * row + 1] = log(1.0 - v); share[3 * row + 2] = log(v); }
  }
}

void rh_fill_shares(const RhEntArgs& e, const double* site_pi, double pi, int stride, double* share, int num_cus, hipStream_t stream) {
  hipLaunchKernelGGL(rh_share_kernel, dim3(persistent_grid(e.nrows, 256, (int64_t)num_cus * 8)), dim3(256), 0, stream, e.nrows, e.site, e.nsites,
                     site_pi, pi, stride, share);
}

// ---------------------------------------------------------------------------------------------------------------- the scan

struct Mat2 { double a, b, c, d; int e; };          // [[a, b], [c, d]] * 2^e: rows the state before, columns the state after
struct Vec2 { double x0, x1; int64_t e; };          // a row vector * 2^e

// the exponent that brings the largest of non-negative entries into [0.5, 1); 0 where there is none to scale by
__device__ __forceinline__ int rh_exponent(double mx) {
  int ex = 0;
  if (mx > 0.0 && mx <= kDblMax) (void)frexp(mx, &ex);
  return ex;
}

__device__ __forceinline__ Mat2 rh_mul(const Mat2& l, const Mat2& r) {
  Mat2 o;
  o.a = l.a * r.a + l.b * r.c; o.b = l.a * r.b + l.b * r.d;
  o.c = l.c * r.a + l.d * r.c; o.d = l.c * r.b + l.d * r.d;
  const int ex = rh_exponent(fmax(fmax(o.a, o.b), fmax(o.c, o.d)));
  o.a = ldexp(o.a, -ex); o.b = ldexp(o.b, -ex); o.c = ldexp(o.c, -ex); o.d = ldexp(o.d, -ex);
  o.e = l.e + r.e + ex;
  return o;
}

__device__ __forceinline__ Vec2 rh_vmul(const Vec2& x, const Mat2& m) {
  Vec2 y;
  y.x0 = x.x0 * m.a + x.x1 * m.c; y.x1 = x.x0 * m.b + x.x1 * m.d;
  const int ex = rh_exponent(fmax(y.x0, y.x1));
  y.x0 = ldexp(y.x0, -ex); y.x1 = ldexp(y.x1, -ex);
  y.e = x.e + m.e + ex;
  return y;
}

__device__ __forceinline__ Mat2 rh_shfl_up(const Mat2& m, int d) {
  Mat2 o;
  o.a = __shfl_up(m.a, d); o.b = __shfl_up(m.b, d); o.c = __shfl_up(m.c, d); o.d = __shfl_up(m.d, d); o.e = __shfl_up(m.e, d);
  return o;
}

// the emission of a score, scaled so that the larger is 1: (exp(-max(s, 0)), exp(min(s, 0)))
__device__ __forceinline__ void rh_emission(double s, double& e0, double& e1) {
  const double en = exp(-fabs(s));
  e0 = s > 0.0 ? en : 1.0; e1 = s < 0.0 ? en : 1.0;
}

// Step k of the scan over the m entries at xs (position, score per entry).  Forward: T_k diag(e_k), T_0 the identity.  Backward: the
// transpose of T_j diag(e_j) for j = m - k, the identity at k = 0.  The identity beyond the read.  PRIOR: the share of T_j is pr[j], that
// of the entry arrived at, and q_j = 1 - pr[j] is formed here (the same double wherever entry j is met); pr is unread otherwise
template <bool BWD, bool PRIOR>
__device__ __forceinline__ Mat2 rh_step(const RhArgs& a, const double* xs, const double* pr, int64_t k, int64_t m) {
  Mat2 o{1.0, 0.0, 0.0, 1.0, 0};
  if (k >= m || (BWD && k == 0)) return o;
  const int64_t j = BWD ? m - k : k;
  double e0, e1;
  rh_emission(xs[2 * j + 1], e0, e1);
  double t00 = 1.0, t01 = 0.0, t10 = 0.0, t11 = 1.0;
  if (j > 0) {
    const double r = (xs[2 * j] - xs[2 * (j - 1)]) / a.length;
    const double rho = exp(-r), eps = -expm1(-r);
    double pi = a.pi, q = a.q;
    if constexpr (PRIOR) { pi = pr[j]; q = 1.0 - pi; }
    t00 = q + pi * rho; t01 = pi * eps; t10 = q * eps; t11 = pi + q * rho;
  }
  if constexpr (BWD) { o.a = e0 * t00; o.b = e0 * t10; o.c = e1 * t01; o.d = e1 * t11; }
  else { o.a = t00 * e0; o.b = t01 * e1; o.c = t10 * e0; o.d = t11 * e1; }
  return o;
}

struct RhShared { Mat2 tot[kRwWaves]; Vec2 carry; };

// One tile of the scan, steps k0 .. k0 + T * kHmmChunk - 1, by the T threads of the read: per_entry(k, x) with x the row vector after
// step k, for the steps inside the read.  Returns the vector after the tile's last step (thread T - 1's), the same in every thread
template <int WAVES, bool BWD, bool PRIOR, class F>
__device__ __forceinline__ Vec2 rh_tile(const RhArgs& a, const double* xs, const double* pr, int64_t m, int64_t k0, const Vec2& carry, RhShared& sh,
                                        F per_entry) {
  constexpr int T = WAVES * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WAVES == 1 ? lane : (int)threadIdx.x;
  const int64_t kb = k0 + (int64_t)t * kHmmChunk;
  Mat2 step[kHmmChunk];
#pragma unroll
  for (int c = 0; c < kHmmChunk; ++c) step[c] = rh_step<BWD, PRIOR>(a, xs, pr, kb + c, m);
  Mat2 prod = step[0];
#pragma unroll
  for (int c = 1; c < kHmmChunk; ++c) prod = rh_mul(prod, step[c]);
  // the inclusive scan over the lanes: steps 1 .. 32, the earlier lanes' product on the left
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const Mat2 o = rh_shfl_up(prod, d);
    if (lane >= d) prod = rh_mul(o, prod);
  }
  Vec2 x = carry;
  if constexpr (WAVES > 1) {
    __syncthreads();                                            // the last tile's totals and carry are read
    if (lane == 63) sh.tot[wave] = prod;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES - 1; ++w) if (w < wave) x = rh_vmul(x, sh.tot[w]);
  }
  const Mat2 before = rh_shfl_up(prod, 1);
  if (lane > 0) x = rh_vmul(x, before);
#pragma unroll
  for (int c = 0; c < kHmmChunk; ++c) {
    if (kb + c < m) {
      x = rh_vmul(x, step[c]);
      per_entry(kb + c, x);
    }
  }
  Vec2 out;
  if constexpr (WAVES == 1) {
    out.x0 = __shfl(x.x0, 63); out.x1 = __shfl(x.x1, 63);
    const long long e = (long long)x.e;
    out.e = ((int64_t)__shfl((int)(e >> 32), 63) << 32) | (int64_t)(uint32_t)__shfl((int)e, 63);
  } else {
    if (t == T - 1) sh.carry = x;
    __syncthreads();
    out = sh.carry;
  }
  return out;
}

template <int WAVES, bool PRIOR>
__global__ __launch_bounds__(kRwThreads) void rh_hmm_kernel(RhArgs a) {
  __shared__ unsigned sh_item;
  __shared__ int sh_cnt[3 * kRwWaves];
  __shared__ int sh_last[kRwWaves + 1];
  __shared__ double sh_sum[kRwWaves];
  __shared__ RhShared sh_scan;
  const ReadGeom<WAVES> geo;
  const unsigned cnt = a.w.count[geo.CLS];
  const nmod_hmm_out& o = a.out;
  for (;;) {
    const unsigned item = draw_read<WAVES>(a.w, sh_item);
    if (item >= cnt) break;
    const int64_t read = (int64_t)a.w.list[geo.CLS][item];
    const int64_t base = a.hoff[read], m = a.hoff[read + 1] - base;
    if (m <= 0 || base < 0 || base > a.nrows - m) {             // no entry (or offsets that are not the rows': skipped)
      if (geo.t == 0) {
        if (o.n_sites) o.n_sites[read] = 0;
        if (o.n_mod) o.n_mod[read] = 0;
        if (o.n_can) o.n_can[read] = 0;
        if (o.n_runs) o.n_runs[read] = 0;
        if (o.ll) o.ll[read] = 0.0;
        if (o.ll_indep) o.ll_indep[read] = 0.0;
        if (o.status) o.status[read] = NMOD_HMM_NO_SITE;
      }
      continue;
    }
    const double* xs = a.xs + 2 * base;
    const double* pr = PRIOR ? a.share + base : nullptr;
    double* alpha = a.alpha + 2 * base;

    // forward: the vectors, the independent likelihood and the sum of the positive scores, a thread's entries in ascending order
    double s_ind = 0.0, s_pos = 0.0;
    Vec2 fw{a.q, a.pi, 0};
    if constexpr (PRIOR) { fw.x0 = 1.0 - pr[0]; fw.x1 = pr[0]; }
    for (int64_t k0 = 0; k0 < m; k0 += geo.TS) {
      fw = rh_tile<WAVES, false, PRIOR>(a, xs, pr, m, k0, fw, sh_scan, [&](int64_t k, const Vec2& x) {
        if (a.backward) { alpha[2 * k] = x.x0; alpha[2 * k + 1] = x.x1; }
        const double s = xs[2 * k + 1], up = fmax(s, 0.0);
        double e0, e1;
        rh_emission(s, e0, e1);
        double pi = a.pi, q = a.q;
        if constexpr (PRIOR) { pi = pr[k]; q = 1.0 - pi; }
        s_ind += log(q * e0 + pi * e1) + up;
        s_pos += up;
      });
    }
    const double ind = read_sum<WAVES>(s_ind, sh_sum), pos = read_sum<WAVES>(s_pos, sh_sum);
    const double ll = (log(fw.x0 + fw.x1) + (double)fw.e * kLn2) + pos;

    // backward: the same scan over the reversed transposes; step k is entry m - 1 - k
    int n_mod = 0, n_can = 0, n_runs = 0;
    if (a.backward) {
      if constexpr (WAVES > 1) __syncthreads();                 // the forward vectors of the other waves are written
      Vec2 bw{1.0, 1.0, 0};
      int tile_prev = 2;                                        // the state of the step in front of the tile (none: not a 1)
      for (int64_t k0 = 0; k0 < m; k0 += geo.TS) {
        int st[kHmmChunk];
        const int64_t kb = k0 + (int64_t)geo.t * kHmmChunk;
        bw = rh_tile<WAVES, true, PRIOR>(a, xs, pr, m, k0, bw, sh_scan, [&](int64_t k, const Vec2& x) {
          const int64_t j = m - 1 - k, row = base + j;
          const double p0 = alpha[2 * j] * x.x0, p1 = alpha[2 * j + 1] * x.x1;
          const double post = p1 / (p0 + p1);
          const int state = post >= a.call_post ? 1 : (post <= a.call_lo ? 0 : 2);
          st[(int)(k - kb)] = state;
          if (o.post) o.post[row] = post;
          if (o.state) o.state[row] = (uint8_t)state;
          n_mod += state == 1; n_can += state == 0;
          const int64_t s = a.site[row];
          if (s >= 0 && s < a.nsites) {
            if (o.site_n) atomicAdd(&o.site_n[s], 1);
            if (o.site_mod && state == 1) atomicAdd(&o.site_mod[s], 1);
            if (o.site_can && state == 0) atomicAdd(&o.site_can[s], 1);
          }
        });
        // the runs of state 1 by their ends in scan order: a step in state 1 whose step before is not.  The step before a thread's
        // first is its neighbour's last (a thread with a step inside the read has only full chunks in front of it)
        int last = 2;
#pragma unroll
        for (int c = 0; c < kHmmChunk; ++c) if (kb + c < m) last = st[c];
        int prev = __shfl_up(last, 1);
        if constexpr (WAVES > 1) {
          __syncthreads();
          if (geo.lane == 63) sh_last[geo.wave] = last;
          __syncthreads();
          if (geo.lane == 0 && geo.wave > 0) prev = sh_last[geo.wave - 1];
        }
        if (geo.t == 0) prev = tile_prev;
#pragma unroll
        for (int c = 0; c < kHmmChunk; ++c) {
          if (kb + c < m) { n_runs += st[c] == 1 && prev != 1; prev = st[c]; }
        }
        if constexpr (WAVES == 1) tile_prev = __shfl(last, 63); else tile_prev = sh_last[WAVES - 1];
      }
      read_counts<WAVES>(sh_cnt, n_mod, n_can, n_runs);
    }
    if (geo.t == 0) {
      if (o.n_sites) o.n_sites[read] = (int32_t)m;
      if (o.n_mod) o.n_mod[read] = n_mod;
      if (o.n_can) o.n_can[read] = n_can;
      if (o.n_runs) o.n_runs[read] = n_runs;
      if (o.ll) o.ll[read] = ll;
      if (o.ll_indep) o.ll_indep[read] = ind;
      if (o.status) o.status[read] = 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the gradient (K21)

// nmod_read_hmm_grad: the chain's arguments (h.backward set: the forward vectors are stored; h.out unused) and the outputs of its own
struct RgArgs {
  int64_t nreads;                                 // (rh_launch reads it)
  RhArgs h;
  double piq;                                     // pi q, formed once on the host
  nmod_hmm_grad_out out;                          // ll, g_eta and g_lam never NULL here: the slab's where the caller asked for none
};

// The forward pass is rh_hmm_kernel's, tile for tile (ll has its bits).  The backward pass is the same scan; at step k, entry j = m - 1 - k,
// the lambda holds b_j and reads a_(j-1), which the forward pass left in the slab: the term of transition j (Fisher's identity) needs
// nothing else.  A thread adds its terms in the order of its steps, then the sums of the read as S's.  PRIOR: the shares of T_j and L_j are
// entry j's, and the term of g_eta is (pi_j q_j) P_j, the product rounded where it is formed: the sums hold the products
template <int WAVES, bool PRIOR>
__global__ __launch_bounds__(kRwThreads) void rh_grad_kernel(RgArgs g) {
  __shared__ unsigned sh_item;
  __shared__ double sh_sum[kRwWaves];
  __shared__ RhShared sh_scan;
  const ReadGeom<WAVES> geo;
  const RhArgs& a = g.h;
  const unsigned cnt = a.w.count[geo.CLS];
  const nmod_hmm_grad_out& o = g.out;
  for (;;) {
    const unsigned item = draw_read<WAVES>(a.w, sh_item);
    if (item >= cnt) break;
    const int64_t read = (int64_t)a.w.list[geo.CLS][item];
    const int64_t base = a.hoff[read], m = a.hoff[read + 1] - base;
    if (m <= 0 || base < 0 || base > a.nrows - m) {             // no entry (or offsets that are not the rows': skipped)
      if (geo.t == 0) {
        o.ll[read] = 0.0; o.g_eta[read] = 0.0; o.g_lam[read] = 0.0;
        if (o.abs_eta) o.abs_eta[read] = 0.0;
        if (o.abs_lam) o.abs_lam[read] = 0.0;
        if (o.status) o.status[read] = NMOD_HMM_NO_SITE;
      }
      continue;
    }
    const double* xs = a.xs + 2 * base;
    const double* pr = PRIOR ? a.share + base : nullptr;
    double* alpha = a.alpha + 2 * base;

    // forward: the vectors and the sum of the positive scores, a thread's entries in ascending order
    double s_pos = 0.0;
    Vec2 fw{a.q, a.pi, 0};
    if constexpr (PRIOR) { fw.x0 = 1.0 - pr[0]; fw.x1 = pr[0]; }
    for (int64_t k0 = 0; k0 < m; k0 += geo.TS) {
      fw = rh_tile<WAVES, false, PRIOR>(a, xs, pr, m, k0, fw, sh_scan, [&](int64_t k, const Vec2& x) {
        alpha[2 * k] = x.x0; alpha[2 * k + 1] = x.x1;
        s_pos += fmax(xs[2 * k + 1], 0.0);
      });
    }
    const double pos = read_sum<WAVES>(s_pos, sh_sum);
    const double ll = (log(fw.x0 + fw.x1) + (double)fw.e * kLn2) + pos;

    // the forward vectors of the other lanes (waves) are written
    if constexpr (WAVES > 1) __syncthreads(); else __threadfence_block();

    // backward: step k is entry j = m - 1 - k; the term of transition j for j >= 1, the posterior of the first entry at j = 0
    double s_p = 0.0, s_l = 0.0, s_ap = 0.0, s_al = 0.0, s_post = 0.0;
    Vec2 bw{1.0, 1.0, 0};
    for (int64_t k0 = 0; k0 < m; k0 += geo.TS) {
      bw = rh_tile<WAVES, true, PRIOR>(a, xs, pr, m, k0, bw, sh_scan, [&](int64_t k, const Vec2& x) {
        const int64_t j = m - 1 - k;
        if (j == 0) {
          const double p0 = alpha[0] * x.x0, p1 = alpha[1] * x.x1;
          s_post = p1 / (p0 + p1);
          return;
        }
        double e0, e1;
        rh_emission(xs[2 * j + 1], e0, e1);
        const double r = (xs[2 * j] - xs[2 * (j - 1)]) / a.length;
        const double rho = exp(-r), eps = -expm1(-r);
        double pi = a.pi, q = a.q;
        if constexpr (PRIOR) { pi = pr[j]; q = 1.0 - pi; }
        const double t00 = q + pi * rho, t01 = pi * eps, t10 = q * eps, t11 = pi + q * rho;
        const double y0 = e0 * x.x0, y1 = e1 * x.x1;
        const double a0 = alpha[2 * (j - 1)], a1 = alpha[2 * (j - 1) + 1];
        const double z = a0 * (t00 * y0 + t01 * y1) + a1 * (t10 * y0 + t11 * y1);
        double p = eps * (a0 + a1) * (y1 - y0) / z;
        if constexpr (PRIOR) p = (pi * q) * p;
        const double l = rho * r * (pi * a0 - q * a1) * (y0 - y1) / z;
        s_p += p; s_l += l; s_ap += fabs(p); s_al += fabs(l);
      });
    }
    // (the posterior lives in one thread and the others add 0: its sum is the value itself)
    const double sum_p = read_sum<WAVES>(s_p, sh_sum), sum_l = read_sum<WAVES>(s_l, sh_sum), sum_ap = read_sum<WAVES>(s_ap, sh_sum);
    const double sum_al = read_sum<WAVES>(s_al, sh_sum), post0 = read_sum<WAVES>(s_post, sh_sum);
    if (geo.t == 0) {
      const double first = post0 - (PRIOR ? pr[0] : a.pi);
      o.ll[read] = ll;
      o.g_eta[read] = PRIOR ? first + sum_p : first + g.piq * sum_p;
      o.g_lam[read] = sum_l;
      if (o.abs_eta) o.abs_eta[read] = PRIOR ? fabs(first) + sum_ap : fabs(first) + g.piq * sum_ap;
      if (o.abs_lam) o.abs_lam[read] = sum_al;
      if (o.status) o.status[read] = 0;
    }
  }
}

// The batch sums in one workgroup of 256: thread t adds reads t, t + 256, ... in ascending order (a product is formed, then added),
// then the block sum of every word.  Words 6 and 7: the reads with an entry and the entries, counted as doubles (exact below 2^53)
__global__ __launch_bounds__(256) void rh_grad_sums_kernel(int64_t nreads, const int64_t* hoff, int64_t nrows, const double* ll, const double* g_eta,
                                                           const double* g_lam, double* sums) {
  __shared__ double sh[4];
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t r = threadIdx.x; r < nreads; r += 256) {
    const double l = ll[r], e = g_eta[r], v = g_lam[r];
    s[0] += l; s[1] += e; s[2] += v; s[3] += e * e; s[4] += e * v; s[5] += v * v;
    const int64_t base = hoff[r], m = hoff[r + 1] - base;
    if (!(m <= 0 || base < 0 || base > nrows - m)) { s[6] += 1.0; s[7] += (double)m; }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const double v = block_sum_f64<4>(s[i], sh);
    if (threadIdx.x == 0) sums[i] = v;
  }
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_read_sites_count(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                     const double* score, int64_t nsites, const int64_t* key, int64_t* hoff_out, int64_t* nrows_out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!hoff_out || !nrows_out) return NMOD_ERR_INVALID_ARG;
  if (!sp_walk_args_ok(prm, nreads, cs, start, roff, score, nsites, key, nullptr, 0)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && nreads == 0) { hoff_out[0] = 0; *nrows_out = 0; return NMOD_OK; }
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t nr = (size_t)nreads;
  const size_t tot = host ? (size_t)roff[nreads] : 0;
  int64_t* hoff = hoff_out;
  int64_t total = 0;

  RhEntArgs a;
  rh_ent_args(a, nreads, cs, start, roff, score, nsites, key);
  Slab slab(host);
  const ReadListSpace lists(slab, nr);
  rh_stage_reads(slab, a, tot);
  slab.out(hoff, (nr + 1) * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.cnt = hoff;
  NMOD_HIP(hipMemsetAsync(hoff, 0, (nr + 1) * 8, stream));
  if (nreads > 0 && nsites > 0) {
    NMOD_HIP(lists.fill(slab, a.roff, nreads, num_cus, stream, a.w));
    rh_launch(a, rh_entries_kernel<1, false>, rh_entries_kernel<kRwWaves, false>, num_cus, stream);
  }
  hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(256), 0, stream, hoff, nreads);
  NMOD_HIP(hipMemcpyAsync(&total, hoff + nreads, 8, hipMemcpyDeviceToHost, stream));
  NMOD_HIP(hipStreamSynchronize(stream));
  const int rc_end = launches_end(slab, stream);
  if (rc_end != NMOD_OK) return rc_end;
  if (total > (int64_t)INT32_MAX) return NMOD_ERR_INVALID_ARG;
  *nrows_out = total;
  return NMOD_OK;
}

// nmod_read_hmm (prior false: site_pi unread) and nmod_read_hmm_prior: one body, the kernels' instances chosen at the launch
static int rh_hmm_entry(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff, const double* score,
                        int64_t nsites, const int64_t* key, bool prior, const double* site_pi, const int64_t* hoff, int64_t nrows,
                        const nmod_hmm_opts* opts, const nmod_hmm_out* out) {
  if (!rh_chain_args_ok(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows)) return NMOD_ERR_INVALID_ARG;
  if (prior && nsites > 0 && !site_pi) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_hmm_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_hmm_out)) return NMOD_ERR_INVALID_ARG;
  if (!rh_chain_opts_ok(opts->pi, opts->length)) return NMOD_ERR_INVALID_ARG;
  if (!(opts->call_post > 0.5) || !(opts->call_post < 1.0)) return NMOD_ERR_INVALID_ARG;
  ChainCall c(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows, !out->site);
  const size_t nr = c.nr, ns = c.ns, nw = c.nw;
  if (c.host && nreads == 0) {                                  // nothing to enqueue: the site counts of no read
    if (out->site_n) memset(out->site_n, 0, ns * 4);
    if (out->site_mod) memset(out->site_mod, 0, ns * 4);
    if (out->site_can) memset(out->site_can, 0, ns * 4);
    return NMOD_OK;
  }
  const int rc = select_device(prm, &c.num_cus);
  if (rc != NMOD_OK) return rc;

  RhArgs a;
  memset(&a, 0, sizeof(a));
  a.nreads = nreads; a.nrows = nrows; a.nsites = nsites;
  a.pi = opts->pi; a.q = 1.0 - opts->pi; a.length = opts->length;
  a.call_post = opts->call_post; a.call_lo = 1.0 - opts->call_post;
  a.out = *out;
  const nmod_hmm_out& o = a.out;
  a.backward = o.post || o.state || o.n_mod || o.n_can || o.n_runs || o.site_n || o.site_mod || o.site_can;

  // the call's slab (ChainCall's share: the read lists of both walks, per row the position and the score, and the site where the caller
  // asked for none): the forward vector; for the host entry the inputs and outputs as well
  Slab& slab = c.slab;
  const size_t o_alpha = slab.take(a.backward ? nw * 16 : 0);
  if (prior) c.prior(site_pi, opts->pi, 1);
  c.stage();
  slab.out(a.out.post, nw * 8); slab.out(a.out.site, nw * 4); slab.out(a.out.state, nw);
  slab.out(a.out.n_sites, nr * 4); slab.out(a.out.n_mod, nr * 4); slab.out(a.out.n_can, nr * 4); slab.out(a.out.n_runs, nr * 4);
  slab.out(a.out.ll, nr * 8); slab.out(a.out.ll_indep, nr * 8); slab.out(a.out.status, nr);
  slab.out(a.out.site_n, ns * 4); slab.out(a.out.site_mod, ns * 4); slab.out(a.out.site_can, ns * 4);
  NMOD_HIP(slab.commit(c.stream, prm->device));
  c.bind(o.site);
  a.hoff = c.e.hoff; a.xs = c.e.xs; a.site = c.e.site; a.alpha = slab.at<double>(o_alpha); a.share = c.share;

  if (o.site_n) NMOD_HIP(hipMemsetAsync(o.site_n, 0, ns * 4, c.stream));
  if (o.site_mod) NMOD_HIP(hipMemsetAsync(o.site_mod, 0, ns * 4, c.stream));
  if (o.site_can) NMOD_HIP(hipMemsetAsync(o.site_can, 0, ns * 4, c.stream));
  if (nreads > 0) {
    NMOD_HIP(c.lists(a.w));
    if (prior) rh_launch(a, rh_hmm_kernel<1, true>, rh_hmm_kernel<kRwWaves, true>, c.num_cus, c.stream);
    else rh_launch(a, rh_hmm_kernel<1, false>, rh_hmm_kernel<kRwWaves, false>, c.num_cus, c.stream);
  }
  return launches_end(slab, c.stream);
}

extern "C" int nmod_read_hmm(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                             const double* score, int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows,
                             const nmod_hmm_opts* opts, const nmod_hmm_out* out) {
  return rh_hmm_entry(prm, nreads, cs, start, roff, score, nsites, key, false, nullptr, hoff, nrows, opts, out);
}

extern "C" int nmod_read_hmm_prior(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                   const double* score, int64_t nsites, const int64_t* key, const double* site_pi, const int64_t* hoff,
                                   int64_t nrows, const nmod_hmm_opts* opts, const nmod_hmm_out* out) {
  return rh_hmm_entry(prm, nreads, cs, start, roff, score, nsites, key, true, site_pi, hoff, nrows, opts, out);
}

// nmod_read_hmm_grad and nmod_read_hmm_grad_prior, as rh_hmm_entry
static int rh_grad_entry(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff, const double* score,
                         int64_t nsites, const int64_t* key, bool prior, const double* site_pi, const int64_t* hoff, int64_t nrows,
                         const nmod_hmm_grad_opts* opts, const nmod_hmm_grad_out* out) {
  if (!rh_chain_args_ok(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows)) return NMOD_ERR_INVALID_ARG;
  if (prior && nsites > 0 && !site_pi) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_hmm_grad_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_hmm_grad_out)) return NMOD_ERR_INVALID_ARG;
  if (!rh_chain_opts_ok(opts->pi, opts->length)) return NMOD_ERR_INVALID_ARG;
  ChainCall c(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows, true);
  const size_t nr = c.nr, nw = c.nw;
  if (c.host && nreads == 0) {                                  // nothing to enqueue: the sums of no read
    if (out->sums) memset(out->sums, 0, 8 * sizeof(double));
    return NMOD_OK;
  }
  const int rc = select_device(prm, &c.num_cus);
  if (rc != NMOD_OK) return rc;

  RgArgs g;
  memset(&g, 0, sizeof(g));
  RhArgs& a = g.h;
  g.nreads = a.nreads = nreads; a.nrows = nrows; a.nsites = nsites;
  a.pi = opts->pi; a.q = 1.0 - opts->pi; a.length = opts->length;
  a.backward = true;
  g.piq = a.pi * a.q;
  g.out = *out;
  nmod_hmm_grad_out& o = g.out;

  // the call's slab (ChainCall's share: the read lists of both walks, per row the position, the score and the site): the forward vector; the
  // per-read values the sums are taken from where the caller asked for the sums without them; for the host entry the inputs and outputs
  Slab& slab = c.slab;
  const size_t o_alpha = slab.take(nw * 16);
  const size_t o_ll = o.ll ? 0 : slab.take(nr * 8), o_ge = o.g_eta ? 0 : slab.take(nr * 8), o_gl = o.g_lam ? 0 : slab.take(nr * 8);
  if (prior) c.prior(site_pi, opts->pi, 1);
  c.stage();
  slab.out(o.ll, nr * 8); slab.out(o.g_eta, nr * 8); slab.out(o.g_lam, nr * 8); slab.out(o.abs_eta, nr * 8); slab.out(o.abs_lam, nr * 8);
  slab.out(o.status, nr); slab.out(o.sums, 8 * sizeof(double));
  NMOD_HIP(slab.commit(c.stream, prm->device));
  c.bind(nullptr);
  a.hoff = c.e.hoff; a.xs = c.e.xs; a.site = c.e.site; a.alpha = slab.at<double>(o_alpha); a.share = c.share;
  if (!o.ll) o.ll = slab.at<double>(o_ll);
  if (!o.g_eta) o.g_eta = slab.at<double>(o_ge);
  if (!o.g_lam) o.g_lam = slab.at<double>(o_gl);

  if (nreads > 0) {
    NMOD_HIP(c.lists(a.w));
    if (prior) rh_launch(g, rh_grad_kernel<1, true>, rh_grad_kernel<kRwWaves, true>, c.num_cus, c.stream);
    else rh_launch(g, rh_grad_kernel<1, false>, rh_grad_kernel<kRwWaves, false>, c.num_cus, c.stream);
  }
  if (o.sums) hipLaunchKernelGGL(rh_grad_sums_kernel, dim3(1), dim3(256), 0, c.stream, nreads, a.hoff, nrows, o.ll, o.g_eta, o.g_lam, o.sums);
  return launches_end(slab, c.stream);
}

extern "C" int nmod_read_hmm_grad(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                  const double* score, int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows,
                                  const nmod_hmm_grad_opts* opts, const nmod_hmm_grad_out* out) {
  return rh_grad_entry(prm, nreads, cs, start, roff, score, nsites, key, false, nullptr, hoff, nrows, opts, out);
}

extern "C" int nmod_read_hmm_grad_prior(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                        const double* score, int64_t nsites, const int64_t* key, const double* site_pi, const int64_t* hoff,
                                        int64_t nrows, const nmod_hmm_grad_opts* opts, const nmod_hmm_grad_out* out) {
  return rh_grad_entry(prm, nreads, cs, start, roff, score, nsites, key, true, site_pi, hoff, nrows, opts, out);
}
