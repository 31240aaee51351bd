// nmod_read_viterbi — per read the jointly most probable state path of K19's two-state chain over the candidate sites it covers, the
// max-marginal margin of every entry and the path's log-probability (K20).  The reference project has no such step; the
// definition is the one in include/nanomod_hip.h (tests/viterbi_ref.py restates it).  What the chain entries of K19 - K22 share is
// read_entries.hpp's (the refusals and ChainCall, which enqueues the entries; ReadGeom, read_sum); all on the caller's stream:
//   read_classify_kernel     (read_walk.hpp) a thread per read: the read's class, by its events for the entries, by its entries for the chain
//   rh_entries_kernel<., 1>  (read_hmm.hip, through ChainCall) entry j of the read writes its site, position and score to row hoff[r] + j
//   rv_viterbi_kernel<1>     a wave per read of up to NMOD_HMM_WAVE_MAX entries, four waves a workgroup
//   rv_viterbi_kernel<4>     a workgroup of four waves per longer read
// nmod_read_viterbi_prior (K23) is the same entry with the <., true> instances: per row (pi_j, log q_j, log pi_j), resolved once a call by
// read_hmm.hip's rh_share_kernel behind the fill, is read beside xs; the other instances never see it.
// K19's scan in the (max, +) algebra: rv_tile<., BWD> is rh_tile with a sum for every product and the larger for every sum, no exponent
// word and no rescaling, and the replay hands the back-pointers of a step to its caller with the vector.  Three passes per read: the
// forward scan (back-pointers, a byte per row, and the forward vectors where delta is asked for, both in the call's slab), the traceback
// from the last entry to the first (the maps {0, 1} -> {0, 1} of a chunk composed, the lanes' scan of the compositions, the state carried
// from tile to tile) and, for delta alone, the backward scan over the reversed transposes.  Integer atomics only (the site counts).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "read_entries.hpp"
#include "read_walk.hpp"
#include "site_search.hpp"

namespace nmod {

struct RvArgs {
  int64_t nreads; const int64_t* hoff; int64_t nrows, nsites;
  ReadLists w;
  const int32_t* site; const double* xs;
  double* alpha;                                  // per row the forward vector (the backward pass reads it)
  uint8_t* psi;                                   // per row the back-pointers of its step: bit c = psi(c) (the traceback reads it)
  double pi, q, length, lq, lpi;
  bool trace, back;                               // an output that needs the path / delta was asked for
  nmod_vit_out out;
  const double* share;                            // the prior entry: per row (pi_j, log q_j, log pi_j) (unread by the other instances)
};

struct LMat { double a, b, c, d; };               // [[a, b], [c, d]] of logarithms: rows the state before, columns the state after
struct LVec { double x0, x1; };

// the larger of two sums, the first of equals: the header's rule for every maximum
__device__ __forceinline__ double rv_max(double s0, double s1) { return s1 > s0 ? s1 : s0; }

__device__ __forceinline__ LMat rv_mul(const LMat& l, const LMat& r) {
  LMat o;
  o.a = rv_max(l.a + r.a, l.b + r.c); o.b = rv_max(l.a + r.b, l.b + r.d);
  o.c = rv_max(l.c + r.a, l.d + r.c); o.d = rv_max(l.c + r.b, l.d + r.d);
  return o;
}

// y = x (max, +) m; psi: bit c set iff x_1 + m_1c > x_0 + m_0c, from the sums that give y_c
__device__ __forceinline__ LVec rv_vmul(const LVec& x, const LMat& m, unsigned& psi) {
  const double s00 = x.x0 + m.a, s10 = x.x1 + m.c, s01 = x.x0 + m.b, s11 = x.x1 + m.d;
  const bool p0 = s10 > s00, p1 = s11 > s01;
  psi = (p0 ? 1u : 0u) | (p1 ? 2u : 0u);
  LVec y;
  y.x0 = p0 ? s10 : s00; y.x1 = p1 ? s11 : s01;
  return y;
}
__device__ __forceinline__ LVec rv_vmul(const LVec& x, const LMat& m) { unsigned psi; return rv_vmul(x, m, psi); }

__device__ __forceinline__ LMat rv_shfl_up(const LMat& m, int d) {
  LMat o;
  o.a = __shfl_up(m.a, d); o.b = __shfl_up(m.b, d); o.c = __shfl_up(m.c, d); o.d = __shfl_up(m.d, d);
  return o;
}

// Step k of the scan over the m entries at xs (position, score per entry).  Forward: L_k = log T_k + le_k by column, T_0 the identity.
// Backward: the transpose of L_j for j = m - k, the identity at k = 0.  The identity beyond the read.  PRIOR: the share and its logarithms
// are pr[3 j ..], those of the entry arrived at, and q_j = 1 - pi_j is formed here; pr is unread otherwise
template <bool BWD, bool PRIOR>
__device__ __forceinline__ LMat rv_step(const RvArgs& a, const double* xs, const double* pr, int64_t k, int64_t m) {
  const double ninf = -__builtin_huge_val();
  LMat o{0.0, ninf, ninf, 0.0};
  if (k >= m || (BWD && k == 0)) return o;
  const int64_t j = BWD ? m - k : k;
  const double s = xs[2 * j + 1];
  const double le0 = s > 0.0 ? -s : 0.0, le1 = s < 0.0 ? s : 0.0;
  double l00 = 0.0, l01 = ninf, l10 = ninf, l11 = 0.0;
  if (j > 0) {
    const double r = (xs[2 * j] - xs[2 * (j - 1)]) / a.length;
    const double rho = exp(-r), eps = -expm1(-r);
    const double leps = log(eps);                               // three logarithms a step: log(pi eps) = log pi + log eps, and so for q
    double pi = a.pi, q = a.q, lq = a.lq, lpi = a.lpi;
    if constexpr (PRIOR) { pi = pr[3 * j]; q = 1.0 - pi; lq = pr[3 * j + 1]; lpi = pr[3 * j + 2]; }
    l00 = log(q + pi * rho); l01 = lpi + leps; l10 = lq + leps; l11 = log(pi + q * rho);
  }
  if constexpr (BWD) { o.a = l00 + le0; o.b = l10 + le0; o.c = l01 + le1; o.d = l11 + le1; }
  else { o.a = l00 + le0; o.b = l01 + le1; o.c = l10 + le0; o.d = l11 + le1; }
  return o;
}

struct RvShared { LMat tot[kRwWaves]; LVec carry; };

// One tile of the scan, steps k0 .. k0 + T * kHmmChunk - 1, by the T threads of the read: per_entry(k, x, psi) with x the row vector
// after step k and psi its back-pointers, for the steps inside the read.  Returns the vector after the tile's last step (thread T - 1's),
// the same in every thread.  (rh_tile of read_hmm.hip in the other algebra: DESIGN.md §3 K20 says why it is a sibling.)
template <int WAVES, bool BWD, bool PRIOR, class F>
__device__ __forceinline__ LVec rv_tile(const RvArgs& a, const double* xs, const double* pr, int64_t m, int64_t k0, const LVec& carry, RvShared& sh,
                                        F per_entry) {
  constexpr int T = WAVES * 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WAVES == 1 ? lane : (int)threadIdx.x;
  const int64_t kb = k0 + (int64_t)t * kHmmChunk;
  LMat step[kHmmChunk];
#pragma unroll
  for (int c = 0; c < kHmmChunk; ++c) step[c] = rv_step<BWD, PRIOR>(a, xs, pr, kb + c, m);
  LMat prod = step[0];
#pragma unroll
  for (int c = 1; c < kHmmChunk; ++c) prod = rv_mul(prod, step[c]);
  // the inclusive scan over the lanes: steps 1 .. 32, the earlier lanes' product on the left
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const LMat o = rv_shfl_up(prod, d);
    if (lane >= d) prod = rv_mul(o, prod);
  }
  LVec x = carry;
  if constexpr (WAVES > 1) {
    __syncthreads();                                            // the last tile's totals and carry are read
    if (lane == 63) sh.tot[wave] = prod;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < WAVES - 1; ++w) if (w < wave) x = rv_vmul(x, sh.tot[w]);
  }
  const LMat before = rv_shfl_up(prod, 1);
  if (lane > 0) x = rv_vmul(x, before);
#pragma unroll
  for (int c = 0; c < kHmmChunk; ++c) {
    if (kb + c < m) {
      unsigned psi;
      x = rv_vmul(x, step[c], psi);
      per_entry(kb + c, x, psi);
    }
  }
  LVec out;
  if constexpr (WAVES == 1) {
    out.x0 = __shfl(x.x0, 63); out.x1 = __shfl(x.x1, 63);
  } else {
    if (t == T - 1) sh.carry = x;
    __syncthreads();
    out = sh.carry;
  }
  return out;
}

// maps {0, 1} -> {0, 1} as two bits, bit z the image of z: 0 and 3 the constants, 2 the identity, 1 the swap
constexpr unsigned kRvIdentity = 2u;
__device__ __forceinline__ int rv_apply(unsigned f, int z) { return (int)((f >> z) & 1u); }
// first f, then g
__device__ __forceinline__ unsigned rv_compose(unsigned f, unsigned g) { return ((g >> (f & 1u)) & 1u) | (((g >> ((f >> 1) & 1u)) & 1u) << 1); }

template <int WAVES, bool PRIOR>
__global__ __launch_bounds__(kRwThreads) void rv_viterbi_kernel(RvArgs a) {
  __shared__ unsigned sh_item;
  __shared__ int sh_cnt[2 * kRwWaves];
  __shared__ int sh_last[kRwWaves + 1];
  __shared__ unsigned sh_map[kRwWaves];
  __shared__ int sh_z;
  __shared__ double sh_sum[kRwWaves];
  __shared__ RvShared sh_scan;
  const ReadGeom<WAVES> geo;
  const unsigned cnt = a.w.count[geo.CLS];
  const nmod_vit_out& o = a.out;
  for (;;) {
    const unsigned item = draw_read<WAVES>(a.w, sh_item);
    if (item >= cnt) break;
    const int64_t read = (int64_t)a.w.list[geo.CLS][item];
    const int64_t base = a.hoff[read], m = a.hoff[read + 1] - base;
    if (m <= 0 || base < 0 || base > a.nrows - m) {             // no entry (or offsets that are not the rows': skipped)
      if (geo.t == 0) {
        if (o.n_sites) o.n_sites[read] = 0;
        if (o.n_mod) o.n_mod[read] = 0;
        if (o.n_runs) o.n_runs[read] = 0;
        if (o.vit) o.vit[read] = 0.0;
        if (o.status) o.status[read] = NMOD_HMM_NO_SITE;
      }
      continue;
    }
    const double* xs = a.xs + 2 * base;
    const double* pr = PRIOR ? a.share + 3 * base : nullptr;
    double* alpha = a.alpha + 2 * base;
    uint8_t* psi_row = a.psi + base;

    // forward: the vectors, the back-pointers and the sum of the positive scores, a thread's entries in ascending order
    double s_pos = 0.0;
    LVec fw{a.lq, a.lpi};
    if constexpr (PRIOR) { fw.x0 = pr[1]; fw.x1 = pr[2]; }
    for (int64_t k0 = 0; k0 < m; k0 += geo.TS) {
      fw = rv_tile<WAVES, false, PRIOR>(a, xs, pr, m, k0, fw, sh_scan, [&](int64_t k, const LVec& x, unsigned psi) {
        if (a.back) { alpha[2 * k] = x.x0; alpha[2 * k + 1] = x.x1; }
        if (a.trace) psi_row[k] = (uint8_t)psi;
        s_pos += fmax(xs[2 * k + 1], 0.0);
        if (o.site_n) {
          const int64_t s = a.site[base + k];
          if (s >= 0 && s < a.nsites) atomicAdd(&o.site_n[s], 1);
        }
      });
    }
    const double pos = read_sum<WAVES>(s_pos, sh_sum);
    const int z_last = fw.x1 > fw.x0 ? 1 : 0;
    const double vit = (z_last ? fw.x1 : fw.x0) + pos;

    // the rows of the other lanes (waves) are written: both later passes read them
    if constexpr (WAVES > 1) __syncthreads(); else __threadfence_block();

    // traceback: step k is entry m - 1 - k; its map is the constant z_last at k = 0, the back-pointers of entry m - k beyond
    int n_mod = 0, n_runs = 0;
    if (a.trace) {
      int z_in = 0;                                             // the state of the step in front of the tile (none: step 0 is a constant)
      int tile_prev = 2;                                        // the same for the runs (none: not a 1)
      for (int64_t k0 = 0; k0 < m; k0 += geo.TS) {
        const int64_t kb = k0 + (int64_t)geo.t * kHmmChunk;
        unsigned g[kHmmChunk];
#pragma unroll
        for (int c = 0; c < kHmmChunk; ++c) {
          const int64_t k = kb + c;
          g[c] = k >= m ? kRvIdentity : (k == 0 ? (z_last ? 3u : 0u) : (unsigned)psi_row[m - k] & 3u);
        }
        unsigned h = g[0];
#pragma unroll
        for (int c = 1; c < kHmmChunk; ++c) h = rv_compose(h, g[c]);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const unsigned f = (unsigned)__shfl_up((int)h, d);
          if (geo.lane >= d) h = rv_compose(f, h);
        }
        int z = z_in;
        if constexpr (WAVES > 1) {
          __syncthreads();                                      // the last tile's maps, state and run ends are read
          if (geo.lane == 63) sh_map[geo.wave] = h;
          __syncthreads();
#pragma unroll
          for (int w = 0; w < WAVES - 1; ++w) if (w < geo.wave) z = rv_apply(sh_map[w], z);
        }
        const unsigned before = (unsigned)__shfl_up((int)h, 1);
        if (geo.lane > 0) z = rv_apply(before, z);
        int st[kHmmChunk];
#pragma unroll
        for (int c = 0; c < kHmmChunk; ++c) {
          st[c] = 2;
          const int64_t k = kb + c;
          if (k < m) {
            z = rv_apply(g[c], z);
            st[c] = z;
            const int64_t row = base + (m - 1 - k);
            if (o.path) o.path[row] = (uint8_t)z;
            n_mod += z;
            if (o.site_mod && z) {
              const int64_t s = a.site[row];
              if (s >= 0 && s < a.nsites) atomicAdd(&o.site_mod[s], 1);
            }
          }
        }
        // the runs of state 1 by their ends in scan order, as K19 counts them: a step in state 1 whose step before is not
        int last = 2;
#pragma unroll
        for (int c = 0; c < kHmmChunk; ++c) if (kb + c < m) last = st[c];
        int prev = __shfl_up(last, 1);
        if constexpr (WAVES > 1) {
          if (geo.lane == 63) sh_last[geo.wave] = last;
          if (geo.t == geo.T - 1) sh_z = z;
          __syncthreads();
          if (geo.lane == 0 && geo.wave > 0) prev = sh_last[geo.wave - 1];
        }
        if (geo.t == 0) prev = tile_prev;
#pragma unroll
        for (int c = 0; c < kHmmChunk; ++c) {
          if (kb + c < m) { n_runs += st[c] == 1 && prev != 1; prev = st[c]; }
        }
        if constexpr (WAVES == 1) { tile_prev = __shfl(last, 63); z_in = __shfl(z, 63); }
        else { tile_prev = sh_last[WAVES - 1]; z_in = sh_z; }
      }
      read_counts<WAVES>(sh_cnt, n_mod, n_runs);
    }

    // backward, for delta: the same scan over the reversed transposes from (0, 0); step k is entry m - 1 - k
    if (a.back) {
      LVec bw{0.0, 0.0};
      for (int64_t k0 = 0; k0 < m; k0 += geo.TS) {
        bw = rv_tile<WAVES, true, PRIOR>(a, xs, pr, m, k0, bw, sh_scan, [&](int64_t k, const LVec& x, unsigned) {
          const int64_t j = m - 1 - k;
          o.delta[base + j] = (alpha[2 * j + 1] + x.x1) - (alpha[2 * j] + x.x0);
        });
      }
    }
    if (geo.t == 0) {
      if (o.n_sites) o.n_sites[read] = (int32_t)m;
      if (o.n_mod) o.n_mod[read] = n_mod;
      if (o.n_runs) o.n_runs[read] = n_runs;
      if (o.vit) o.vit[read] = vit;
      if (o.status) o.status[read] = 0;
    }
  }
}

}  // namespace nmod

using namespace nmod;

// nmod_read_viterbi (prior false: site_pi unread) and nmod_read_viterbi_prior: one body, the kernel's instances chosen at the launch
static int rv_viterbi_entry(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                            const double* score, int64_t nsites, const int64_t* key, bool prior, const double* site_pi, const int64_t* hoff,
                            int64_t nrows, const nmod_vit_opts* opts, const nmod_vit_out* out) {
  if (!rh_chain_args_ok(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows)) return NMOD_ERR_INVALID_ARG;
  if (prior && nsites > 0 && !site_pi) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_vit_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_vit_out)) return NMOD_ERR_INVALID_ARG;
  if (!rh_chain_opts_ok(opts->pi, opts->length)) return NMOD_ERR_INVALID_ARG;
  ChainCall c(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows, !out->site);
  const size_t nr = c.nr, ns = c.ns, nw = c.nw;
  if (c.host && nreads == 0) {                                  // nothing to enqueue: the site counts of no read
    if (out->site_n) memset(out->site_n, 0, ns * 4);
    if (out->site_mod) memset(out->site_mod, 0, ns * 4);
    return NMOD_OK;
  }
  const int rc = select_device(prm, &c.num_cus);
  if (rc != NMOD_OK) return rc;

  RvArgs a;
  memset(&a, 0, sizeof(a));
  a.nreads = nreads; a.nrows = nrows; a.nsites = nsites;
  a.pi = opts->pi; a.q = 1.0 - opts->pi; a.length = opts->length;
  a.lq = log(a.q); a.lpi = log(a.pi);
  a.out = *out;
  const nmod_vit_out& o = a.out;
  a.trace = o.path || o.n_mod || o.n_runs || o.site_mod;
  a.back = o.delta != nullptr;

  // the call's slab (ChainCall's share: the read lists of both walks, per row the position and the score, and the site where the caller
  // asked for none): the forward vector (delta) and the back-pointers (the path); for the host entry the inputs and outputs as well
  Slab& slab = c.slab;
  const size_t o_alpha = slab.take(a.back ? nw * 16 : 0), o_psi = slab.take(a.trace ? nw : 0);
  if (prior) c.prior(site_pi, opts->pi, 3);
  c.stage();
  slab.out(a.out.path, nw); slab.out(a.out.site, nw * 4); slab.out(a.out.delta, nw * 8);
  slab.out(a.out.n_sites, nr * 4); slab.out(a.out.n_mod, nr * 4); slab.out(a.out.n_runs, nr * 4);
  slab.out(a.out.vit, nr * 8); slab.out(a.out.status, nr);
  slab.out(a.out.site_n, ns * 4); slab.out(a.out.site_mod, ns * 4);
  NMOD_HIP(slab.commit(c.stream, prm->device));
  c.bind(o.site);
  a.hoff = c.e.hoff; a.xs = c.e.xs; a.site = c.e.site; a.alpha = slab.at<double>(o_alpha); a.psi = slab.at<uint8_t>(o_psi);
  a.share = c.share;

  if (o.site_n) NMOD_HIP(hipMemsetAsync(o.site_n, 0, ns * 4, c.stream));
  if (o.site_mod) NMOD_HIP(hipMemsetAsync(o.site_mod, 0, ns * 4, c.stream));
  if (nreads > 0) {
    NMOD_HIP(c.lists(a.w));
    if (prior) rh_launch(a, rv_viterbi_kernel<1, true>, rv_viterbi_kernel<kRwWaves, true>, c.num_cus, c.stream);
    else rh_launch(a, rv_viterbi_kernel<1, false>, rv_viterbi_kernel<kRwWaves, false>, c.num_cus, c.stream);
  }
  return launches_end(slab, c.stream);
}

extern "C" int nmod_read_viterbi(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                 const double* score, int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows,
                                 const nmod_vit_opts* opts, const nmod_vit_out* out) {
  return rv_viterbi_entry(prm, nreads, cs, start, roff, score, nsites, key, false, nullptr, hoff, nrows, opts, out);
}

extern "C" int nmod_read_viterbi_prior(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                       const double* score, int64_t nsites, const int64_t* key, const double* site_pi, const int64_t* hoff,
                                       int64_t nrows, const nmod_vit_opts* opts, const nmod_vit_out* out) {
  return rv_viterbi_entry(prm, nreads, cs, start, roff, score, nsites, key, true, site_pi, hoff, nrows, opts, out);
}
