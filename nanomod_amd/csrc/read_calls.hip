// nmod_read_calls / nmod_site_calls — per-read modification calls against a k-mer model, and their per-position counts, on the device
// (K12).  The reference project has no such step; the definition is the one in include/nanomod_hip.h
// (tests/readcalls_ref.py restates it in numpy).  The walk over the reads is read_walk.hpp's, shared with K11 and K13; all on the caller's
// stream:
//   rc_table_kernel      a thread per code: the model as (mu, sd) with sd = -1 for an entry that makes its events ineligible
//   read_classify_kernel (read_walk.hpp) a thread per read: the read's class by its length, ballot-compacted into one list per class
//   rc_read_kernel<.., 1>  a wave per read of up to NMOD_CALLS_WAVE_MAX events, four waves a workgroup
//   rc_read_kernel<.., 4>  a workgroup of four waves per longer read, a tile of the read per wave and step
//   site_kernel<RcSiteRule>  (read_walk.hpp; nmod_site_calls) a wave per row of pivoted scores
// Both read forms are one function, and a wave works alone in both until the read's counts are summed.  A wave stages the log tails l of
// 512 consecutive events (64 lanes x a run of 8, the 2-bit code rolled over the run's bases and a k - 1 byte halo as in K11) in its own
// 4 KiB of LDS; the first and last ceil(nb / 8) runs of the tile are the window halo, recomputed by the neighbouring tiles, and the
// events between them are the tile's own: their z and p are stored from the runs, their windows summed directly from the staged l in
// ascending order, event e of the tile on lane e mod 64 (consecutive lanes: consecutive LDS words and one contiguous store).  No
// running prefix over the read: with |l| up to 1e3 and 1e5 .. 1e6 events the difference of two prefixes would not keep 1e-9 of a
// window's sum.  The grids are persistent; a wave / workgroup draws its next read with one returning atomic on a ticket word
// (draw_read, read_walk.hpp).  No float atomics: the counts are integer sums, and a read's bits
// depend on the read alone — its class comes from its length — not on the batch, the list order, the memspace or the outputs asked for.
// The table lives in LDS up to 1 024 codes (k <= 5: 16 KiB); beyond it is read through L2.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "read_walk.hpp"

namespace nmod {

constexpr int kRcLdsCodes = 1024;                 // the table lives in LDS up to here: 16 bytes per code

struct RcArgs {
  const void* val; const uint8_t* base; const int64_t* off; int64_t nreads;
  const double* mean; const double* sd;           // the model as given
  double* tab;                                    // mu[ncodes], sd[ncodes] (-1: ineligible)
  int32_t k, center, ncodes, nb;
  double alpha;
  double *z, *p, *p_win; int32_t *n_sites, *n_called; uint8_t* status;
  ReadLists w;
};

__global__ __launch_bounds__(256) void rc_table_kernel(RcArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.ncodes) return;
  const double mu = a.mean[c], sd = a.sd[c];
  const bool ok = fabs(mu) <= kDblMax && sd > 0.0 && sd <= kDblMax;
  a.tab[c] = ok ? mu : 0.0;
  a.tab[a.ncodes + c] = ok ? sd : -1.0;
}

// WAVES == 1: a wave per read (list 0), the workgroup's waves independent; else the workgroup per read (list 1)
template <int DT, int WAVES, bool LDS_TAB>
__global__ __launch_bounds__(kRwThreads) void rc_read_kernel(RcArgs a) {
#pragma clang fp contract(off)
  constexpr int CLS = WAVES == 1 ? 0 : 1;
  constexpr int T = WAVES * 64;                                 // threads of a read
  __shared__ double lds_tab[LDS_TAB ? 2 * kRcLdsCodes : 1];
  __shared__ double lds_stage[kRwWaves][kRwTile];
  __shared__ int sh_cnt[2 * kRwWaves];
  __shared__ unsigned sh_item;
  const int nc = a.ncodes;
  const double* tmu = a.tab; const double* tsd = a.tab + nc;
  if constexpr (LDS_TAB) {
    for (int c = threadIdx.x; c < 2 * nc; c += kRwThreads) lds_tab[c] = a.tab[c];
    tmu = lds_tab; tsd = lds_tab + nc;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WAVES == 1 ? lane : (int)threadIdx.x;
  double* stage = lds_stage[wave];
  const unsigned cnt = a.w.count[CLS];
  const int k = a.k, center = a.center, nb = a.nb;
  const int halo = halo_events(nb);                             // the same on each side
  const int inner = kRwTile - 2 * halo;                         // the tile's own events (384 .. 512)
  const double alpha = a.alpha, nan = nan_f64();

  for (;;) {
    const unsigned item = draw_read<WAVES>(a.w, sh_item);
    if (item >= cnt) break;
    const int64_t read = (int64_t)a.w.list[CLS][item];
    int64_t begin, n;
    csr_row(a.off, 0, read, begin, n);
    const uint8_t* bs = a.base + begin;

    unsigned st = 0;
    int sites = 0, called = 0;
    if (n > (int64_t)NMOD_MAX_DEEP) {
      st = NMOD_CALLS_TOO_LARGE;
      nan_fill(a.z, a.p, a.p_win, begin, n, t, T);
    } else {
      const int64_t ntiles = (n + inner - 1) / inner;
      for (int64_t ti = WAVES == 1 ? 0 : wave; ti < ntiles; ti += WAVES) {
        int64_t a0, s0, a1;                                     // the tile's own events: a0 .. a1 - 1, the staged ones start at s0
        tile_span(ti, inner, halo, n, a0, s0, a1);
        // the tails of the staged events: stage[j - s0] = l_j, NaN for an ineligible event (0 <= j < n; no other word is read below)
        rs_run(bs, n, s0 + (int64_t)kRsRun * lane, k, center, [&](int64_t j, int code) {
          if (j < 0) return;
          double z = nan, p = nan, l = nan;
          if (code >= 0) {
            const double sd = tsd[code];
            if (sd > 0.0) {
              const double x = rs_load<DT>(a.val, begin + j);
              if (fabs(x) <= kDblMax) {
                z = (x - tmu[code]) / sd;
                const double u = fabs(z) * kInvSqrt2;
                p = clamp_p(erfc(u));
                l = log(erfcx(u)) - u * u;
              }
            }
          }
          stage[j - s0] = l;
          if (j >= a0 && j < a1) {
            if (a.z) a.z[begin + j] = z;
            if (a.p) a.p[begin + j] = p;
            if (nb == 0) {                                      // no window: P is p, the same bits
              if (a.p_win) a.p_win[begin + j] = p;
              sites += l == l ? 1 : 0;
              called += p <= alpha ? 1 : 0;
            }
          }
        });
        if (nb > 0) {
          wave_lds_sync();
          const int own = (int)(a1 - a0);
          for (int e = lane; e < own; e += 64) {
            const int64_t j = a0 + e;
            const int c = e + halo;                             // j's word of the stage
            double P = nan;
            if (stage[c] == stage[c]) {
              int lo, hi, W = 0;
              window_bounds(j, n, nb, nb, lo, hi);
              double S = 0.0;
              for (int d = lo; d <= hi; ++d) {
                const double l = stage[c + d];
                if (l == l) { ++W; S += l; }
              }
              P = clamp_p(chi2_sf_even(-2.0 * S, W));
              ++sites;
              called += P <= alpha ? 1 : 0;
            }
            if (a.p_win) a.p_win[begin + j] = P;
          }
          wave_lds_sync();                                      // the tile is read before the next one is staged
        }
      }
    }
    read_counts<WAVES>(sh_cnt, sites, called);                  // the read's counts: integer sums over its threads
    if (t == 0) {
      if (a.n_sites) a.n_sites[read] = sites;
      if (a.n_called) a.n_called[read] = called;
      if (a.status) a.status[read] = (uint8_t)st;
    }
  }
}

struct RcKernels {
  template <int DT, int WAVES, bool LDS_TAB> static auto kernel() { return &rc_read_kernel<DT, WAVES, LDS_TAB>; }
};

// nmod_site_calls' counters: scores in [0, 1], those of them <= alpha; frac = n_called / n_valid
struct RcSiteRule {
  static constexpr int N = 2;
  double alpha;
  __device__ void count(double s, unsigned long long (&c)[N]) const {
    const bool ok = s >= 0.0 && s <= 1.0;
    c[0] += ok ? 1 : 0;
    c[1] += ok && s <= alpha ? 1 : 0;
  }
  __device__ double frac(const unsigned long long (&c)[N]) const { return c[0] ? (double)c[1] / (double)c[0] : nan_f64(); }
};

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_read_calls(const nmod_params* prm, int64_t nreads, const int64_t* off, const void* val, const uint8_t* base,
                               const nmod_rescale_model* model, const nmod_calls_opts* opts, const nmod_calls_out* out) {
  if (check_prm_common(prm) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_calls_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_calls_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->nb < 0 || opts->nb > NMOD_MAX_NB) return NMOD_ERR_INVALID_ARG;
  if (!(opts->alpha > 0.0 && opts->alpha <= 1.0)) return NMOD_ERR_INVALID_ARG;
  if (!read_count_ok(nreads) || !kmer_model_ok(model)) return NMOD_ERR_INVALID_ARG;
  if (nreads > 0 && (!off || !val || !base || !model->mean || !model->sd)) return NMOD_ERR_INVALID_ARG;
  int num_cus = 0;
  const int rc = rows_begin(prm, nreads, off, &num_cus);
  if (rc != NMOD_OK || nreads == 0) return rc;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t nr = (size_t)nreads, esz = elem_bytes(prm->dtype);
  const size_t tot = host ? (size_t)off[nreads] : 0;
  const size_t nc = (size_t)1 << (2 * model->k);

  RcArgs a;
  memset(&a, 0, sizeof(a));
  a.val = val; a.base = base; a.off = off; a.nreads = nreads;
  a.mean = model->mean; a.sd = model->sd; a.k = model->k; a.center = model->center; a.ncodes = (int32_t)nc;
  a.nb = opts->nb; a.alpha = opts->alpha;
  a.z = out->z; a.p = out->p; a.p_win = out->p_win; a.n_sites = out->n_sites; a.n_called = out->n_called; a.status = out->status;

  // one slab: the work lists with their count and ticket words and the table; for the host entry the inputs and outputs as well
  Slab slab(host);
  const ReadListSpace lists(slab, nr);
  const size_t o_tab = slab.take(nc * 16);
  slab.in(a.off, (nr + 1) * 8); slab.in(a.val, tot * esz); slab.in(a.base, tot); slab.in(a.mean, nc * 8); slab.in(a.sd, nc * 8);
  slab.out(a.z, tot * 8); slab.out(a.p, tot * 8); slab.out(a.p_win, tot * 8);
  slab.out(a.n_sites, nr * 4); slab.out(a.n_called, nr * 4); slab.out(a.status, nr);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.tab = slab.at<double>(o_tab);

  NMOD_HIP(lists.fill(slab, a.off, nreads, num_cus, stream, a.w));
  hipLaunchKernelGGL(rc_table_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, a);
  // (the fp64 tails keep 256 VGPRs and some AGPRs live: one workgroup per CU is resident; a second one in the grid only shortens the tail)
  const int64_t cap = (int64_t)num_cus * 2;
  if (a.ncodes <= kRcLdsCodes) launch_read_kernels<RcKernels, true>(a, prm->dtype, cap, 0, stream);
  else launch_read_kernels<RcKernels, false>(a, prm->dtype, cap, 0, stream);
  return launches_end(slab, stream);
}

extern "C" int nmod_site_calls(const nmod_params* prm, int64_t npos, const double* score, const int64_t* off, double alpha,
                               const nmod_site_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_site_out)) return NMOD_ERR_INVALID_ARG;
  if (!(alpha > 0.0 && alpha <= 1.0)) return NMOD_ERR_INVALID_ARG;
  return site_counts(prm, npos, score, off, RcSiteRule{alpha}, SiteOut<RcSiteRule>{{out->n_valid, out->n_called}, out->frac});
}
