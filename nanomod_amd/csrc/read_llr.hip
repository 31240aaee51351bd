// nmod_read_llr / nmod_site_llr — per-read log-likelihood ratios between two k-mer models, and their per-position counts, on the
// device (K13).  The reference project has no such step; the definition is the one in include/nanomod_hip.h
// (tests/readllr_ref.py restates it in numpy).  The walk over the reads is read_walk.hpp's, shared with K11 and K12; all on the caller's
// stream:
//   rl_table_kernel      a thread per code: (mu0, sd0, mu1, sd1, g = log(sd0 / sd1)) side by side, sd0 = -1 for an unusable code
//   read_classify_kernel (read_walk.hpp) a thread per read: the read's class by its length, ballot-compacted into one list per class
//   rl_read_kernel<.., 1>  a wave per read of up to NMOD_CALLS_WAVE_MAX events, four waves a workgroup
//   rl_read_kernel<.., 4>  a workgroup of four waves per longer read, a tile of the read per wave and step
//   site_kernel<RlSiteRule>  (read_walk.hpp; nmod_site_llr) a wave per row of pivoted window sums
// A wave stages llr of 512 consecutive events (64 lanes x a run of 8, the code rolled over the run as in K11 / K12) in its own 4 KiB of
// LDS, NaN for an ineligible event; the first 8 ceil(nb_lo / 8) and the last 8 ceil(nb_hi / 8) events of the tile are the window halo,
// recomputed by the neighbouring tiles.  The tile's own events are then taken from the stage, event e on lane e mod 64: llr is the
// staged word itself, the window is summed directly from the staged words in ascending order (no running prefix over the read, for
// K12's reason), and all three tracks leave as contiguous stores.  The grids are persistent and a wave / workgroup draws its next read
// from a ticket word (draw_read, read_walk.hpp).  No float atomics: the counts are integer sums, and a read's bits depend on the read
// alone.  The table (40 bytes per code) lives in LDS up to 256 codes (k <= 4: 10 KiB, sized by the call's own
// code count); beyond it is read through L2: at k = 5 its 40 KiB of LDS would leave two workgroups per CU where the registers allow
// five, and that measured 12 % (k-mer cover) to 32 % ((64, 64)) slower than the L2 path (profiles/read_llr.txt).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "read_walk.hpp"

namespace nmod {

constexpr int kRlTabWords = 5;                    // doubles per code: mu0, sd0, mu1, sd1, g
constexpr int kRlLdsCodes = 256;                  // the table lives in LDS up to here: 40 bytes per code
constexpr size_t kRlLdsPerCu = 160 * 1024;        // gfx950

struct RlArgs {
  const void* val; const uint8_t* base; const int64_t* off; int64_t nreads;
  const double *mean0, *sd0, *mean1, *sd1;        // the two models as given
  double* tab;                                    // kRlTabWords per code
  int32_t k, center, ncodes, nb_lo, nb_hi;
  double thr, prior;
  double *llr, *llr_win, *p_mod; int32_t *n_sites, *n_mod, *n_can; uint8_t* status;
  ReadLists w;
};

__global__ __launch_bounds__(256) void rl_table_kernel(RlArgs a) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.ncodes) return;
  const double mu0 = a.mean0[c], sd0 = a.sd0[c], mu1 = a.mean1[c], sd1 = a.sd1[c];
  const bool ok = fabs(mu0) <= kDblMax && fabs(mu1) <= kDblMax && sd0 > 0.0 && sd0 <= kDblMax && sd1 > 0.0 && sd1 <= kDblMax;
  double* t = a.tab + (size_t)kRlTabWords * c;
  t[0] = ok ? mu0 : 0.0;
  t[1] = ok ? sd0 : -1.0;
  t[2] = ok ? mu1 : 0.0;
  t[3] = ok ? sd1 : 1.0;
  t[4] = ok ? log(sd0 / sd1) : 0.0;
}

// WAVES == 1: a wave per read (list 0), the workgroup's waves independent; else the workgroup per read (list 1)
template <int DT, int WAVES, bool LDS_TAB>
__global__ __launch_bounds__(kRwThreads) void rl_read_kernel(RlArgs a) {
#pragma clang fp contract(off)
  constexpr int CLS = WAVES == 1 ? 0 : 1;
  constexpr int T = WAVES * 64;                                 // threads of a read
  extern __shared__ double lds_tab[];                           // kRlTabWords * ncodes doubles when LDS_TAB, else nothing
  __shared__ double lds_stage[kRwWaves][kRwTile];
  __shared__ int sh_cnt[3 * kRwWaves];
  __shared__ unsigned sh_item;
  const double* tab = a.tab;
  if constexpr (LDS_TAB) {
    for (int c = threadIdx.x; c < kRlTabWords * a.ncodes; c += kRwThreads) lds_tab[c] = a.tab[c];
    tab = lds_tab;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WAVES == 1 ? lane : (int)threadIdx.x;
  double* stage = lds_stage[wave];
  const unsigned cnt = a.w.count[CLS];
  const int k = a.k, center = a.center, nb_lo = a.nb_lo, nb_hi = a.nb_hi;
  const int halo_lo = halo_events(nb_lo), halo_hi = halo_events(nb_hi);
  const int inner = kRwTile - halo_lo - halo_hi;                // the tile's own events (384 .. 512)
  const double thr = a.thr, prior = a.prior, nan = nan_f64();

  for (;;) {
    const unsigned item = draw_read<WAVES>(a.w, sh_item);
    if (item >= cnt) break;
    const int64_t read = (int64_t)a.w.list[CLS][item];
    int64_t begin, n;
    csr_row(a.off, 0, read, begin, n);
    const uint8_t* bs = a.base + begin;

    unsigned st = 0;
    int sites = 0, mod = 0, can = 0;
    if (n > (int64_t)NMOD_MAX_DEEP) {
      st = NMOD_CALLS_TOO_LARGE;
      nan_fill(a.llr, a.llr_win, a.p_mod, begin, n, t, T);
    } else {
      const int64_t ntiles = (n + inner - 1) / inner;
      for (int64_t ti = WAVES == 1 ? 0 : wave; ti < ntiles; ti += WAVES) {
        int64_t a0, s0, a1;                                     // the tile's own events: a0 .. a1 - 1, the staged ones start at s0
        tile_span(ti, inner, halo_lo, n, a0, s0, a1);
        // stage[j - s0] = llr_j, NaN for an ineligible event (0 <= j < n, j - s0 in 0 .. 511; no other word is read below)
        rs_run(bs, n, s0 + (int64_t)kRsRun * lane, k, center, [&](int64_t j, int code) {
          if (j < 0) return;
          double l = nan;
          if (code >= 0) {
            const double* e = tab + kRlTabWords * code;
            const double sd0 = e[1];
            if (sd0 > 0.0) {
              const double x = rs_load<DT>(a.val, begin + j);
              if (fabs(x) <= kDblMax) {
                const double z0 = (x - e[0]) / sd0;
                const double z1 = (x - e[2]) / e[3];
                const double d = 0.5 * ((z0 - z1) * (z0 + z1));
                const double v = e[4] + d;
                if (fabs(v) <= NMOD_LLR_MAX) l = v;
              }
            }
          }
          stage[j - s0] = l;
        });
        wave_lds_sync();
        const int own = (int)(a1 - a0);
        for (int e = lane; e < own; e += 64) {
          const int64_t j = a0 + e;
          const int c = e + halo_lo;                            // j's word of the stage
          const double l = stage[c];
          double S = nan, P = nan;
          if (l == l) {
            if ((nb_lo | nb_hi) == 0) {
              S = l;                                            // no window: L is llr, the same bits
            } else {
              int lo, hi;
              window_bounds(j, n, nb_lo, nb_hi, lo, hi);
              S = 0.0;
              for (int d = lo; d <= hi; ++d) {
                const double v = stage[c + d];
                if (v == v) S += v;
              }
            }
            ++sites;
            mod += S >= thr ? 1 : 0;
            can += S <= -thr ? 1 : 0;
            if (a.p_mod) {
              const double u = S + prior;
              if (u >= 0.0) { P = 1.0 / (1.0 + exp(-u)); } else { const double q = exp(u); P = q / (1.0 + q); }
            }
          }
          if (a.llr) a.llr[begin + j] = l;
          if (a.llr_win) a.llr_win[begin + j] = S;
          if (a.p_mod) a.p_mod[begin + j] = P;
        }
        wave_lds_sync();                                        // the tile is read before the next one is staged
      }
    }
    read_counts<WAVES>(sh_cnt, sites, mod, can);                // the read's counts: integer sums over its threads
    if (t == 0) {
      if (a.n_sites) a.n_sites[read] = sites;
      if (a.n_mod) a.n_mod[read] = mod;
      if (a.n_can) a.n_can[read] = can;
      if (a.status) a.status[read] = (uint8_t)st;
    }
  }
}

struct RlKernels {
  template <int DT, int WAVES, bool LDS_TAB> static auto kernel() { return &rl_read_kernel<DT, WAVES, LDS_TAB>; }
};

template <bool LDS_TAB>
static void rl_launch(const RlArgs& a, int32_t dtype, int num_cus, hipStream_t stream) {
  // workgroups a CU holds: five by the registers (87 .. 98 VGPRs: 5 waves per SIMD), unless the LDS of one — the stage, the counts,
  // and the table of this call — allows fewer (it does not up to kRlLdsCodes: 26 KiB)
  const size_t tab_bytes = LDS_TAB ? (size_t)a.ncodes * kRlTabWords * sizeof(double) : 0;
  const size_t per_group = tab_bytes + sizeof(double) * kRwWaves * kRwTile + 256;
  const int64_t resident = (int64_t)(kRlLdsPerCu / per_group) < 5 ? (int64_t)(kRlLdsPerCu / per_group) : 5;
  launch_read_kernels<RlKernels, LDS_TAB>(a, dtype, (int64_t)num_cus * resident, tab_bytes, stream);
}

// nmod_site_llr's counters: finite sums, sums >= thr, sums <= -thr; frac = n_mod / (n_mod + n_can)
struct RlSiteRule {
  static constexpr int N = 3;
  double thr;
  __device__ void count(double s, unsigned long long (&c)[N]) const {
    c[0] += fabs(s) <= kDblMax ? 1 : 0;
    c[1] += s >= thr ? 1 : 0;
    c[2] += s <= -thr ? 1 : 0;
  }
  __device__ double frac(const unsigned long long (&c)[N]) const { return c[1] + c[2] ? (double)c[1] / (double)(c[1] + c[2]) : nan_f64(); }
};

static bool rl_thr_ok(double thr) { return thr > 0.0 && thr <= kDblMax; }

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_read_llr(const nmod_params* prm, int64_t nreads, const int64_t* off, const void* val, const uint8_t* base,
                             const nmod_rescale_model* model, const nmod_rescale_model* alt, const nmod_llr_opts* opts,
                             const nmod_llr_out* out) {
  if (check_prm_common(prm) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_llr_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_llr_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->nb_lo < 0 || opts->nb_lo > NMOD_MAX_NB || opts->nb_hi < 0 || opts->nb_hi > NMOD_MAX_NB) return NMOD_ERR_INVALID_ARG;
  if (!rl_thr_ok(opts->thr)) return NMOD_ERR_INVALID_ARG;
  if (!(fabs(opts->prior_logit) <= 700.0)) return NMOD_ERR_INVALID_ARG;
  if (!read_count_ok(nreads) || !kmer_model_ok(model)) return NMOD_ERR_INVALID_ARG;
  if (!alt || alt->k != model->k || alt->center != model->center) return NMOD_ERR_INVALID_ARG;
  if (nreads > 0 && (!off || !val || !base || !model->mean || !model->sd || !alt->mean || !alt->sd)) return NMOD_ERR_INVALID_ARG;
  int num_cus = 0;
  const int rc = rows_begin(prm, nreads, off, &num_cus);
  if (rc != NMOD_OK || nreads == 0) return rc;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t nr = (size_t)nreads, esz = elem_bytes(prm->dtype);
  const size_t tot = host ? (size_t)off[nreads] : 0;
  const size_t nc = (size_t)1 << (2 * model->k);

  RlArgs a;
  memset(&a, 0, sizeof(a));
  a.val = val; a.base = base; a.off = off; a.nreads = nreads;
  a.mean0 = model->mean; a.sd0 = model->sd; a.mean1 = alt->mean; a.sd1 = alt->sd;
  a.k = model->k; a.center = model->center; a.ncodes = (int32_t)nc;
  a.nb_lo = opts->nb_lo; a.nb_hi = opts->nb_hi; a.thr = opts->thr; a.prior = opts->prior_logit;
  a.llr = out->llr; a.llr_win = out->llr_win; a.p_mod = out->p_mod;
  a.n_sites = out->n_sites; a.n_mod = out->n_mod; a.n_can = out->n_can; a.status = out->status;

  // one slab: the work lists with their count and ticket words and the table; for the host entry the inputs and outputs as well
  Slab slab(host);
  const ReadListSpace lists(slab, nr);
  const size_t o_tab = slab.take(nc * kRlTabWords * 8);
  slab.in(a.off, (nr + 1) * 8); slab.in(a.val, tot * esz); slab.in(a.base, tot);
  slab.in(a.mean0, nc * 8); slab.in(a.sd0, nc * 8); slab.in(a.mean1, nc * 8); slab.in(a.sd1, nc * 8);
  slab.out(a.llr, tot * 8); slab.out(a.llr_win, tot * 8); slab.out(a.p_mod, tot * 8);
  slab.out(a.n_sites, nr * 4); slab.out(a.n_mod, nr * 4); slab.out(a.n_can, nr * 4); slab.out(a.status, nr);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.tab = slab.at<double>(o_tab);

  NMOD_HIP(lists.fill(slab, a.off, nreads, num_cus, stream, a.w));
  hipLaunchKernelGGL(rl_table_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, a);
  if (a.ncodes <= kRlLdsCodes) rl_launch<true>(a, prm->dtype, num_cus, stream); else rl_launch<false>(a, prm->dtype, num_cus, stream);
  return launches_end(slab, stream);
}

extern "C" int nmod_site_llr(const nmod_params* prm, int64_t npos, const double* score, const int64_t* off, double thr,
                             const nmod_site_llr_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_site_llr_out)) return NMOD_ERR_INVALID_ARG;
  if (!rl_thr_ok(thr)) return NMOD_ERR_INVALID_ARG;
  return site_counts(prm, npos, score, off, RlSiteRule{thr}, SiteOut<RlSiteRule>{{out->n_valid, out->n_mod, out->n_can}, out->frac});
}
