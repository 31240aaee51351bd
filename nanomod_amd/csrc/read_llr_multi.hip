// nmod_read_llr_multi — per-read log-likelihood ratios of one unmodified k-mer table against up to NMOD_MULTI_MAX alternative tables in
// one walk over the reads, with a joint call and a posterior over the states per event (K26).  The reference project has no
// such step; the definition is the one in include/nanomod_hip.h (tests/multi_ref.py restates it in numpy on top of K13's restatement).
// The walk is read_walk.hpp's, shared with K11 .. K13, all on the caller's stream:
//   rm_table_kernel       a thread per code: (mu0, sd0) and per table (mu_m, sd_m, g_m = log(sd0 / sd_m)) side by side; sd0 = -1 where the
//                         unmodified entry is unusable, sd_m = -1 where the pair (model, alt[m-1]) is
//   read_classify_kernel  (read_walk.hpp) the read's class by its length
//   rm_read_kernel<NALT, .., 1>  a wave per read of up to NMOD_CALLS_WAVE_MAX events, four waves a workgroup
//   rm_read_kernel<NALT, .., 4>  a workgroup of four waves per longer read, a tile of the read per wave and step
// Plane m is K13's kernel for the pair (model, alt[m-1]) operation for operation — the same table words, the same expression, the same
// ascending window sum over the staged words — so its bits are nmod_read_llr's; what is shared between the planes is read or computed
// once per event: the value, the rolled code, z0 and the tile geometry.  A wave stages NALT x 512 llr words (NALT x 4 KiB) per tile; the
// joint call, the posterior and the counts are taken from the NALT window sums of an event while they are in registers.  No float
// atomics: the counts are integer sums by read_counts, and a read's bits depend on the read alone.
// Table placement.  A row is 2 + 3 NALT doubles per code.  The stage costs NALT x 16 KiB of LDS per workgroup, which alone bounds the
// workgroups a CU holds (160 KiB) at 5 (by kRmRegGroups), 4, 3 and 2 for NALT = 1 .. 4; the table goes to LDS iff adding its bytes to
// the workgroup leaves that number unchanged (table_in_lds below), and is read through L2 otherwise.  With k-mer tables of 4^k codes
// that is: NALT = 1: k <= 4 in LDS (K13's switch, and K13's measurement: at k = 5 the LDS form lost 12 % to 32 %); NALT = 2: k <= 3;
// NALT = 3: k <= 2 (at k = 3 its 5.5 KiB would take the CU from three workgroups to two); NALT = 4: k <= 3.
// MEASURED (profiles/read_llr_multi.txt; MI355X, 20 M int16 events, k-mer cover, llr_win + call against n_alt separate nmod_read_llr calls
// for llr_win, alternated): k = 3 (LDS) 1.19 x faster at n_alt = 2 and 1.31 x at 4; k = 5 (L2) 1.28 x and 1.22 x; planes bit-equal.
// NOT measured: either case with the other placement — the rule is K13's finding (residency first) applied to the bytes of the call, not
// a timing of this kernel — nor other windows and dtypes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "read_walk.hpp"

namespace nmod {

constexpr size_t kRmLdsPerCu = 160 * 1024;        // gfx950
constexpr int kRmRegGroups = 5;                   // workgroups a CU holds by the registers at most (K13's figure; more tables only lower it)
constexpr int kRmCounts = 2 + NMOD_MULTI_MAX;     // sites, can, mod[0 .. 3]

__host__ __device__ constexpr int rm_tab_words(int nalt) { return 2 + 3 * nalt; }

struct RmArgs {
  const void* val; const uint8_t* base; const int64_t* off; int64_t nreads, total;
  const double *mean0, *sd0, *mean1[NMOD_MULTI_MAX], *sd1[NMOD_MULTI_MAX];
  double* tab;                                    // rm_tab_words(n_alt) per code
  int32_t k, center, ncodes, nb_lo, nb_hi, n_alt;
  double thr, prior[NMOD_MULTI_MAX];
  double *llr, *llr_win, *post; uint8_t* call;    // n_alt, n_alt, n_alt + 1 planes of `total` events; one byte per event
  int32_t *n_sites, *n_can, *n_mod; uint8_t* status;   // n_mod: n_alt planes of nreads
  ReadLists w;
};

__global__ __launch_bounds__(256) void rm_table_kernel(RmArgs a) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.ncodes) return;
  const double mu0 = a.mean0[c], sd0 = a.sd0[c];
  const bool ok0 = fabs(mu0) <= kDblMax && sd0 > 0.0 && sd0 <= kDblMax;
  double* t = a.tab + (size_t)rm_tab_words(a.n_alt) * c;
  t[0] = ok0 ? mu0 : 0.0;
  t[1] = ok0 ? sd0 : -1.0;
  for (int m = 0; m < a.n_alt; ++m) {
    const double mu1 = a.mean1[m][c], sd1 = a.sd1[m][c];
    const bool ok = ok0 && fabs(mu1) <= kDblMax && sd1 > 0.0 && sd1 <= kDblMax;
    t[2 + 3 * m] = ok ? mu1 : 0.0;
    t[3 + 3 * m] = ok ? sd1 : -1.0;
    t[4 + 3 * m] = ok ? log(sd0 / sd1) : 0.0;
  }
}

// WAVES == 1: a wave per read (list 0), the workgroup's waves independent; else the workgroup per read (list 1)
template <int NALT, int DT, int WAVES, bool LDS_TAB>
__global__ __launch_bounds__(kRwThreads) void rm_read_kernel(RmArgs a) {
#pragma clang fp contract(off)
  constexpr int CLS = WAVES == 1 ? 0 : 1;
  constexpr int T = WAVES * 64;                                 // threads of a read
  constexpr int TW = rm_tab_words(NALT);
  extern __shared__ double lds_tab[];                           // TW * ncodes doubles when LDS_TAB, else nothing
  __shared__ double lds_stage[kRwWaves][NALT][kRwTile];
  __shared__ int sh_cnt[kRmCounts * kRwWaves];
  __shared__ unsigned sh_item;
  const double* tab = a.tab;
  if constexpr (LDS_TAB) {
    for (int c = threadIdx.x; c < TW * a.ncodes; c += kRwThreads) lds_tab[c] = a.tab[c];
    tab = lds_tab;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WAVES == 1 ? lane : (int)threadIdx.x;
  double (*stage)[kRwTile] = lds_stage[wave];
  const unsigned cnt = a.w.count[CLS];
  const int k = a.k, center = a.center, nb_lo = a.nb_lo, nb_hi = a.nb_hi;
  const int halo_lo = halo_events(nb_lo), halo_hi = halo_events(nb_hi);
  const int inner = kRwTile - halo_lo - halo_hi;                // the tile's own events (384 .. 512)
  const double thr = a.thr, nan = nan_f64();
  const int64_t total = a.total;

  for (;;) {
    const unsigned item = draw_read<WAVES>(a.w, sh_item);
    if (item >= cnt) break;
    const int64_t read = (int64_t)a.w.list[CLS][item];
    int64_t begin, n;
    csr_row(a.off, 0, read, begin, n);
    const uint8_t* bs = a.base + begin;

    unsigned st = 0;
    int sites = 0, can = 0, mod[NMOD_MULTI_MAX] = {0, 0, 0, 0};
    if (n > (int64_t)NMOD_MAX_DEEP) {
      st = NMOD_CALLS_TOO_LARGE;
      for (int64_t j = t; j < n; j += T) {
#pragma unroll
        for (int m = 0; m < NALT; ++m) {
          if (a.llr) a.llr[m * total + begin + j] = nan;
          if (a.llr_win) a.llr_win[m * total + begin + j] = nan;
        }
        if (a.post) {
#pragma unroll
          for (int m = 0; m <= NALT; ++m) a.post[m * total + begin + j] = nan;
        }
        if (a.call) a.call[begin + j] = (uint8_t)NMOD_MULTI_NONE;
      }
    } else {
      const int64_t ntiles = (n + inner - 1) / inner;
      for (int64_t ti = WAVES == 1 ? 0 : wave; ti < ntiles; ti += WAVES) {
        int64_t a0, s0, a1;                                     // the tile's own events: a0 .. a1 - 1, the staged ones start at s0
        tile_span(ti, inner, halo_lo, n, a0, s0, a1);
        // stage[m][j - s0] = llr_j of plane m, NaN for an ineligible event (0 <= j < n, j - s0 in 0 .. 511; no other word is read below)
        rs_run(bs, n, s0 + (int64_t)kRsRun * lane, k, center, [&](int64_t j, int code) {
          if (j < 0) return;
          double l[NALT];
#pragma unroll
          for (int m = 0; m < NALT; ++m) l[m] = nan;
          if (code >= 0) {
            const double* e = tab + TW * code;
            const double sd0 = e[1];
            if (sd0 > 0.0) {
              const double x = rs_load<DT>(a.val, begin + j);
              if (fabs(x) <= kDblMax) {
                const double z0 = (x - e[0]) / sd0;
#pragma unroll
                for (int m = 0; m < NALT; ++m) {
                  const double sd1 = e[3 + 3 * m];
                  if (sd1 > 0.0) {
                    const double z1 = (x - e[2 + 3 * m]) / sd1;
                    const double d = 0.5 * ((z0 - z1) * (z0 + z1));
                    const double v = e[4 + 3 * m] + d;
                    if (fabs(v) <= NMOD_LLR_MAX) l[m] = v;
                  }
                }
              }
            }
          }
#pragma unroll
          for (int m = 0; m < NALT; ++m) stage[m][j - s0] = l[m];
        });
        wave_lds_sync();
        const int own = (int)(a1 - a0);
        for (int e = lane; e < own; e += 64) {
          const int64_t j = a0 + e;
          const int c = e + halo_lo;                            // j's word of the stage
          double L[NALT];
          unsigned open = 0;
#pragma unroll
          for (int m = 0; m < NALT; ++m) {
            const double l = stage[m][c];
            double S = nan;
            if (l == l) {
              if ((nb_lo | nb_hi) == 0) {
                S = l;                                          // no window: L is llr, the same bits
              } else {
                int lo, hi;
                window_bounds(j, n, nb_lo, nb_hi, lo, hi);
                S = 0.0;
                for (int d = lo; d <= hi; ++d) {
                  const double v = stage[m][c + d];
                  if (v == v) S += v;
                }
              }
              open |= 1u << m;
            }
            L[m] = S;
            if (a.llr) a.llr[m * total + begin + j] = l;
            if (a.llr_win) a.llr_win[m * total + begin + j] = S;
          }
          unsigned call = NMOD_MULTI_NONE;
          if (open) {
            int b = -1;
            double Lb = 0.0;
#pragma unroll
            for (int m = 0; m < NALT; ++m)
              if ((open >> m & 1u) && (b < 0 || L[m] > Lb)) { b = m; Lb = L[m]; }
            double second = 0.0;
            bool all_can = true;
#pragma unroll
            for (int m = 0; m < NALT; ++m)
              if (open >> m & 1u) {
                if (m != b && L[m] > second) second = L[m];
                all_can = all_can && L[m] <= -thr;
              }
            call = Lb - second >= thr ? (unsigned)(b + 1) : (all_can ? 0u : (unsigned)NMOD_MULTI_AMBIGUOUS);
            ++sites;
            can += call == 0u ? 1 : 0;
#pragma unroll
            for (int m = 0; m < NALT; ++m) mod[m] += call == (unsigned)(m + 1) ? 1 : 0;
          }
          if (a.call) a.call[begin + j] = (uint8_t)call;
          if (a.post) {
            double P[NALT + 1];
#pragma unroll
            for (int m = 0; m <= NALT; ++m) P[m] = nan;
            if (open) {
              double u[NALT], mx = 0.0;
#pragma unroll
              for (int m = 0; m < NALT; ++m) {
                u[m] = L[m] + a.prior[m];
                if ((open >> m & 1u) && u[m] > mx) mx = u[m];
              }
              P[0] = exp(-mx);
              double Z = P[0];
#pragma unroll
              for (int m = 0; m < NALT; ++m) {
                P[m + 1] = 0.0;
                if (open >> m & 1u) { P[m + 1] = exp(u[m] - mx); Z += P[m + 1]; }
              }
#pragma unroll
              for (int m = 0; m <= NALT; ++m) P[m] = P[m] / Z;
            }
#pragma unroll
            for (int m = 0; m <= NALT; ++m) a.post[m * total + begin + j] = P[m];
          }
        }
        wave_lds_sync();                                        // the tile is read before the next one is staged
      }
    }
    read_counts<WAVES>(sh_cnt, sites, can, mod[0], mod[1], mod[2], mod[3]);   // the read's counts: integer sums over its threads
    if (t == 0) {
      if (a.n_sites) a.n_sites[read] = sites;
      if (a.n_can) a.n_can[read] = can;
      if (a.n_mod) {
#pragma unroll
        for (int m = 0; m < NALT; ++m) a.n_mod[m * a.nreads + read] = mod[m];
      }
      if (a.status) a.status[read] = (uint8_t)st;
    }
  }
}

template <int NALT>
struct RmKernels {
  template <int DT, int WAVES, bool LDS_TAB> static auto kernel() { return &rm_read_kernel<NALT, DT, WAVES, LDS_TAB>; }
};

// LDS of a workgroup without the table: the stage, the counts and the ticket word
static size_t rm_group_bytes(int nalt) { return sizeof(double) * kRwWaves * kRwTile * (size_t)nalt + 256; }
static int64_t rm_resident(size_t per_group) {
  const int64_t by_lds = (int64_t)(kRmLdsPerCu / per_group);
  return by_lds < kRmRegGroups ? by_lds : kRmRegGroups;
}
// the table lives in LDS iff its bytes do not lower the workgroups a CU holds
static bool table_in_lds(int nalt, size_t ncodes) {
  const size_t tab_bytes = ncodes * rm_tab_words(nalt) * sizeof(double);
  return rm_resident(rm_group_bytes(nalt) + tab_bytes) >= rm_resident(rm_group_bytes(nalt));
}

template <int NALT>
static void rm_launch(const RmArgs& a, int32_t dtype, int num_cus, hipStream_t stream) {
  const bool lds = table_in_lds(NALT, (size_t)a.ncodes);
  const size_t tab_bytes = lds ? (size_t)a.ncodes * rm_tab_words(NALT) * sizeof(double) : 0;
  const int64_t cap = (int64_t)num_cus * rm_resident(rm_group_bytes(NALT) + tab_bytes);
  if (lds) launch_read_kernels<RmKernels<NALT>, true>(a, dtype, cap, tab_bytes, stream);
  else launch_read_kernels<RmKernels<NALT>, false>(a, dtype, cap, 0, stream);
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_read_llr_multi_table_in_lds(int32_t n_alt, int32_t k) {
  if (n_alt < 1 || n_alt > NMOD_MULTI_MAX || k < 1 || k > 8) return -1;
  return table_in_lds(n_alt, (size_t)1 << (2 * k)) ? 1 : 0;
}

extern "C" int nmod_read_llr_multi(const nmod_params* prm, int64_t nreads, int64_t total_events, const int64_t* off, const void* val,
                                   const uint8_t* base, const nmod_rescale_model* model, int32_t n_alt, const nmod_rescale_model* const* alt,
                                   const nmod_llr_multi_opts* opts, const nmod_llr_multi_out* out) {
  if (check_prm_common(prm) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_llr_multi_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_llr_multi_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->nb_lo < 0 || opts->nb_lo > NMOD_MAX_NB || opts->nb_hi < 0 || opts->nb_hi > NMOD_MAX_NB) return NMOD_ERR_INVALID_ARG;
  if (!(opts->thr > 0.0 && opts->thr <= kDblMax)) return NMOD_ERR_INVALID_ARG;
  if (n_alt < 1 || n_alt > NMOD_MULTI_MAX || !alt) return NMOD_ERR_INVALID_ARG;
  for (int m = 0; m < n_alt; ++m) if (!(fabs(opts->prior_logit[m]) <= 700.0)) return NMOD_ERR_INVALID_ARG;
  if (!read_count_ok(nreads) || !kmer_model_ok(model) || total_events < 0) return NMOD_ERR_INVALID_ARG;
  for (int m = 0; m < n_alt; ++m) {
    if (!alt[m] || alt[m]->k != model->k || alt[m]->center != model->center) return NMOD_ERR_INVALID_ARG;
    if (nreads > 0 && (!alt[m]->mean || !alt[m]->sd)) return NMOD_ERR_INVALID_ARG;
  }
  if (nreads > 0 && (!off || !val || !base || !model->mean || !model->sd)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && nreads > 0 && (!csr_offsets_ok(off, nreads) || off[nreads] > total_events)) return NMOD_ERR_INVALID_ARG;
  int num_cus = 0;
  const int rc = rows_begin(prm, nreads, off, &num_cus);
  if (rc != NMOD_OK || nreads == 0) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t nr = (size_t)nreads, esz = elem_bytes(prm->dtype);
  const size_t tot = host ? (size_t)off[nreads] : 0;            // events the host call copies in
  const size_t plane = host ? (size_t)total_events : 0;
  const size_t nc = (size_t)1 << (2 * model->k), na = (size_t)n_alt;

  RmArgs a;
  memset(&a, 0, sizeof(a));
  a.val = val; a.base = base; a.off = off; a.nreads = nreads; a.total = total_events;
  a.mean0 = model->mean; a.sd0 = model->sd;
  for (int m = 0; m < n_alt; ++m) { a.mean1[m] = alt[m]->mean; a.sd1[m] = alt[m]->sd; a.prior[m] = opts->prior_logit[m]; }
  a.k = model->k; a.center = model->center; a.ncodes = (int32_t)nc; a.n_alt = n_alt;
  a.nb_lo = opts->nb_lo; a.nb_hi = opts->nb_hi; a.thr = opts->thr;
  a.llr = out->llr; a.llr_win = out->llr_win; a.post = out->post; a.call = out->call;
  a.n_sites = out->n_sites; a.n_can = out->n_can; a.n_mod = out->n_mod; a.status = out->status;

  // one slab: the work lists with their count and ticket words and the table; for the host entry the inputs and outputs as well
  Slab slab(host);
  const ReadListSpace lists(slab, nr);
  const size_t o_tab = slab.take(nc * rm_tab_words(n_alt) * 8);
  slab.in(a.off, (nr + 1) * 8); slab.in(a.val, tot * esz); slab.in(a.base, tot);
  slab.in(a.mean0, nc * 8); slab.in(a.sd0, nc * 8);
  for (int m = 0; m < n_alt; ++m) { slab.in(a.mean1[m], nc * 8); slab.in(a.sd1[m], nc * 8); }
  slab.out(a.llr, na * plane * 8); slab.out(a.llr_win, na * plane * 8); slab.out(a.post, (na + 1) * plane * 8); slab.out(a.call, plane);
  slab.out(a.n_sites, nr * 4); slab.out(a.n_can, nr * 4); slab.out(a.n_mod, na * nr * 4); slab.out(a.status, nr);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.tab = slab.at<double>(o_tab);

  NMOD_HIP(lists.fill(slab, a.off, nreads, num_cus, stream, a.w));
  hipLaunchKernelGGL(rm_table_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, a);
  switch (n_alt) {
    case 1: rm_launch<1>(a, prm->dtype, num_cus, stream); break;
    case 2: rm_launch<2>(a, prm->dtype, num_cus, stream); break;
    case 3: rm_launch<3>(a, prm->dtype, num_cus, stream); break;
    default: rm_launch<4>(a, prm->dtype, num_cus, stream); break;
  }
  return launches_end(slab, stream);
}
