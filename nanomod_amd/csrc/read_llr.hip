// nmod_read_llr / nmod_site_llr — per-read log-likelihood ratios between two k-mer models, and their per-position counts, on the
// device (K13).  The reference project has no such step; the definition is the one in include/nanomod_hip.h
// (tests/readllr_ref.py restates it in numpy).  K12's skeleton, all on the caller's stream:
//   rl_table_kernel      a thread per code: (mu0, sd0, mu1, sd1, g = log(sd0 / sd1)) side by side, sd0 = -1 for an unusable code
//   rl_classify_kernel   a thread per read: the read's class by its length, ballot-compacted into one list per class
//   rl_read_kernel<.., 1>  a wave per read of up to NMOD_CALLS_WAVE_MAX events, four waves a workgroup
//   rl_read_kernel<.., 4>  a workgroup of four waves per longer read, a tile of the read per wave and step
//   rl_site_kernel       (nmod_site_llr) a wave per row of pivoted window sums
// A wave stages llr of 512 consecutive events (64 lanes x a run of 8, the code rolled over the run as in K11 / K12) in its own 4 KiB of
// LDS, NaN for an ineligible event; the first 8 ceil(nb_lo / 8) and the last 8 ceil(nb_hi / 8) events of the tile are the window halo,
// recomputed by the neighbouring tiles.  The tile's own events are then taken from the stage, event e on lane e mod 64: llr is the
// staged word itself, the window is summed directly from the staged words in ascending order (no running prefix over the read, for
// K12's reason), and all three tracks leave as contiguous stores.  The grids are persistent and a wave / workgroup draws its next read
// from a ticket word, every lane taking part in the draw.  No float atomics: the counts are integer sums, and a read's
// bits depend on the read alone.  The table (40 bytes per code) lives in LDS up to 256 codes (k <= 4: 10 KiB, sized by the call's own
// code count); beyond it is read through L2: at k = 5 its 40 KiB of LDS would leave two workgroups per CU where the registers allow
// five, and that measured 12 % (k-mer cover) to 32 % ((64, 64)) slower than the L2 path (profiles/read_llr.txt).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "entry_device.hpp"
#include "read_events.hpp"
#include "special_math.hpp"

namespace nmod {

constexpr int kRlThreads = 256;
constexpr int kRlWaves = kRlThreads / 64;
constexpr int kRlTile = 64 * kRsRun;              // events a wave stages at a time
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
  uint32_t* list[2]; uint32_t* count;             // count[0 .. 1]: the lists' lengths, count[2 .. 3]: their ticket words
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

__global__ __launch_bounds__(256) void rl_classify_kernel(RlArgs a) {
  const int lane = threadIdx.x & 63;
  for (int64_t b0 = (int64_t)blockIdx.x * 256; b0 < a.nreads; b0 += (int64_t)gridDim.x * 256) {
    const int64_t i = b0 + threadIdx.x;
    int cls = -1;
    if (i < a.nreads) {
      int64_t b, n;
      csr_row(a.off, 0, i, b, n);
      cls = n <= NMOD_CALLS_WAVE_MAX ? 0 : 1;
    }
    compact_to_lists<2>(cls, lane, a.list, a.count, i);
  }
}

// the stores of a wave to its LDS tile are visible to its own later loads, and the other way round
__device__ __forceinline__ void rl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// WAVES == 1: a wave per read (list 0), the workgroup's waves independent; else the workgroup per read (list 1)
template <int DT, int WAVES, bool LDS_TAB>
__global__ __launch_bounds__(kRlThreads) void rl_read_kernel(RlArgs a) {
#pragma clang fp contract(off)
  constexpr int CLS = WAVES == 1 ? 0 : 1;
  constexpr int T = WAVES * 64;                                 // threads of a read
  extern __shared__ double lds_tab[];                           // kRlTabWords * ncodes doubles when LDS_TAB, else nothing
  __shared__ double lds_stage[kRlWaves][kRlTile];
  __shared__ int sh_cnt[3 * kRlWaves];
  __shared__ unsigned sh_item;
  const double* tab = a.tab;
  if constexpr (LDS_TAB) {
    for (int c = threadIdx.x; c < kRlTabWords * a.ncodes; c += kRlThreads) lds_tab[c] = a.tab[c];
    tab = lds_tab;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WAVES == 1 ? lane : (int)threadIdx.x;
  double* stage = lds_stage[wave];
  const unsigned cnt = a.count[CLS];
  const int k = a.k, center = a.center, nb_lo = a.nb_lo, nb_hi = a.nb_hi;
  const int halo_lo = kRsRun * ((nb_lo + kRsRun - 1) / kRsRun);   // events of the halo before and after: whole runs (0 .. 64 each)
  const int halo_hi = kRsRun * ((nb_hi + kRsRun - 1) / kRsRun);
  const int inner = kRlTile - halo_lo - halo_hi;                // the tile's own events (384 .. 512)
  const double thr = a.thr, prior = a.prior, nan = nan_f64();

  for (;;) {
    unsigned item = 0;
    if constexpr (WAVES == 1) {
      // Every lane takes part in the draw and lane 0 alone adds one: the broadcast below is then reached by the whole wave on
      // every path (DESIGN.md K11 on the hazard of drawing under `if (lane == 0)`).
      const unsigned got = atomicAdd(&a.count[2 + CLS], lane == 0 ? 1u : 0u);
      item = (unsigned)__builtin_amdgcn_readlane((int)got, 0);
    } else {
      __syncthreads();                                          // the last read's uses of sh_cnt / sh_item are over
      if (threadIdx.x == 0) sh_item = atomicAdd(&a.count[2 + CLS], 1u);
      __syncthreads();
      item = sh_item;
    }
    if (item >= cnt) break;
    const int64_t read = (int64_t)a.list[CLS][item];
    int64_t begin, n;
    csr_row(a.off, 0, read, begin, n);
    const uint8_t* bs = a.base + begin;

    unsigned st = 0;
    int sites = 0, mod = 0, can = 0;
    if (n > (int64_t)NMOD_MAX_DEEP) {
      st = NMOD_CALLS_TOO_LARGE;
      for (int64_t j = t; j < n; j += T) {
        if (a.llr) a.llr[begin + j] = nan;
        if (a.llr_win) a.llr_win[begin + j] = nan;
        if (a.p_mod) a.p_mod[begin + j] = nan;
      }
    } else {
      const int64_t ntiles = (n + inner - 1) / inner;
      for (int64_t ti = WAVES == 1 ? 0 : wave; ti < ntiles; ti += WAVES) {
        const int64_t a0 = ti * inner, s0 = a0 - halo_lo;       // the tile's own events start at a0, the staged ones at s0
        const int64_t a1 = a0 + inner < n ? a0 + inner : n;
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
        rl_wave_sync();
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
              const int lo = j < nb_lo ? -(int)j : -nb_lo, hi = n - 1 - j < nb_hi ? (int)(n - 1 - j) : nb_hi;
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
        rl_wave_sync();                                         // the tile is read before the next one is staged
      }
    }
    // the read's counts: integer sums over its threads
    int tot_sites = (int)wave_sum_u64((unsigned long long)sites), tot_mod = (int)wave_sum_u64((unsigned long long)mod),
        tot_can = (int)wave_sum_u64((unsigned long long)can);
    if constexpr (WAVES > 1) {
      if (lane == 0) { sh_cnt[wave] = tot_sites; sh_cnt[kRlWaves + wave] = tot_mod; sh_cnt[2 * kRlWaves + wave] = tot_can; }
      __syncthreads();
      tot_sites = tot_mod = tot_can = 0;
#pragma unroll
      for (int i = 0; i < WAVES; ++i) { tot_sites += sh_cnt[i]; tot_mod += sh_cnt[kRlWaves + i]; tot_can += sh_cnt[2 * kRlWaves + i]; }
    }
    if (t == 0) {
      if (a.n_sites) a.n_sites[read] = tot_sites;
      if (a.n_mod) a.n_mod[read] = tot_mod;
      if (a.n_can) a.n_can[read] = tot_can;
      if (a.status) a.status[read] = (uint8_t)st;
    }
  }
}

template <int DT, bool LDS_TAB>
static void rl_launch(const RlArgs& a, int num_cus, hipStream_t stream) {
  // workgroups a CU holds: five by the registers (87 .. 98 VGPRs: 5 waves per SIMD), unless the LDS of one — the stage, the counts,
  // and the table of this call — allows fewer (it does not up to kRlLdsCodes: 26 KiB)
  const size_t tab_bytes = LDS_TAB ? (size_t)a.ncodes * kRlTabWords * sizeof(double) : 0;
  const size_t per_group = tab_bytes + sizeof(double) * kRlWaves * kRlTile + 256;
  const int64_t resident = (int64_t)(kRlLdsPerCu / per_group) < 5 ? (int64_t)(kRlLdsPerCu / per_group) : 5;
  const int64_t cap = (int64_t)num_cus * resident;
  hipLaunchKernelGGL((rl_read_kernel<DT, 1, LDS_TAB>), dim3(persistent_grid(a.nreads, kRlWaves, cap)), dim3(kRlThreads), tab_bytes, stream, a);
  hipLaunchKernelGGL((rl_read_kernel<DT, kRlWaves, LDS_TAB>), dim3(persistent_grid(a.nreads, 1, cap)), dim3(kRlThreads), tab_bytes, stream, a);
}

template <int DT>
static void rl_launch_dt(const RlArgs& a, int num_cus, hipStream_t stream) {
  if (a.ncodes <= kRlLdsCodes) rl_launch<DT, true>(a, num_cus, stream); else rl_launch<DT, false>(a, num_cus, stream);
}

// a wave per row of window sums; rows strided over the grid's waves
__global__ __launch_bounds__(256) void rl_site_kernel(const double* score, const int64_t* off, int64_t stride, int64_t npos, double thr,
                                                     int32_t* n_valid, int32_t* n_mod, int32_t* n_can, double* frac) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < npos; row += (int64_t)gridDim.x * 4) {
    int64_t begin, n;
    csr_row(off, stride, row, begin, n);
    unsigned long long valid = 0, mod = 0, can = 0;
    for (int64_t j = lane; j < n; j += 64) {
      const double s = score[begin + j];
      valid += fabs(s) <= kDblMax ? 1 : 0;
      mod += s >= thr ? 1 : 0;
      can += s <= -thr ? 1 : 0;
    }
    valid = wave_sum_u64(valid);
    mod = wave_sum_u64(mod);
    can = wave_sum_u64(can);
    if (lane == 0) {
      if (n_valid) n_valid[row] = (int32_t)valid;
      if (n_mod) n_mod[row] = (int32_t)mod;
      if (n_can) n_can[row] = (int32_t)can;
      if (frac) frac[row] = mod + can ? (double)mod / (double)(mod + can) : nan_f64();
    }
  }
}

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
  if (nreads < 0 || nreads > (int64_t)UINT32_MAX - 1) return NMOD_ERR_INVALID_ARG;
  if (!model || model->k < 1 || model->k > 8 || model->center < 0 || model->center >= model->k) return NMOD_ERR_INVALID_ARG;
  if (!alt || alt->k != model->k || alt->center != model->center) return NMOD_ERR_INVALID_ARG;
  if (nreads > 0 && (!off || !val || !base || !model->mean || !model->sd || !alt->mean || !alt->sd)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && nreads > 0 && !csr_offsets_ok(off, nreads)) return NMOD_ERR_INVALID_ARG;
  if (nreads == 0) return NMOD_OK;
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
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
  const size_t o_list = slab.take(nr * 4 * 2), o_count = slab.take(16), o_tab = slab.take(nc * kRlTabWords * 8);
  slab.in(a.off, (nr + 1) * 8); slab.in(a.val, tot * esz); slab.in(a.base, tot);
  slab.in(a.mean0, nc * 8); slab.in(a.sd0, nc * 8); slab.in(a.mean1, nc * 8); slab.in(a.sd1, nc * 8);
  slab.out(a.llr, tot * 8); slab.out(a.llr_win, tot * 8); slab.out(a.p_mod, tot * 8);
  slab.out(a.n_sites, nr * 4); slab.out(a.n_mod, nr * 4); slab.out(a.n_can, nr * 4); slab.out(a.status, nr);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.list[0] = slab.at<uint32_t>(o_list); a.list[1] = a.list[0] + nr;
  a.count = slab.at<uint32_t>(o_count);
  a.tab = slab.at<double>(o_tab);

  NMOD_HIP(hipMemsetAsync(a.count, 0, 16, stream));
  hipLaunchKernelGGL(rl_table_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, a);
  const int64_t cb = (nreads + 255) / 256, ccap = (int64_t)num_cus * 16;
  hipLaunchKernelGGL(rl_classify_kernel, dim3((unsigned)(cb < ccap ? cb : ccap)), dim3(256), 0, stream, a);
  if (prm->dtype == NMOD_DTYPE_F32) rl_launch_dt<NMOD_DTYPE_F32>(a, num_cus, stream);
  else if (prm->dtype == NMOD_DTYPE_I16_MILLI) rl_launch_dt<NMOD_DTYPE_I16_MILLI>(a, num_cus, stream);
  else rl_launch_dt<NMOD_DTYPE_F64>(a, num_cus, stream);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(slab.finish(stream));
  return NMOD_OK;
}

extern "C" int nmod_site_llr(const nmod_params* prm, int64_t npos, const double* score, const int64_t* off, double thr,
                             const nmod_site_llr_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_site_llr_out)) return NMOD_ERR_INVALID_ARG;
  if (!rl_thr_ok(thr)) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > (int64_t)INT32_MAX - 1) return NMOD_ERR_INVALID_ARG;
  if (!off && prm->stride0 <= 0) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && !score) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && off && npos > 0 && !csr_offsets_ok(off, npos)) return NMOD_ERR_INVALID_ARG;
  if (npos == 0) return NMOD_OK;
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t np = (size_t)npos;
  const size_t tot = !host ? 0 : (off ? (size_t)off[npos] : np * (size_t)prm->stride0);
  int32_t* n_valid = out->n_valid; int32_t* n_mod = out->n_mod; int32_t* n_can = out->n_can; double* frac = out->frac;

  Slab slab(host);
  slab.in(off, (np + 1) * 8); slab.in(score, tot * 8);
  slab.out(n_valid, np * 4); slab.out(n_mod, np * 4); slab.out(n_can, np * 4); slab.out(frac, np * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  hipLaunchKernelGGL(rl_site_kernel, dim3(persistent_grid(npos, 4, (int64_t)num_cus * 8)), dim3(256), 0, stream, score, off,
                     off ? 0 : prm->stride0, npos, thr, n_valid, n_mod, n_can, frac);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(slab.finish(stream));
  return NMOD_OK;
}
