// nmod_read_calls / nmod_site_calls — per-read modification calls against a k-mer model, and their per-position counts, on the device
// (K12).  The reference project has no such step; the definition is the one in include/nanomod_hip.h
// (tests/readcalls_ref.py restates it in numpy).  All on the caller's stream:
//   rc_table_kernel      a thread per code: the model as (mu, sd) with sd = -1 for an entry that makes its events ineligible
//   rc_classify_kernel   a thread per read: the read's class by its length, ballot-compacted into one list per class
//   rc_read_kernel<.., 1>  a wave per read of up to NMOD_CALLS_WAVE_MAX events, four waves a workgroup
//   rc_read_kernel<.., 4>  a workgroup of four waves per longer read, a tile of the read per wave and step
//   rc_site_kernel       (nmod_site_calls) a wave per row of pivoted scores
// Both read forms are one function, and a wave works alone in both until the read's counts are summed.  A wave stages the log tails l of
// 512 consecutive events (64 lanes x a run of 8, the 2-bit code rolled over the run's bases and a k - 1 byte halo as in K11) in its own
// 4 KiB of LDS; the first and last ceil(nb / 8) runs of the tile are the window halo, recomputed by the neighbouring tiles, and the
// events between them are the tile's own: their z and p are stored from the runs, their windows summed directly from the staged l in
// ascending order, event e of the tile on lane e mod 64 (consecutive lanes: consecutive LDS words and one contiguous store).  No
// running prefix over the read: with |l| up to 1e3 and 1e5 .. 1e6 events the difference of two prefixes would not keep 1e-9 of a
// window's sum.  The grids are persistent; a wave / workgroup draws its next read with one returning atomic on a ticket word (K11's
// idiom, and DESIGN.md K11 on why every lane takes part in it).  No float atomics: the counts are integer sums, and a read's bits
// depend on the read alone — its class comes from its length — not on the batch, the list order, the memspace or the outputs asked for.
// The table lives in LDS up to 1 024 codes (k <= 5: 16 KiB); beyond it is read through L2.
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

constexpr int kRcThreads = 256;
constexpr int kRcWaves = kRcThreads / 64;
constexpr int kRcTile = 64 * kRsRun;              // events a wave stages at a time
constexpr int kRcLdsCodes = 1024;                 // the table lives in LDS up to here: 16 bytes per code

struct RcArgs {
  const void* val; const uint8_t* base; const int64_t* off; int64_t nreads;
  const double* mean; const double* sd;           // the model as given
  double* tab;                                    // mu[ncodes], sd[ncodes] (-1: ineligible)
  int32_t k, center, ncodes, nb;
  double alpha;
  double *z, *p, *p_win; int32_t *n_sites, *n_called; uint8_t* status;
  uint32_t* list[2]; uint32_t* count;             // count[0 .. 1]: the lists' lengths, count[2 .. 3]: their ticket words
};

__global__ __launch_bounds__(256) void rc_table_kernel(RcArgs a) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.ncodes) return;
  const double mu = a.mean[c], sd = a.sd[c];
  const bool ok = fabs(mu) <= kDblMax && sd > 0.0 && sd <= kDblMax;
  a.tab[c] = ok ? mu : 0.0;
  a.tab[a.ncodes + c] = ok ? sd : -1.0;
}

__global__ __launch_bounds__(256) void rc_classify_kernel(RcArgs a) {
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
__device__ __forceinline__ void rc_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// WAVES == 1: a wave per read (list 0), the workgroup's waves independent; else the workgroup per read (list 1)
template <int DT, int WAVES, bool LDS_TAB>
__global__ __launch_bounds__(kRcThreads) void rc_read_kernel(RcArgs a) {
#pragma clang fp contract(off)
  constexpr int CLS = WAVES == 1 ? 0 : 1;
  constexpr int T = WAVES * 64;                                 // threads of a read
  __shared__ double lds_tab[LDS_TAB ? 2 * kRcLdsCodes : 1];
  __shared__ double lds_stage[kRcWaves][kRcTile];
  __shared__ int sh_cnt[2 * kRcWaves];
  __shared__ unsigned sh_item;
  const int nc = a.ncodes;
  const double* tmu = a.tab; const double* tsd = a.tab + nc;
  if constexpr (LDS_TAB) {
    for (int c = threadIdx.x; c < 2 * nc; c += kRcThreads) lds_tab[c] = a.tab[c];
    tmu = lds_tab; tsd = lds_tab + nc;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int t = WAVES == 1 ? lane : (int)threadIdx.x;
  double* stage = lds_stage[wave];
  const unsigned cnt = a.count[CLS];
  const int k = a.k, center = a.center, nb = a.nb;
  const int halo = kRsRun * ((nb + kRsRun - 1) / kRsRun);       // events of the halo on each side: whole runs (0 .. 64)
  const int inner = kRcTile - 2 * halo;                         // the tile's own events (384 .. 512)
  const double alpha = a.alpha, nan = nan_f64();

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
    int sites = 0, called = 0;
    if (n > (int64_t)NMOD_MAX_DEEP) {
      st = NMOD_CALLS_TOO_LARGE;
      for (int64_t j = t; j < n; j += T) {
        if (a.z) a.z[begin + j] = nan;
        if (a.p) a.p[begin + j] = nan;
        if (a.p_win) a.p_win[begin + j] = nan;
      }
    } else {
      const int64_t ntiles = (n + inner - 1) / inner;
      for (int64_t ti = WAVES == 1 ? 0 : wave; ti < ntiles; ti += WAVES) {
        const int64_t a0 = ti * inner, s0 = a0 - halo;          // the tile's own events start at a0, the staged ones at s0
        const int64_t a1 = a0 + inner < n ? a0 + inner : n;
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
          rc_wave_sync();
          const int own = (int)(a1 - a0);
          for (int e = lane; e < own; e += 64) {
            const int64_t j = a0 + e;
            const int c = e + halo;                             // j's word of the stage
            double P = nan;
            if (stage[c] == stage[c]) {
              const int lo = j < nb ? -(int)j : -nb, hi = n - 1 - j < nb ? (int)(n - 1 - j) : nb;
              int W = 0;
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
          rc_wave_sync();                                       // the tile is read before the next one is staged
        }
      }
    }
    // the read's counts: integer sums over its threads
    int tot_sites = (int)wave_sum_u64((unsigned long long)sites), tot_called = (int)wave_sum_u64((unsigned long long)called);
    if constexpr (WAVES > 1) {
      if (lane == 0) { sh_cnt[wave] = tot_sites; sh_cnt[kRcWaves + wave] = tot_called; }
      __syncthreads();
      tot_sites = tot_called = 0;
#pragma unroll
      for (int i = 0; i < WAVES; ++i) { tot_sites += sh_cnt[i]; tot_called += sh_cnt[kRcWaves + i]; }
    }
    if (t == 0) {
      if (a.n_sites) a.n_sites[read] = tot_sites;
      if (a.n_called) a.n_called[read] = tot_called;
      if (a.status) a.status[read] = (uint8_t)st;
    }
  }
}

template <int DT, bool LDS_TAB>
static void rc_launch(const RcArgs& a, int num_cus, hipStream_t stream) {
  // (the fp64 tails keep 256 VGPRs and some AGPRs live: one workgroup per CU is resident; a second one in the grid only shortens the tail)
  const int64_t cap = (int64_t)num_cus * 2;
  hipLaunchKernelGGL((rc_read_kernel<DT, 1, LDS_TAB>), dim3(persistent_grid(a.nreads, kRcWaves, cap)), dim3(kRcThreads), 0, stream, a);
  hipLaunchKernelGGL((rc_read_kernel<DT, kRcWaves, LDS_TAB>), dim3(persistent_grid(a.nreads, 1, cap)), dim3(kRcThreads), 0, stream, a);
}

template <int DT>
static void rc_launch_dt(const RcArgs& a, int num_cus, hipStream_t stream) {
  if (a.ncodes <= kRcLdsCodes) rc_launch<DT, true>(a, num_cus, stream); else rc_launch<DT, false>(a, num_cus, stream);
}

// a wave per row of scores; rows strided over the grid's waves
__global__ __launch_bounds__(256) void rc_site_kernel(const double* score, const int64_t* off, int64_t stride, int64_t npos, double alpha,
                                                     int32_t* n_valid, int32_t* n_called, double* frac) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < npos; row += (int64_t)gridDim.x * 4) {
    int64_t begin, n;
    csr_row(off, stride, row, begin, n);
    unsigned long long valid = 0, called = 0;
    for (int64_t j = lane; j < n; j += 64) {
      const double s = score[begin + j];
      const bool ok = s >= 0.0 && s <= 1.0;
      valid += ok ? 1 : 0;
      called += ok && s <= alpha ? 1 : 0;
    }
    valid = wave_sum_u64(valid);
    called = wave_sum_u64(called);
    if (lane == 0) {
      if (n_valid) n_valid[row] = (int32_t)valid;
      if (n_called) n_called[row] = (int32_t)called;
      if (frac) frac[row] = valid ? (double)called / (double)valid : nan_f64();
    }
  }
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_read_calls(const nmod_params* prm, int64_t nreads, const int64_t* off, const void* val, const uint8_t* base,
                               const nmod_rescale_model* model, const nmod_calls_opts* opts, const nmod_calls_out* out) {
  if (check_prm_common(prm) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_calls_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_calls_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->nb < 0 || opts->nb > NMOD_MAX_NB) return NMOD_ERR_INVALID_ARG;
  if (!(opts->alpha > 0.0 && opts->alpha <= 1.0)) return NMOD_ERR_INVALID_ARG;
  if (nreads < 0 || nreads > (int64_t)UINT32_MAX - 1) return NMOD_ERR_INVALID_ARG;
  if (!model || model->k < 1 || model->k > 8 || model->center < 0 || model->center >= model->k) return NMOD_ERR_INVALID_ARG;
  if (nreads > 0 && (!off || !val || !base || !model->mean || !model->sd)) return NMOD_ERR_INVALID_ARG;
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

  RcArgs a;
  memset(&a, 0, sizeof(a));
  a.val = val; a.base = base; a.off = off; a.nreads = nreads;
  a.mean = model->mean; a.sd = model->sd; a.k = model->k; a.center = model->center; a.ncodes = (int32_t)nc;
  a.nb = opts->nb; a.alpha = opts->alpha;
  a.z = out->z; a.p = out->p; a.p_win = out->p_win; a.n_sites = out->n_sites; a.n_called = out->n_called; a.status = out->status;

  // one slab: the work lists with their count and ticket words and the table; for the host entry the inputs and outputs as well
  Slab slab(host);
  const size_t o_list = slab.take(nr * 4 * 2), o_count = slab.take(16), o_tab = slab.take(nc * 16);
  slab.in(a.off, (nr + 1) * 8); slab.in(a.val, tot * esz); slab.in(a.base, tot); slab.in(a.mean, nc * 8); slab.in(a.sd, nc * 8);
  slab.out(a.z, tot * 8); slab.out(a.p, tot * 8); slab.out(a.p_win, tot * 8);
  slab.out(a.n_sites, nr * 4); slab.out(a.n_called, nr * 4); slab.out(a.status, nr);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.list[0] = slab.at<uint32_t>(o_list); a.list[1] = a.list[0] + nr;
  a.count = slab.at<uint32_t>(o_count);
  a.tab = slab.at<double>(o_tab);

  NMOD_HIP(hipMemsetAsync(a.count, 0, 16, stream));
  hipLaunchKernelGGL(rc_table_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, a);
  const int64_t cb = (nreads + 255) / 256, ccap = (int64_t)num_cus * 16;
  hipLaunchKernelGGL(rc_classify_kernel, dim3((unsigned)(cb < ccap ? cb : ccap)), dim3(256), 0, stream, a);
  if (prm->dtype == NMOD_DTYPE_F32) rc_launch_dt<NMOD_DTYPE_F32>(a, num_cus, stream);
  else if (prm->dtype == NMOD_DTYPE_I16_MILLI) rc_launch_dt<NMOD_DTYPE_I16_MILLI>(a, num_cus, stream);
  else rc_launch_dt<NMOD_DTYPE_F64>(a, num_cus, stream);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(slab.finish(stream));
  return NMOD_OK;
}

extern "C" int nmod_site_calls(const nmod_params* prm, int64_t npos, const double* score, const int64_t* off, double alpha,
                               const nmod_site_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_site_out)) return NMOD_ERR_INVALID_ARG;
  if (!(alpha > 0.0 && alpha <= 1.0)) return NMOD_ERR_INVALID_ARG;
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
  int32_t* n_valid = out->n_valid; int32_t* n_called = out->n_called; double* frac = out->frac;

  Slab slab(host);
  slab.in(off, (np + 1) * 8); slab.in(score, tot * 8);
  slab.out(n_valid, np * 4); slab.out(n_called, np * 4); slab.out(frac, np * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  hipLaunchKernelGGL(rc_site_kernel, dim3(persistent_grid(npos, 4, (int64_t)num_cus * 8)), dim3(256), 0, stream, score, off,
                     off ? 0 : prm->stride0, npos, alpha, n_valid, n_called, frac);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(slab.finish(stream));
  return NMOD_OK;
}
