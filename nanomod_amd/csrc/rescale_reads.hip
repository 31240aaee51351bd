// nmod_rescale_reads — per-read shift and scale against a k-mer model, and the rescaled events, on the device (K11).
// The reference project has no such step; the definition is the one in include/nanomod_hip.h (tests/rescale_ref.py restates it
// in numpy).  The walk over the reads is read_walk.hpp's, shared with K12 and K13; all on the caller's stream:
//   rs_table_kernel      (fitting modes) a thread per code: the model as (mu, sd, w) with sd = -1 for an entry that makes its
//                        events ineligible, so that the fit reads one table and divides nothing per event
//   read_classify_kernel (read_walk.hpp) a thread per read: the read's class by its length, ballot-compacted into one list per class
//   rs_read_kernel<.., 1>  a wave per read of up to NMOD_RESCALE_WAVE_MAX events, four waves a workgroup
//   rs_read_kernel<.., 4>  a workgroup of four waves per longer read
// Both forms are one function.  A lane takes runs of 8 consecutive events (run c of the read on lane c mod lanes) and rolls the
// 2-bit code over the run's bases and a k - 1 byte halo; per fit it chains W, sum w mu', sum w x', sum w mu' mu', sum w mu' x'
// (primes: about the read's first eligible event) in fp64 in event order, and the lanes' words are summed in a fixed order
// (wave_sum_f64, block_sum_f64).  The apply pass follows the fits in the same kernel, while the read's events are L2-resident.
// The grids are persistent; a wave / workgroup draws its next read with one returning atomic on a ticket word (draw_read,
// read_walk.hpp; a read is hundreds of events or more: the ticket is noise, and the lengths differ by orders of magnitude).  No float
// atomics: a read's bits depend on the read alone — its class comes from its length — not on the batch, the list order or the memspace.
// The table lives in LDS up to 1 024 codes (k <= 5: 24 KiB); beyond it is read through L2.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "read_walk.hpp"

namespace nmod {

constexpr int kRsLdsCodes = 1024;                 // the table lives in LDS up to here: 24 bytes per code

struct RsArgs {
  const void* val; void* val_out; const uint8_t* base; const int64_t* off; int64_t nreads;
  const double* mean; const double* sd;           // the model as given
  double* tab;                                    // mu[ncodes], sd[ncodes] (-1: ineligible), w[ncodes]
  int32_t k, center, ncodes;
  int32_t mode, weighted, clip_rounds, min_events;
  double clip_sigma, scale_lo, scale_hi;
  double* shift; double* scale; int32_t* n_used; uint8_t* status;
  ReadLists w;
};

__global__ __launch_bounds__(256) void rs_table_kernel(RsArgs a) {
#pragma clang fp contract(off)
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.ncodes) return;
  const double mu = a.mean[c], sd = a.sd[c];
  const bool ok = fabs(mu) <= kDblMax && sd > 0.0 && sd <= kDblMax;
  a.tab[c] = ok ? mu : 0.0;
  a.tab[a.ncodes + c] = ok ? sd : -1.0;
  a.tab[2 * a.ncodes + c] = !ok ? 0.0 : (a.weighted ? 1.0 / (sd * sd) : 1.0);
}

// sum / maximum over the group that computes a read (a wave, or the workgroup), the same bits in every thread
template <int WAVES>
__device__ __forceinline__ double rs_sum(double v, double* sh) {
  if constexpr (WAVES == 1) return wave_sum_f64(v); else return block_sum_f64<WAVES>(v, sh);
}
template <int WAVES>
__device__ __forceinline__ double rs_max(double v, double* sh) {   // v >= 0
  const double w = wave_max_f64(v);
  if constexpr (WAVES == 1) return w;
  else {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = w;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < WAVES; ++i) t = fmax(t, sh[i]);
    return t;
  }
}

template <int DT>
__device__ __forceinline__ void rs_copy(const RsArgs& a, int64_t begin, int64_t n, int t, int T) {
  if (!a.val_out || a.val_out == a.val) return;
  using E = typename std::conditional<DT == NMOD_DTYPE_F32, float, typename std::conditional<DT == NMOD_DTYPE_F64, double, int16_t>::type>::type;
  const E* src = static_cast<const E*>(a.val) + begin;
  E* dst = static_cast<E*>(a.val_out) + begin;
  for (int64_t j = t; j < n; j += T) dst[j] = src[j];
}

// x' of one event, stored; whether an int16 saturated
template <int DT>
__device__ __forceinline__ bool rs_apply_one(const void* val, void* out, int64_t i, double a0, double r) {
#pragma clang fp contract(off)
  const double x = rs_load<DT>(val, i);
  if (!(fabs(x) <= kDblMax)) {                                  // a non-finite value stays as it is
    if constexpr (DT == NMOD_DTYPE_F32) static_cast<float*>(out)[i] = static_cast<const float*>(val)[i];
    else if constexpr (DT == NMOD_DTYPE_F64) static_cast<double*>(out)[i] = x;
    return false;
  }
  const double y = (x - a0) * r;
  if constexpr (DT == NMOD_DTYPE_F64) { static_cast<double*>(out)[i] = y; return false; }
  else if constexpr (DT == NMOD_DTYPE_F32) { static_cast<float*>(out)[i] = (float)y; return false; }
  else {
    const double q = rint(1000.0 * y);
    const bool sat = !(fabs(q) <= 32767.0);
    static_cast<int16_t*>(out)[i] = (int16_t)(sat ? (q > 0.0 ? 32767 : -32767) : (int)q);
    return sat;
  }
}

// WAVES == 1: a wave per read (list 0), the workgroup's waves independent; else the workgroup per read (list 1)
template <int DT, int WAVES, bool LDS_TAB>
__global__ __launch_bounds__(kRwThreads) void rs_read_kernel(RsArgs a) {
#pragma clang fp contract(off)
  constexpr int CLS = WAVES == 1 ? 0 : 1;
  constexpr int T = WAVES * 64;                                 // threads of a read
  __shared__ double lds_tab[LDS_TAB ? 3 * kRsLdsCodes : 1];
  __shared__ double sh[kRwWaves];
  __shared__ unsigned sh_item;
  const bool fit = a.mode != NMOD_RESCALE_APPLY_ONLY, apply = a.mode != NMOD_RESCALE_FIT_ONLY;
  const int nc = a.ncodes;
  const double* tmu = a.tab; const double* tsd = a.tab + nc; const double* tw = a.tab + 2 * nc;
  if constexpr (LDS_TAB) {
    if (fit) for (int c = threadIdx.x; c < 3 * nc; c += kRwThreads) lds_tab[c] = a.tab[c];
    tmu = lds_tab; tsd = lds_tab + nc; tw = lds_tab + 2 * nc;
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int t = WAVES == 1 ? lane : (int)threadIdx.x;
  const unsigned cnt = a.w.count[CLS];
  const int k = a.k, center = a.center;

  for (;;) {
    const unsigned item = draw_read<WAVES>(a.w, sh_item);
    if (item >= cnt) break;
    const int64_t read = (int64_t)a.w.list[CLS][item];
    int64_t begin, n;
    csr_row(a.off, 0, read, begin, n);
    const uint8_t* bs = a.base + begin;
    const int64_t nruns = (n + kRsRun - 1) / kRsRun;

    unsigned st = 0;
    double fa = 0.0, fb = 1.0, used = 0.0;
    if (n > (int64_t)NMOD_MAX_DEEP) {
      st = NMOD_RESCALE_TOO_LARGE;
    } else if (!fit) {
      fa = a.shift[read]; fb = a.scale[read];
      if (!(fabs(fa) <= kDblMax) || !(fb > 0.0) || !(fb <= kDblMax)) st = NMOD_RESCALE_DEGENERATE;
    } else {
      // the read's first eligible event: the origin of the sums.  A step of the group at a time, until one has it
      double first = 0.0;                                       // n - j of it (0: none)
      for (int64_t c0 = 0; c0 < nruns && first == 0.0; c0 += T) {
        double mine = 0.0;
        const int64_t c = c0 + t;
        if (c < nruns) {
          rs_run(bs, n, c * kRsRun, k, center, [&](int64_t j, int code) {
            if (code < 0 || mine != 0.0 || !(tsd[code] > 0.0)) return;
            const double x = rs_load<DT>(a.val, begin + j);
            if (fabs(x) <= kDblMax) mine = (double)(n - j);
          });
        }
        first = rs_max<WAVES>(mine, sh);
      }
      double mu0 = 0.0, x0 = 0.0;
      if (first != 0.0) {
        // its code again, from its own bases (every thread: the same bytes)
        const int64_t j0 = n - (int64_t)first;
        unsigned code = 0;
        for (int d = 0; d < k; ++d) code = (code << 2) | (unsigned)rs_base2(bs[j0 - center + d]);
        mu0 = tmu[code];
        x0 = rs_load<DT>(a.val, begin + j0);
      }
      for (int round = 0; round <= a.clip_rounds && !st; ++round) {
        const double ca = fa, cb = fb, lim = a.clip_sigma * fabs(fb);
        double cn = 0.0, W = 0.0, sm = 0.0, sx = 0.0, smm = 0.0, smx = 0.0;
        if (first != 0.0) {
          for (int64_t c = t; c < nruns; c += T) {
            rs_run(bs, n, c * kRsRun, k, center, [&](int64_t j, int code) {
              if (code < 0) return;
              const double sd = tsd[code];
              if (!(sd > 0.0)) return;
              const double x = rs_load<DT>(a.val, begin + j);
              if (!(fabs(x) <= kDblMax)) return;
              const double mu = tmu[code];
              if (round > 0 && !(fabs(x - ca - cb * mu) <= lim * sd)) return;
              const double w = tw[code], dm = mu - mu0, dx = x - x0;
              const double wm = w * dm;
              cn += 1.0; W += w; sm += wm; sx += w * dx; smm += wm * dm; smx += wm * dx;
            });
          }
        }
        cn = rs_sum<WAVES>(cn, sh); W = rs_sum<WAVES>(W, sh); sm = rs_sum<WAVES>(sm, sh); sx = rs_sum<WAVES>(sx, sh);
        smm = rs_sum<WAVES>(smm, sh); smx = rs_sum<WAVES>(smx, sh);
        used = cn;
        if (cn < (double)a.min_events) { st = NMOD_RESCALE_TOO_FEW; break; }
        const double mb = sm / W, xb = sx / W;
        const double Smm = smm - sm * mb, Smx = smx - sm * xb;
        const double b = Smx / Smm;
        if (!(Smm > 0.0) || !(fabs(b) <= kDblMax) || !(b > 0.0)) { st = NMOD_RESCALE_DEGENERATE; break; }
        fb = b;
        fa = (x0 + xb) - b * (mu0 + mb);
        if (!(fabs(fa) <= kDblMax)) { st = NMOD_RESCALE_DEGENERATE; break; }
      }
      if (!st && !(fb >= a.scale_lo && fb <= a.scale_hi)) st = NMOD_RESCALE_OUT_OF_RANGE;
    }

    bool sat = false;
    if (st) {
      fa = 0.0; fb = 1.0;
      if (apply) rs_copy<DT>(a, begin, n, t, T);
    } else if (apply) {
      const double r = 1.0 / fb;
      for (int64_t j = t; j < n; j += T) sat |= rs_apply_one<DT>(a.val, a.val_out, begin + j, fa, r);
    }
    if constexpr (DT == NMOD_DTYPE_I16_MILLI) {
      if constexpr (WAVES == 1) sat = __ballot(sat) != 0ull; else sat = __syncthreads_or(sat ? 1 : 0) != 0;
      if (sat) st |= NMOD_RESCALE_CLAMPED;
    }
    if (t == 0) {
      if (fit) {
        if (a.shift) a.shift[read] = fa;
        if (a.scale) a.scale[read] = fb;
      }
      if (a.n_used) a.n_used[read] = (int32_t)used;
      if (a.status) a.status[read] = (uint8_t)st;
    }
  }
}

struct RsKernels {
  template <int DT, int WAVES, bool LDS_TAB> static auto kernel() { return &rs_read_kernel<DT, WAVES, LDS_TAB>; }
};

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_rescale_reads(const nmod_params* prm, int64_t nreads, const int64_t* off, const void* val, const uint8_t* base,
                                  const nmod_rescale_model* model, const nmod_rescale_opts* opts, const nmod_rescale_out* out) {
  if (check_prm_common(prm) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_rescale_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_rescale_out)) return NMOD_ERR_INVALID_ARG;
  const int mode = opts->mode;
  if (mode != NMOD_RESCALE_FIT_APPLY && mode != NMOD_RESCALE_FIT_ONLY && mode != NMOD_RESCALE_APPLY_ONLY) return NMOD_ERR_INVALID_ARG;
  const bool fit = mode != NMOD_RESCALE_APPLY_ONLY, apply = mode != NMOD_RESCALE_FIT_ONLY;
  if (!read_count_ok(nreads) || (fit && !kmer_model_ok(model))) return NMOD_ERR_INVALID_ARG;
  if (opts->clip_rounds < 0 || opts->clip_rounds > 8) return NMOD_ERR_INVALID_ARG;
  if (opts->clip_rounds > 0 && !(opts->clip_sigma > 0.0 && opts->clip_sigma <= kDblMax)) return NMOD_ERR_INVALID_ARG;
  if (opts->min_events < 2) return NMOD_ERR_INVALID_ARG;
  if (!(opts->scale_lo > 0.0) || !(opts->scale_lo <= kDblMax) || !(opts->scale_lo <= opts->scale_hi)) return NMOD_ERR_INVALID_ARG;
  if (nreads > 0) {
    if (!off || !val) return NMOD_ERR_INVALID_ARG;
    if (fit && (!base || !model->mean || !model->sd)) return NMOD_ERR_INVALID_ARG;
    if (apply && !out->val_out) return NMOD_ERR_INVALID_ARG;
    if (!fit && (!out->shift || !out->scale)) return NMOD_ERR_INVALID_ARG;
  }
  int num_cus = 0;
  const int rc = rows_begin(prm, nreads, off, &num_cus);
  if (rc != NMOD_OK || nreads == 0) return rc;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t nr = (size_t)nreads, esz = elem_bytes(prm->dtype);
  const size_t tot = host ? (size_t)off[nreads] : 0;
  const size_t nc = fit ? (size_t)1 << (2 * model->k) : 0;

  RsArgs a;
  memset(&a, 0, sizeof(a));
  a.val = val; a.val_out = apply ? out->val_out : nullptr; a.base = base; a.off = off; a.nreads = nreads;
  if (fit) { a.mean = model->mean; a.sd = model->sd; a.k = model->k; a.center = model->center; }
  else { a.k = 1; }
  a.ncodes = (int32_t)nc;
  a.mode = mode; a.weighted = opts->weighted != 0; a.clip_rounds = fit ? opts->clip_rounds : 0; a.min_events = opts->min_events;
  a.clip_sigma = opts->clip_sigma; a.scale_lo = opts->scale_lo; a.scale_hi = opts->scale_hi;
  a.shift = out->shift; a.scale = out->scale; a.n_used = out->n_used; a.status = out->status;

  // one slab: the work lists with their count and ticket words and the table; for the host entry the inputs and outputs as well
  // (an in-place host call has two device copies of the events: the bits are the same)
  Slab slab(host);
  const ReadListSpace lists(slab, nr);
  const size_t o_tab = slab.take(nc * 24);
  slab.in(a.off, (nr + 1) * 8); slab.in(a.val, tot * esz);
  if (fit) { slab.in(a.base, tot); slab.in(a.mean, nc * 8); slab.in(a.sd, nc * 8); }
  if (fit) { slab.out(a.shift, nr * 8); slab.out(a.scale, nr * 8); }
  else { slab.in(a.shift, nr * 8); slab.in(a.scale, nr * 8); }
  slab.out(a.n_used, nr * 4); slab.out(a.status, nr);
  slab.out(a.val_out, tot * esz);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.tab = slab.at<double>(o_tab);

  NMOD_HIP(lists.fill(slab, a.off, nreads, num_cus, stream, a.w));
  if (fit) hipLaunchKernelGGL(rs_table_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, stream, a);
  // (workgroups a CU: six beside the 24 KiB table in LDS, eight without it)
  if (a.ncodes <= kRsLdsCodes) launch_read_kernels<RsKernels, true>(a, prm->dtype, (int64_t)num_cus * 6, 0, stream);
  else launch_read_kernels<RsKernels, false>(a, prm->dtype, (int64_t)num_cus * 8, 0, stream);
  return launches_end(slab, stream);
}
