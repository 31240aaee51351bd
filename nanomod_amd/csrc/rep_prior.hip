// nmod_rep_prior — the prior law of K24's per-site dispersions fitted over all sites of a call: limma's fitFDist at equal degrees of
// freedom, on the device (K25).  The reference project has no such step; the definition is the one in
// include/nanomod_hip.h (tests/diff_mod_ref.py restates it in numpy).  Four launches on the caller's stream, nothing read by the host:
//   rp_part_kernel<false>  a workgroup per CHUNK of NMOD_REP_PRIOR_CHUNK consecutive sites (strided over a persistent grid): the chunk's
//                          sum of e, its count of sites in the fit and its count of zeros, three words per chunk
//   rp_mean_kernel         one workgroup: the chunks' words in ascending chunk order; emean, n_used, n_zero
//   rp_part_kernel<true>   the same walk: the chunk's sum of (e - emean)^2
//   rp_solve_kernel        one workgroup: the chunks' words in ascending chunk order, then one thread: evar, d0, s0^2, df_tot and the
//                          quantile — the record
// The order of every sum is fixed by the chunk size and the workgroup size alone: thread t of a chunk adds its sites t, t + 256, ...
// in ascending order, block_sum_f64 joins the threads, and the one-workgroup kernels give thread t a contiguous run of chunks, added
// in ascending order, the 256 runs joined in ascending t by thread 0.  No float atomics, and nothing depends on the grid: the record
// has the same bits in every run, for every grid size and in both memspaces.  e is computed twice (once per pass) by the same
// operations; contraction is off for the unit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "entry_device.hpp"
#include "special_math.hpp"

namespace nmod {

constexpr int kRpThreads = 256, kRpWaves = kRpThreads / 64;
static_assert(NMOD_REP_PRIOR_CHUNK % kRpThreads == 0, "a thread takes the same number of sites of every chunk");
constexpr unsigned kRpNoEstimate = NMOD_REP_TOO_FEW | NMOD_REP_FLAT | NMOD_REP_TOO_LARGE;

struct RpArgs {
  const double* phi; const uint8_t* status;
  int64_t npos, nchunks;
  int df; double level;
  double* part;                                   // [3 * nchunks]: per chunk the sum, the count in the fit, the count of zeros
  double* mid;                                    // emean, n_used, n_zero
  double* prior;                                  // the record
};

// SQ false: sum e, count the sites of the fit and the zeros;  SQ true: sum (e - emean)^2
template <bool SQ>
__global__ __launch_bounds__(kRpThreads) void rp_part_kernel(RpArgs a) {
  __shared__ double sh[kRpWaves];
  const double half = 0.5 * (double)a.df;
  const double psi = digamma(half), lg = log(half);
  const double emean = SQ ? a.mid[0] : 0.0;
  for (int64_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    double s = 0.0, n = 0.0, z = 0.0;
#pragma unroll 1
    for (int j = 0; j < NMOD_REP_PRIOR_CHUNK / kRpThreads; ++j) {
      const int64_t i = c * NMOD_REP_PRIOR_CHUNK + j * kRpThreads + threadIdx.x;
      if (i >= a.npos) break;
      if (a.status[i] & kRpNoEstimate) continue;
      const double ph = a.phi[i];
      if (ph > 0.0 && ph <= kDblMax) {
        const double e = log(ph) - psi + lg;
        if constexpr (SQ) { const double d = e - emean; s += d * d; }
        else { s += e; n += 1.0; }
      } else if (ph <= 0.0) {
        z += 1.0;
      }
    }
    s = block_sum_f64<kRpWaves>(s, sh);
    if constexpr (!SQ) { n = block_sum_f64<kRpWaves>(n, sh); z = block_sum_f64<kRpWaves>(z, sh); }
    if (threadIdx.x == 0) {
      if constexpr (SQ) a.part[c] = s;
      else { a.part[3 * c] = s; a.part[3 * c + 1] = n; a.part[3 * c + 2] = z; }
    }
    __syncthreads();
  }
}

// word `w` of every chunk (`stride` words apart) summed in ascending chunk order by one workgroup; the sum in thread 0 alone
__device__ __forceinline__ double rp_chunk_sum(const double* part, int64_t nchunks, int stride, int w, double* sh) {
  const int64_t per = (nchunks + kRpThreads - 1) / kRpThreads;
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < nchunks ? lo + per : nchunks;
  double s = 0.0;
#pragma unroll 1
  for (int64_t c = lo; c < hi; ++c) s += part[c * stride + w];
  __syncthreads();
  sh[threadIdx.x] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll 1
    for (int k = 0; k < kRpThreads; ++k) t += sh[k];
  }
  return t;
}

__global__ __launch_bounds__(kRpThreads) void rp_mean_kernel(RpArgs a) {
  __shared__ double sh[kRpThreads];
  const double s = rp_chunk_sum(a.part, a.nchunks, 3, 0, sh);
  const double n = rp_chunk_sum(a.part, a.nchunks, 3, 1, sh);
  const double z = rp_chunk_sum(a.part, a.nchunks, 3, 2, sh);
  if (threadIdx.x == 0) { a.mid[0] = s / n; a.mid[1] = n; a.mid[2] = z; }      // (n == 0: emean NaN)
}

__global__ __launch_bounds__(kRpThreads) void rp_solve_kernel(RpArgs a) {
  __shared__ double sh[kRpThreads];
  const double q = rp_chunk_sum(a.part, a.nchunks, 1, 0, sh);
  if (threadIdx.x != 0) return;
  const double emean = a.mid[0], n = a.mid[1], zeros = a.mid[2];
  const double df = (double)a.df;
  double d0 = 0.0, s0 = nan_f64(), evar = nan_f64();
  if (n >= 2.0) {
    evar = q / (n - 1.0) - trigamma(0.5 * df);
    if (evar > 0.0) {
      d0 = 2.0 * trigamma_inverse(evar);
      s0 = exp(emean + digamma(0.5 * d0) - log(0.5 * d0));
    } else {
      d0 = __builtin_inf();
      s0 = exp(emean);
    }
  }
  const double df_tot = df + d0;
  a.prior[0] = d0; a.prior[1] = s0; a.prior[2] = df_tot; a.prior[3] = f1_quantile(a.level, df_tot);
  a.prior[4] = n; a.prior[5] = zeros; a.prior[6] = emean; a.prior[7] = evar;
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_rep_prior(const nmod_params* prm, int64_t npos, int32_t df, const double* phi, const uint8_t* status, double ci_level,
                              double* prior) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > (int64_t)INT32_MAX - 1 || df < 1 || df > NMOD_REP_MAX_SAMPLES - 2) return NMOD_ERR_INVALID_ARG;
  if (!(ci_level > 0.0) || !(ci_level < 1.0) || !prior) return NMOD_ERR_INVALID_ARG;
  if (npos > 0 && (!phi || !status)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;

  RpArgs a;
  memset(&a, 0, sizeof(a));
  a.phi = phi; a.status = status; a.npos = npos;
  a.nchunks = (npos + NMOD_REP_PRIOR_CHUNK - 1) / NMOD_REP_PRIOR_CHUNK;
  a.df = df; a.level = ci_level; a.prior = prior;

  Slab slab(host);
  const size_t o_part = slab.take((size_t)a.nchunks * 3 * 8), o_mid = slab.take(3 * 8);
  slab.in(a.phi, (size_t)npos * 8); slab.in(a.status, (size_t)npos);
  slab.out(a.prior, NMOD_REP_PRIOR_WORDS * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.part = slab.at<double>(o_part); a.mid = slab.at<double>(o_mid);
  const dim3 grid(persistent_grid(a.nchunks, 1, (int64_t)num_cus * 4)), block(kRpThreads);
  if (a.nchunks > 0) hipLaunchKernelGGL(rp_part_kernel<false>, grid, block, 0, stream, a);
  hipLaunchKernelGGL(rp_mean_kernel, dim3(1), block, 0, stream, a);
  if (a.nchunks > 0) hipLaunchKernelGGL(rp_part_kernel<true>, grid, block, 0, stream, a);
  hipLaunchKernelGGL(rp_solve_kernel, dim3(1), block, 0, stream, a);
  return launches_end(slab, stream);
}
