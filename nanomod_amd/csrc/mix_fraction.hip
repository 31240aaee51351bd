// nmod_mix_fraction — per-position modified fraction by a two-component EM on the device (K8).
// The reference has no such step; the definition is the one in include/nanomod_hip.h (tests/mix_ref.py restates it in numpy).
// One group is the reference group R (its mean mu and variance s2 are fixed), the other the mixed group Y:
//   y ~ (1 - pi) N(mu, s2) + pi N(m, v).  All on the caller's stream:
//   mix_classify_kernel     a thread per position: the gate, the size checks, and the position's class by |Y|; the indices of the
//                           positions to compute are ballot-compacted into one list per class (one atomic per wave and class on a
//                           device count word); skipped / degenerate-by-size / too-large positions get their outputs here
//   mix_em_kernel<16>       |Y| <= 256: 16 lanes x 16 doubles hold a position's Y in registers over all iterations, four positions
//                           per wave, DPP row sums only; a finished position freezes while the others of its wave go on
//   mix_em_kernel<64>       |Y| <= 1 024: the whole wave x 16 doubles
//   mix_stream_kernel       beyond: a workgroup per position re-reads Y every iteration (L2-resident up to 65 535 float32
//                           samples), partial sums through LDS in a fixed order; up to NMOD_MAX_DEEP
// The EM grids are persistent and read their list's length from the device: no host read anywhere.  Every sum is a fixed-order
// chain per lane followed by a fixed-order lane / wave reduction, no atomics: a position's numbers do not depend on the other
// positions of the batch, on the list order the atomics happened to give, or on CSR versus stride.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "entry_device.hpp"

namespace nmod {

constexpr int kMixPer = 16;                       // doubles of Y a lane keeps
constexpr int kMixSmall = 16 * kMixPer;           // largest |Y| of the 16-lane form
constexpr int kMixWave = 64 * kMixPer;            // largest |Y| of the whole-wave form (tests/test_mix_gpu.py names both)
constexpr int kMixThreads = 256;
constexpr int kMixStreamThreads = 1024;
constexpr int kMixStreamWaves = kMixStreamThreads / 64;

struct MixArgs {
  const void* y; const int64_t* yoff; int64_t ystride;       // the mixed group
  const void* r; const int64_t* roff; int64_t rstride;       // the reference group
  int64_t npos;
  int max_iter; double tol;
  const double* gate; double gate_max;
  nmod_mix_out out;
  uint32_t* list[3]; uint32_t* count;                        // per class: indices of the positions to compute, their number
};

template <int DT>
__device__ __forceinline__ double mix_load(const void* p, int64_t i) {
  if constexpr (DT == NMOD_DTYPE_F32) return (double)static_cast<const float*>(p)[i];
  else if constexpr (DT == NMOD_DTYPE_I16_MILLI) return (double)static_cast<const int16_t*>(p)[i] / 1000.0;
  else return static_cast<const double*>(p)[i];
}

__device__ __forceinline__ void mix_write_nan(const nmod_mix_out& o, int64_t i, unsigned status) {
  const double nan = nan_f64();
  if (o.pi) o.pi[i] = nan;
  if (o.mu_mod) o.mu_mod[i] = nan;
  if (o.sd_mod) o.sd_mod[i] = nan;
  if (o.llr) o.llr[i] = nan;
  if (o.iters) o.iters[i] = 0;
  if (o.status) o.status[i] = (uint8_t)status;
}

__global__ __launch_bounds__(256) void mix_classify_kernel(MixArgs a) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.npos; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < a.npos;
    int cls = -1;
    int64_t yb = 0, yn = 0;
    if (in) {
      int64_t rb, rn;
      csr_row(a.roff, a.rstride, i, rb, rn);
      csr_row(a.yoff, a.ystride, i, yb, yn);
      unsigned st = 0;
      if (a.gate && !(a.gate[i] <= a.gate_max)) st = NMOD_MIX_SKIPPED;                 // NaN compares false: skipped
      else if (rn > NMOD_MAX_DEEP || yn > NMOD_MAX_DEEP) st = NMOD_MIX_TOO_LARGE;
      else if (rn < 2 || yn < 2) st = NMOD_MIX_DEGENERATE;
      else cls = yn <= kMixSmall ? 0 : (yn <= kMixWave ? 1 : 2);
      if (cls < 0) mix_write_nan(a.out, i, st);
    }
    compact_to_lists<3>(cls, lane, a.list, a.count, i);
    if (a.out.resp) {                                       // the reads of the positions left out: NaN, a wave per row
      unsigned long long mask = __ballot(in && cls < 0);
      while (mask) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1ull;
        const int64_t b = __shfl((long long)yb, src), n = __shfl((long long)yn, src);
        for (int64_t k = lane; k < n; k += 64) a.out.resp[b + k] = __int_as_float(0x7FC00000);
      }
    }
  }
}

// softplus(x) = ln(1 + e^x) without overflow
__device__ __forceinline__ double mix_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// The register-resident form: a group of G lanes per position, lane g of it keeps y[g + G j], j < 16.  Everything between the
// loads and the stores runs with all lanes on (a group without a position, or a finished one, computes and does not commit),
// so the DPP sums always see a full row.
template <int G, int DT, int MODEL>
__global__ __launch_bounds__(kMixThreads) void mix_em_kernel(MixArgs a) {
  constexpr int CLS = G == 16 ? 0 : 1;
  constexpr int GPB = kMixThreads / G;
  const int64_t cnt = (int64_t)a.count[CLS];
  const int lane = threadIdx.x & 63, gl = threadIdx.x & (G - 1), gidx = threadIdx.x / G;
  for (int64_t w0 = (int64_t)blockIdx.x * GPB; w0 < cnt; w0 += (int64_t)gridDim.x * GPB) {
    const int64_t w = w0 + gidx;
    const bool have = w < cnt;
    int64_t pos = 0, yb = 0, yn = 0, rb = 0, rn = 0;
    if (have) {
      pos = (int64_t)a.list[CLS][w];
      csr_row(a.yoff, a.ystride, pos, yb, yn);
      csr_row(a.roff, a.rstride, pos, rb, rn);
    }
    // R: two passes, mean then the squares about it
    bool bad = false, varies = false;
    const double x0 = rn > 0 ? mix_load<DT>(a.r, rb) : 0.0;
    double acc = 0.0;
    for (int64_t k = gl; k < rn; k += G) {
      const double x = mix_load<DT>(a.r, rb + k);
      bad |= !isfinite(x);
      varies |= x != x0;
      acc += x;
    }
    const double mu = group_sum_f64<G>(acc) / (double)rn;
    acc = 0.0;
    for (int64_t k = gl; k < rn; k += G) {
      const double dx = mix_load<DT>(a.r, rb + k) - mu;
      acc += dx * dx;
    }
    const double s2 = group_sum_f64<G>(acc) / (double)rn;
    // Y: loaded once
    double y[kMixPer];
    const int ny = (int)yn;
    acc = 0.0;
#pragma unroll
    for (int j = 0; j < kMixPer; ++j) {
      const int idx = gl + G * j;
      y[j] = idx < ny ? mix_load<DT>(a.y, yb + idx) : 0.0;
      bad |= !isfinite(y[j]);
      acc += y[j];
    }
    const double d = group_sum_f64<G>(acc) / (double)yn - mu;
    bad = group_any<G>(bad, lane);
    varies = group_any<G>(varies, lane);                 // a constant reference group has s2 == 0 whatever its sums round to
    bool degenerate = !have || bad || !varies || !(s2 > 0.0);

    const double sd = sqrt(s2), hs = 1.0 / (2.0 * s2), vfloor = s2 / 16.0, dn = (double)yn;
    double pi = 0.5, m = mu + 2.0 * d, v = s2;
    int iters = 0;
    bool active = !degenerate, floored = false;
    for (int k = 1; k <= a.max_iter; ++k) {
      if (!__any(active)) break;
      double c0 = log((1.0 - pi) / pi);
      if constexpr (MODEL == NMOD_MIX_FREE_VAR) c0 += 0.5 * log(v / s2);
      const double hv = 1.0 / (2.0 * v);
      double rr[MODEL == NMOD_MIX_FREE_VAR ? kMixPer : 1];
      double sr = 0.0, sy = 0.0;
#pragma unroll
      for (int j = 0; j < kMixPer; ++j) {
        const double dy = y[j] - m, dm = y[j] - mu;
        const double t = c0 + dy * dy * hv - dm * dm * hs;
        const double r = gl + G * j < ny ? 1.0 / (1.0 + exp(t)) : 0.0;
        sr += r;
        sy += r * y[j];
        if constexpr (MODEL == NMOD_MIX_FREE_VAR) rr[j] = r;
      }
      sr = group_sum_f64<G>(sr);
      sy = group_sum_f64<G>(sy);
      const double pn = sr / dn, mn = sy / sr;
      double vn = v;
      bool fl = false;
      if constexpr (MODEL == NMOD_MIX_FREE_VAR) {
        double sq = 0.0;
#pragma unroll
        for (int j = 0; j < kMixPer; ++j) {
          const double e = y[j] - mn;
          sq += rr[j] * (e * e);
        }
        vn = group_sum_f64<G>(sq) / sr;
        fl = vn < vfloor;
        if (fl) vn = vfloor;
      }
      double delta = fmax(fabs(pn - pi), fabs(mn - m) / sd);
      if constexpr (MODEL == NMOD_MIX_FREE_VAR) delta = fmax(delta, fabs(sqrt(vn) - sqrt(v)) / sd);
      if (active) {
        if (!(sr > 0.0)) {                                  // every responsibility underflowed
          degenerate = true; active = false;
        } else {
          pi = pn; m = mn; v = vn; floored = fl; iters = k;
          if (a.tol > 0.0 && delta <= a.tol) active = false;
        }
      }
    }
    const bool not_converged = active;                      // still running when max_iter was reached

    // final evaluation: llr and the posteriors
    double c0 = log((1.0 - pi) / pi);
    if constexpr (MODEL == NMOD_MIX_FREE_VAR) c0 += 0.5 * log(v / s2);
    const double hv = 1.0 / (2.0 * v), l1 = log(1.0 - pi);
    double ll = 0.0;
    float* resp = a.out.resp;
#pragma unroll
    for (int j = 0; j < kMixPer; ++j) {
      const int idx = gl + G * j;
      const double dy = y[j] - m, dm = y[j] - mu;
      const double t = c0 + dy * dy * hv - dm * dm * hs;
      ll += idx < ny ? l1 + mix_softplus(-t) : 0.0;
      if (resp && have && idx < ny) resp[yb + idx] = degenerate ? __int_as_float(0x7FC00000) : (float)(1.0 / (1.0 + exp(t)));
    }
    ll = 2.0 * group_sum_f64<G>(ll);
    if (have && gl == 0) {
      if (degenerate) {
        mix_write_nan(a.out, pos, NMOD_MIX_DEGENERATE);
      } else {
        if (a.out.pi) a.out.pi[pos] = pi;
        if (a.out.mu_mod) a.out.mu_mod[pos] = m;
        if (a.out.sd_mod) a.out.sd_mod[pos] = sqrt(v);
        if (a.out.llr) a.out.llr[pos] = ll;
        if (a.out.iters) a.out.iters[pos] = iters;
        if (a.out.status) a.out.status[pos] = (uint8_t)((not_converged ? NMOD_MIX_NOT_CONVERGED : 0) | (floored ? NMOD_MIX_VAR_FLOORED : 0));
      }
    }
  }
}

// The streaming form: a workgroup per position, Y re-read every iteration.  The free-variance model makes two passes per
// iteration (the second, about the new mean, evaluates the responsibilities again instead of storing them).
template <int DT, int MODEL>
__global__ __launch_bounds__(kMixStreamThreads) void mix_stream_kernel(MixArgs a) {
  __shared__ double sh[kMixStreamWaves];
  const int64_t cnt = (int64_t)a.count[2];
  const int tid = threadIdx.x;
  for (int64_t w = blockIdx.x; w < cnt; w += gridDim.x) {
    const int64_t pos = (int64_t)a.list[2][w];
    int64_t yb, yn, rb, rn;
    csr_row(a.yoff, a.ystride, pos, yb, yn);
    csr_row(a.roff, a.rstride, pos, rb, rn);
    int bad = 0, varies = 0;
    const double x0 = mix_load<DT>(a.r, rb);
    double acc = 0.0;
    for (int64_t k = tid; k < rn; k += kMixStreamThreads) {
      const double x = mix_load<DT>(a.r, rb + k);
      bad |= !isfinite(x);
      varies |= x != x0;
      acc += x;
    }
    const double mu = block_sum_f64<kMixStreamWaves>(acc, sh) / (double)rn;
    acc = 0.0;
    for (int64_t k = tid; k < rn; k += kMixStreamThreads) {
      const double dx = mix_load<DT>(a.r, rb + k) - mu;
      acc += dx * dx;
    }
    const double s2 = block_sum_f64<kMixStreamWaves>(acc, sh) / (double)rn;
    acc = 0.0;
    for (int64_t k = tid; k < yn; k += kMixStreamThreads) {
      const double x = mix_load<DT>(a.y, yb + k);
      bad |= !isfinite(x);
      acc += x;
    }
    const double d = block_sum_f64<kMixStreamWaves>(acc, sh) / (double)yn - mu;
    bool degenerate = __syncthreads_or(bad) != 0;
    degenerate = __syncthreads_or(varies) == 0 || degenerate || !(s2 > 0.0);   // (a constant reference group: s2 == 0 exactly)

    const double sd = sqrt(s2), hs = 1.0 / (2.0 * s2), vfloor = s2 / 16.0, dn = (double)yn;
    double pi = 0.5, m = mu + 2.0 * d, v = s2;
    int iters = 0;
    bool active = !degenerate, floored = false;                // block-uniform from here on
    for (int k = 1; k <= a.max_iter && active; ++k) {
      double c0 = log((1.0 - pi) / pi);
      if constexpr (MODEL == NMOD_MIX_FREE_VAR) c0 += 0.5 * log(v / s2);
      const double hv = 1.0 / (2.0 * v);
      double sr = 0.0, sy = 0.0;
      for (int64_t i = tid; i < yn; i += kMixStreamThreads) {
        const double yv = mix_load<DT>(a.y, yb + i);
        const double dy = yv - m, dm = yv - mu;
        const double r = 1.0 / (1.0 + exp(c0 + dy * dy * hv - dm * dm * hs));
        sr += r;
        sy += r * yv;
      }
      sr = block_sum_f64<kMixStreamWaves>(sr, sh);
      sy = block_sum_f64<kMixStreamWaves>(sy, sh);
      if (!(sr > 0.0)) { degenerate = true; active = false; break; }
      const double pn = sr / dn, mn = sy / sr;
      double vn = v;
      bool fl = false;
      if constexpr (MODEL == NMOD_MIX_FREE_VAR) {
        double sq = 0.0;
        for (int64_t i = tid; i < yn; i += kMixStreamThreads) {
          const double yv = mix_load<DT>(a.y, yb + i);
          const double dy = yv - m, dm = yv - mu, e = yv - mn;
          const double r = 1.0 / (1.0 + exp(c0 + dy * dy * hv - dm * dm * hs));
          sq += r * (e * e);
        }
        vn = block_sum_f64<kMixStreamWaves>(sq, sh) / sr;
        fl = vn < vfloor;
        if (fl) vn = vfloor;
      }
      double delta = fmax(fabs(pn - pi), fabs(mn - m) / sd);
      if constexpr (MODEL == NMOD_MIX_FREE_VAR) delta = fmax(delta, fabs(sqrt(vn) - sqrt(v)) / sd);
      pi = pn; m = mn; v = vn; floored = fl; iters = k;
      if (a.tol > 0.0 && delta <= a.tol) active = false;
    }
    const bool not_converged = active;

    double c0 = log((1.0 - pi) / pi);
    if constexpr (MODEL == NMOD_MIX_FREE_VAR) c0 += 0.5 * log(v / s2);
    const double hv = 1.0 / (2.0 * v), l1 = log(1.0 - pi);
    double ll = 0.0;
    float* resp = a.out.resp;
    for (int64_t i = tid; i < yn; i += kMixStreamThreads) {
      const double yv = mix_load<DT>(a.y, yb + i);
      const double dy = yv - m, dm = yv - mu;
      const double t = c0 + dy * dy * hv - dm * dm * hs;
      ll += l1 + mix_softplus(-t);
      if (resp) resp[yb + i] = degenerate ? __int_as_float(0x7FC00000) : (float)(1.0 / (1.0 + exp(t)));
    }
    ll = 2.0 * block_sum_f64<kMixStreamWaves>(ll, sh);
    if (tid == 0) {
      if (degenerate) {
        mix_write_nan(a.out, pos, NMOD_MIX_DEGENERATE);
      } else {
        if (a.out.pi) a.out.pi[pos] = pi;
        if (a.out.mu_mod) a.out.mu_mod[pos] = m;
        if (a.out.sd_mod) a.out.sd_mod[pos] = sqrt(v);
        if (a.out.llr) a.out.llr[pos] = ll;
        if (a.out.iters) a.out.iters[pos] = iters;
        if (a.out.status) a.out.status[pos] = (uint8_t)((not_converged ? NMOD_MIX_NOT_CONVERGED : 0) | (floored ? NMOD_MIX_VAR_FLOORED : 0));
      }
    }
  }
}

template <int DT, int MODEL>
static void mix_launch(const MixArgs& a, int num_cus, hipStream_t stream) {
  const int64_t cap = (int64_t)num_cus * 8;
  hipLaunchKernelGGL((mix_em_kernel<16, DT, MODEL>), dim3(persistent_grid(a.npos, kMixThreads / 16, cap)), dim3(kMixThreads), 0, stream, a);
  hipLaunchKernelGGL((mix_em_kernel<64, DT, MODEL>), dim3(persistent_grid(a.npos, kMixThreads / 64, cap)), dim3(kMixThreads), 0, stream, a);
  const int64_t sb = a.npos < (int64_t)num_cus * 2 ? a.npos : (int64_t)num_cus * 2;
  hipLaunchKernelGGL((mix_stream_kernel<DT, MODEL>), dim3((unsigned)sb), dim3(kMixStreamThreads), 0, stream, a);
}

template <int DT>
static void mix_launch_model(const MixArgs& a, int model, int num_cus, hipStream_t stream) {
  if (model == NMOD_MIX_FREE_VAR) mix_launch<DT, NMOD_MIX_FREE_VAR>(a, num_cus, stream);
  else mix_launch<DT, NMOD_MIX_EQUAL_VAR>(a, num_cus, stream);
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_mix_fraction(const nmod_params* prm, int64_t npos, const void* sig0, const int64_t* off0, const void* sig1,
                                 const int64_t* off1, int32_t mix_group, int32_t model, int32_t max_iter, double tol,
                                 const double* gate, double gate_max, const nmod_mix_out* out) {
  if (check_prm_common(prm) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > (int64_t)UINT32_MAX - 1 || !out) return NMOD_ERR_INVALID_ARG;
  if (mix_group != 0 && mix_group != 1) return NMOD_ERR_INVALID_ARG;
  if (model != NMOD_MIX_EQUAL_VAR && model != NMOD_MIX_FREE_VAR) return NMOD_ERR_INVALID_ARG;
  if (max_iter < 1 || max_iter > 10000 || !(tol >= 0.0) || isinf(tol)) return NMOD_ERR_INVALID_ARG;
  if (npos == 0) return NMOD_OK;
  if (!sig0 || !sig1) return NMOD_ERR_INVALID_ARG;
  if ((!off0 && prm->stride0 <= 0) || (!off1 && prm->stride1 <= 0)) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host && ((off0 && !csr_offsets_ok(off0, npos)) || (off1 && !csr_offsets_ok(off1, npos)))) return NMOD_ERR_INVALID_ARG;
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t np = (size_t)npos, esz = elem_bytes(prm->dtype);
  const size_t tot0 = host ? (size_t)(off0 ? off0[npos] : npos * prm->stride0) : 0;
  const size_t tot1 = host ? (size_t)(off1 ? off1[npos] : npos * prm->stride1) : 0;
  const bool y1 = mix_group == 1;

  MixArgs a;
  memset(&a, 0, sizeof(a));
  a.y = y1 ? sig1 : sig0; a.yoff = y1 ? off1 : off0; a.ystride = y1 ? prm->stride1 : prm->stride0;
  a.r = y1 ? sig0 : sig1; a.roff = y1 ? off0 : off1; a.rstride = y1 ? prm->stride0 : prm->stride1;
  a.npos = npos; a.max_iter = max_iter; a.tol = tol;
  a.gate = gate; a.gate_max = gate_max;
  a.out = *out;

  // one slab: the three work lists and their count words; for the host entry the inputs and outputs as well
  Slab slab(host);
  const size_t o_list = slab.take(np * 4 * 3), o_count = slab.take(16);
  const size_t toty = y1 ? tot1 : tot0, totr = y1 ? tot0 : tot1;
  slab.in(a.y, toty * esz); slab.in(a.yoff, (np + 1) * 8);
  slab.in(a.r, totr * esz); slab.in(a.roff, (np + 1) * 8);
  slab.in(a.gate, np * 8);
  slab.out(a.out.pi, np * 8); slab.out(a.out.mu_mod, np * 8); slab.out(a.out.sd_mod, np * 8); slab.out(a.out.llr, np * 8);
  slab.out(a.out.iters, np * 4); slab.out(a.out.status, np); slab.out(a.out.resp, toty * 4);
  NMOD_HIP(slab.commit(stream, prm->device));
  for (int c = 0; c < 3; ++c) a.list[c] = slab.at<uint32_t>(o_list) + (size_t)c * np;
  a.count = slab.at<uint32_t>(o_count);

  NMOD_HIP(hipMemsetAsync(a.count, 0, 16, stream));
  const int64_t cb = (npos + 255) / 256;
  hipLaunchKernelGGL(mix_classify_kernel, dim3((unsigned)(cb < (int64_t)num_cus * 16 ? cb : (int64_t)num_cus * 16)), dim3(256), 0, stream, a);
  if (prm->dtype == NMOD_DTYPE_F32) mix_launch_model<NMOD_DTYPE_F32>(a, model, num_cus, stream);
  else if (prm->dtype == NMOD_DTYPE_I16_MILLI) mix_launch_model<NMOD_DTYPE_I16_MILLI>(a, model, num_cus, stream);
  else mix_launch_model<NMOD_DTYPE_F64>(a, model, num_cus, stream);
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(slab.finish(stream));
  return NMOD_OK;
}
