// nmod_mix_fraction — per-position modified fraction by a two-component EM on the device (K8).
// The reference has no such step; the definition is the one in include/nanomod_hip.h (tests/mix_ref.py restates it in numpy).
// One group is the reference group R (its mean mu and variance s2 are fixed), the other the mixed group Y:
//   y ~ (1 - pi) N(mu, s2) + pi N(m, v).  All on the caller's stream:
//   pos_classify_kernel<MixRule>  (pos_walk.hpp) a thread per position: the gate, the size checks, and the position's class by |Y|,
//                           ballot-compacted into one list per class (one atomic per wave and class on a device count word);
//                           skipped / degenerate-by-size / too-large positions get their outputs here
//   mix_em_kernel<16>       |Y| <= 256: 16 lanes x 16 doubles hold a position's Y in registers over all iterations, four positions
//                           per wave, DPP row sums only; a finished position freezes while the others of its wave go on
//   mix_em_kernel<64>       |Y| <= 1 024: the whole wave x 16 doubles
//   mix_stream_kernel       beyond: a workgroup per position re-reads Y every iteration (L2-resident up to 65 535 float32
//                           samples), partial sums through LDS in a fixed order; up to NMOD_MAX_DEEP
// The EM itself is written once (mix_estimate) over two row policies, MixRegRow<G> and MixBlockRow, which supply the sums over Y.
// The EM grids are persistent and read their list's length from the device: no host read anywhere.  Every sum is a fixed-order
// chain per lane followed by a fixed-order lane / wave reduction, no atomics: a position's numbers do not depend on the other
// positions of the batch, on the list order the atomics happened to give, or on CSR versus stride.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "pos_walk.hpp"

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
  PosLists<3> pl;                                            // per class: indices of the positions to compute, their number
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

// the class of position i by |Y|; the gate and the size checks leave a position out (the resp of its reads: NaN, by the classify kernel)
struct MixRule {
  static constexpr int NC = 3;
  using Track = float;
  static __device__ __forceinline__ float* track(const MixArgs& a) { return a.out.resp; }
  static __device__ __forceinline__ int cls(const MixArgs& a, int64_t i, int64_t& yb, int64_t& yn) {
    int64_t rb, rn;
    csr_row(a.roff, a.rstride, i, rb, rn);
    csr_row(a.yoff, a.ystride, i, yb, yn);
    unsigned st;
    if (a.gate && !(a.gate[i] <= a.gate_max)) st = NMOD_MIX_SKIPPED;                   // NaN compares false: skipped
    else if (rn > NMOD_MAX_DEEP || yn > NMOD_MAX_DEEP) st = NMOD_MIX_TOO_LARGE;
    else if (rn < 2 || yn < 2) st = NMOD_MIX_DEGENERATE;
    else return yn <= kMixSmall ? 0 : (yn <= kMixWave ? 1 : 2);
    mix_write_nan(a.out, i, st);
    return -1;
  }
};

// softplus(x) = ln(1 + e^x) without overflow
__device__ __forceinline__ double mix_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }

// the parameters of one evaluation; t(y) = ln of the ratio of y's weighted densities, reference component over modified
struct MixAt {
  double c0, m, mu, hv, hs;
  __device__ __forceinline__ double t(double y) const {
    const double dy = y - m, dm = y - mu;
    return c0 + dy * dy * hv - dm * dm * hs;
  }
};

// A row policy hands the samples of Y to the EM: each(f) calls f(y, j, idx, live) for the caller's samples in a fixed order (idx: the
// sample's place in the row, live: whether there is one), sum() adds a per-thread chain over the row, keep() / resp() hold or
// recompute the responsibilities between the two passes of a free-variance iteration.
// MixRegRow: a position in the registers of a group of G lanes, lane g of it keeps y[g + G j], j < 16.  Reached with all lanes on (a
// group without a position, or a finished one, computes and does not commit), so the DPP sums always see a full row.
template <int G, int DT>
struct MixRegRow {
  static constexpr int kLanes = G;
  const void* sig; int64_t yb, yn;
  double y[kMixPer], rr[kMixPer];
  static __device__ __forceinline__ int lane() { return threadIdx.x & (G - 1); }
  static __device__ __forceinline__ bool any(bool f) { return __any(f); }
  __device__ __forceinline__ bool flag(bool f) const { return group_any<G>(f, threadIdx.x & 63); }
  __device__ __forceinline__ double sum(double v) const { return group_sum_f64<G>(v); }
  __device__ __forceinline__ void load() {                  // Y: loaded once
#pragma unroll
    for (int j = 0; j < kMixPer; ++j) y[j] = lane() + G * j < (int)yn ? mix_load<DT>(sig, yb + lane() + G * j) : 0.0;
  }
  template <class F>
  __device__ __forceinline__ void each(F f) const {
#pragma unroll
    for (int j = 0; j < kMixPer; ++j) f(y[j], j, (int64_t)(lane() + G * j), lane() + G * j < (int)yn);
  }
  __device__ __forceinline__ void keep(int j, double r) { rr[j] = r; }
  __device__ __forceinline__ double resp(const MixAt&, double, int j) const { return rr[j]; }
};

// MixBlockRow: a position of a workgroup, thread t takes y[t + 1024 j], read again on every pass; the second pass of a free-variance
// iteration evaluates the responsibilities again instead of storing them.  Everything a decision rests on is a block sum, the same
// bits in every thread: the control flow is uniform over the workgroup.
template <int DT>
struct MixBlockRow {
  static constexpr int kLanes = kMixStreamThreads;
  const void* sig; int64_t yb, yn; double* sh;
  static __device__ __forceinline__ int lane() { return threadIdx.x; }
  static __device__ __forceinline__ bool any(bool f) { return f; }
  __device__ __forceinline__ bool flag(bool f) const { return __syncthreads_or(f) != 0; }
  __device__ __forceinline__ double sum(double v) const { return block_sum_f64<kMixStreamWaves>(v, sh); }
  __device__ __forceinline__ void load() {}
  template <class F>
  __device__ __forceinline__ void each(F f) const {
    for (int64_t i = lane(); i < yn; i += kLanes) f(mix_load<DT>(sig, yb + i), 0, i, true);
  }
  __device__ __forceinline__ void keep(int, double) {}
  __device__ __forceinline__ double resp(const MixAt& at, double y, int) const { return 1.0 / (1.0 + exp(at.t(y))); }
};

// A position from its rows to its outputs: the moments of R (two passes, mean then the squares about it), the start values from
// Y's mean, the iteration, the final llr / resp pass and the commit by `lead`, the thread that writes.  A row without a position
// (have false: rn == yn == 0), a degenerate or a finished one computes along and keeps its state.
template <int DT, int MODEL, class Row>
__device__ __forceinline__ void mix_estimate(const MixArgs& a, Row& row, bool have, bool lead, int64_t pos, int64_t rb, int64_t rn) {
  constexpr bool FREE = MODEL == NMOD_MIX_FREE_VAR;
  bool bad = false, varies = false;
  const double x0 = rn > 0 ? mix_load<DT>(a.r, rb) : 0.0;
  double acc = 0.0;
  for (int64_t k = Row::lane(); k < rn; k += Row::kLanes) {
    const double x = mix_load<DT>(a.r, rb + k);
    bad |= !isfinite(x);
    varies |= x != x0;
    acc += x;
  }
  const double mu = row.sum(acc) / (double)rn;
  acc = 0.0;
  for (int64_t k = Row::lane(); k < rn; k += Row::kLanes) {
    const double dx = mix_load<DT>(a.r, rb + k) - mu;
    acc += dx * dx;
  }
  const double s2 = row.sum(acc) / (double)rn;
  acc = 0.0;
  row.load();
  row.each([&](double y, int, int64_t, bool) { bad |= !isfinite(y); acc += y; });
  const double dn = (double)row.yn, d = row.sum(acc) / dn - mu;
  bad = row.flag(bad);
  varies = row.flag(varies);                                // a constant reference group has s2 == 0 whatever its sums round to
  bool degenerate = !have || bad || !varies || !(s2 > 0.0);

  const double sd = sqrt(s2), vfloor = s2 / 16.0;
  MixAt at{0.0, mu + 2.0 * d, mu, 0.0, 1.0 / (2.0 * s2)};
  double pi = 0.5, v = s2;
  int iters = 0;
  bool active = !degenerate, floored = false;
  auto set_at = [&] {
    at.c0 = log((1.0 - pi) / pi);
    if constexpr (FREE) at.c0 += 0.5 * log(v / s2);
    at.hv = 1.0 / (2.0 * v);
  };
  for (int k = 1; k <= a.max_iter; ++k) {
    if (!Row::any(active)) break;
    set_at();
    double sr = 0.0, sy = 0.0;
    row.each([&](double y, int j, int64_t, bool live) {
      const double t = at.t(y);
      const double r = live ? 1.0 / (1.0 + exp(t)) : 0.0;
      sr += r;
      sy += r * y;
      if constexpr (FREE) row.keep(j, r);
    });
    sr = row.sum(sr);
    sy = row.sum(sy);
    const double pn = sr / dn, mn = sy / sr;
    double vn = v;
    bool fl = false;
    if constexpr (FREE) {                                   // the second pass, about the new mean
      double sq = 0.0;
      row.each([&](double y, int j, int64_t, bool) {
        const double e = y - mn;
        sq += row.resp(at, y, j) * (e * e);
      });
      vn = row.sum(sq) / sr;
      fl = vn < vfloor;
      if (fl) vn = vfloor;
    }
    double delta = fmax(fabs(pn - pi), fabs(mn - at.m) / sd);
    if constexpr (FREE) delta = fmax(delta, fabs(sqrt(vn) - sqrt(v)) / sd);
    if (active) {
      if (!(sr > 0.0)) {                                    // every responsibility underflowed
        degenerate = true; active = false;
      } else {
        pi = pn; at.m = mn; v = vn; floored = fl; iters = k;
        if (a.tol > 0.0 && delta <= a.tol) active = false;
      }
    }
  }
  const bool not_converged = active;                        // still running when max_iter was reached

  // final evaluation: llr and the posteriors
  set_at();
  const double l1 = log(1.0 - pi);
  double ll = 0.0;
  float* const resp = a.out.resp;
  row.each([&](double y, int, int64_t idx, bool live) {
    const double t = at.t(y);
    ll += live ? l1 + mix_softplus(-t) : 0.0;
    if (resp && live) resp[row.yb + idx] = degenerate ? __int_as_float(0x7FC00000) : (float)(1.0 / (1.0 + exp(t)));
  });
  ll = 2.0 * row.sum(ll);
  if (have && lead) {
    if (degenerate) {
      mix_write_nan(a.out, pos, NMOD_MIX_DEGENERATE);
    } else {
      if (a.out.pi) a.out.pi[pos] = pi;
      if (a.out.mu_mod) a.out.mu_mod[pos] = at.m;
      if (a.out.sd_mod) a.out.sd_mod[pos] = sqrt(v);
      if (a.out.llr) a.out.llr[pos] = ll;
      if (a.out.iters) a.out.iters[pos] = iters;
      if (a.out.status) a.out.status[pos] = (uint8_t)((not_converged ? NMOD_MIX_NOT_CONVERGED : 0) | (floored ? NMOD_MIX_VAR_FLOORED : 0));
    }
  }
}

template <int G, int DT, int MODEL>
__global__ __launch_bounds__(kMixThreads) void mix_em_kernel(MixArgs a) {
  for (GroupWalk<G == 16 ? 0 : 1, G, kMixThreads> it(a.pl); it.more(); it.next()) {
    const bool have = it.have();
    MixRegRow<G, DT> row{a.y, 0, 0};
    int64_t pos = 0, rb = 0, rn = 0;
    if (have) {
      pos = it.pos();
      csr_row(a.yoff, a.ystride, pos, row.yb, row.yn);
      csr_row(a.roff, a.rstride, pos, rb, rn);
    }
    mix_estimate<DT, MODEL>(a, row, have, row.lane() == 0, pos, rb, rn);
  }
}

template <int DT, int MODEL>
__global__ __launch_bounds__(kMixStreamThreads) void mix_stream_kernel(MixArgs a) {
  __shared__ double sh[kMixStreamWaves];
  for (BlockWalk<2> it(a.pl); it.more(); it.next()) {
    const int64_t pos = it.pos();
    MixBlockRow<DT> row{a.y, 0, 0, sh};
    int64_t rb, rn;
    csr_row(a.yoff, a.ystride, pos, row.yb, row.yn);
    csr_row(a.roff, a.rstride, pos, rb, rn);
    mix_estimate<DT, MODEL>(a, row, true, row.lane() == 0, pos, rb, rn);
  }
}

template <int DT, int MODEL>
static void mix_launch(const MixArgs& a, int num_cus, hipStream_t stream) {
  launch_groups<16, kMixThreads>(mix_em_kernel<16, DT, MODEL>, a, num_cus, stream);
  launch_groups<64, kMixThreads>(mix_em_kernel<64, DT, MODEL>, a, num_cus, stream);
  launch_blocks<kMixStreamThreads>(mix_stream_kernel<DT, MODEL>, a, num_cus, stream);
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
  const PosListSpace<3> lists(slab, np);
  const size_t toty = y1 ? tot1 : tot0, totr = y1 ? tot0 : tot1;
  slab.in(a.y, toty * esz); slab.in(a.yoff, (np + 1) * 8);
  slab.in(a.r, totr * esz); slab.in(a.roff, (np + 1) * 8);
  slab.in(a.gate, np * 8);
  slab.out(a.out.pi, np * 8); slab.out(a.out.mu_mod, np * 8); slab.out(a.out.sd_mod, np * 8); slab.out(a.out.llr, np * 8);
  slab.out(a.out.iters, np * 4); slab.out(a.out.status, np); slab.out(a.out.resp, toty * 4);
  NMOD_HIP(slab.commit(stream, prm->device));

  NMOD_HIP(lists.fill<MixRule>(slab, a, num_cus, stream));
  for_dtype(prm->dtype, [&](auto dt) {
    if (model == NMOD_MIX_FREE_VAR) mix_launch<decltype(dt)::value, NMOD_MIX_FREE_VAR>(a, num_cus, stream);
    else mix_launch<decltype(dt)::value, NMOD_MIX_EQUAL_VAR>(a, num_cus, stream);
  });
  return launches_end(slab, stream);
}
