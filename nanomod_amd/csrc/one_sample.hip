// nmod_one_sample — one read group against a stored per-position reference (mu, sd [, n]) on the device (K9).
// The reference project has no such step; the definition is the one in include/nanomod_hip.h (tests/one_ref.py restates it
// in numpy).  All on the caller's stream:
//   pos_classify_kernel<OneRule>  (pos_walk.hpp) a thread per position: the size and reference checks and the position's class
//                             by n; the indices of the positions to compute are ballot-compacted into one list per class (one
//                             atomic per wave and class on a device count word); EMPTY / TOO_LARGE / BAD_REFERENCE positions
//                             get their NaN outputs here
//   one_wave_kernel<16,16>    n <= 256, float32 / int16: 16 lanes x 16 float32 keys, four positions per wave (seg_sort)
//   one_wave_kernel<64,16>    n <= 1 024: the whole wave x 16 keys (wave_sort)
//   one_wave_kernel<64,32>    n <= 2 048: the whole wave x 32 keys
//   one_block_kernel          beyond, and every float64 position: a workgroup per position, keys in LDS (float32, or the
//                             order-preserving 64-bit images of the doubles), bitonic sort
// then nmod_combine_track on the KS track.  The grids are persistent and read their list's length from the device: no host
// read anywhere.  The sums are a fixed-order chain per lane and a fixed-order lane / wave reduction, D is a maximum, and both
// kernel families evaluate a slot with the same function (one_d_terms): a position's numbers do not depend on the other
// positions of the batch, on the list order the atomics happened to give, or on CSR versus stride.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "pos_walk.hpp"
#include "rank_stats_packed.hpp"
#include "special_math.hpp"
#include "wave_ops.hpp"

namespace nmod {

constexpr int kOneThreads = 256;                  // one_wave_kernel: four waves
constexpr int kOneBlockThreads = 512;             // one_block_kernel
constexpr int kOneBlockWaves = kOneBlockThreads / 64;
constexpr int kOneClasses = 4;
constexpr int kOneSmall = 256, kOneWave = 1024, kOneWave2 = 2048;   // class limits (tests/test_one_sample_gpu.py names them)

struct OneArgs {
  const void* sig; const int64_t* off; int64_t stride;
  const double* ref_mean; const double* ref_sd; const int32_t* ref_n;
  int64_t npos;
  nmod_one_out out;                                           // comb_st / comb_p are the combine kernel's
  PosLists<kOneClasses> pl;                                   // per class: indices of the positions to compute, their number
};

__device__ __forceinline__ void one_write_nan(const nmod_one_out& o, int64_t i, unsigned status) {
  const double nan = nan_f64();
  if (o.ks_d) o.ks_d[i] = nan;
  if (o.ks_p) o.ks_p[i] = nan;
  if (o.t_t) o.t_t[i] = nan;
  if (o.t_p) o.t_p[i] = nan;
  if (o.shift) o.shift[i] = nan;
  if (o.mean) o.mean[i] = nan;
  if (o.std) o.std[i] = nan;
  if (o.status) o.status[i] = (uint8_t)status;
}

// the class of position i by n (every float64 position: the workgroup form's); the size and reference checks leave a position out
template <int DT>
struct OneRule {
  static constexpr int NC = kOneClasses;
  using Track = void;                                         // no per-sample output
  static __device__ __forceinline__ int cls(const OneArgs& a, int64_t i, int64_t& b, int64_t& n) {
    constexpr int64_t CAP = DT == NMOD_DTYPE_F64 ? NMOD_MAX_ONE_F64 : NMOD_MAX_ONE;
    csr_row(a.off, a.stride, i, b, n);
    const double mu = a.ref_mean[i], sd = a.ref_sd[i];
    unsigned st = 0;
    if (n == 0) st |= NMOD_STATUS_EMPTY;
    if (n > CAP) st |= NMOD_STATUS_TOO_LARGE;
    if (!(fabs(mu) <= kDblMax) || !(sd > 0.0) || !(sd <= kDblMax) || (a.ref_n && a.ref_n[i] < 2)) st |= NMOD_STATUS_BAD_REFERENCE;
    if (st) { one_write_nan(a.out, i, st); return -1; }
    if constexpr (DT == NMOD_DTYPE_F64) return 3;
    else return n <= kOneSmall ? 0 : (n <= kOneWave ? 1 : (n <= kOneWave2 ? 2 : 3));
  }
};

// Both D terms of the order statistic of rank k (1-based): k/n - F_k and F_k - (k-1)/n, F the reference's normal CDF.
// zs = 1 / (sd sqrt 2), rn = 1 / n.  No contraction: the wave and the block kernels must round every step alike.
__device__ __forceinline__ double one_d_terms(double x, int k, double mu, double zs, double rn) {
#pragma clang fp contract(off)
  const double z = (x - mu) * zs;
  const double f = 0.5 * erfc(-z);
  const double hi = (double)k * rn - f;
  const double lo = f - (double)(k - 1) * rn;
  return fmax(hi, lo);
}

// The outputs of a computed position from its moments and D (one lane).  m, s2 in signal units; s2 is ddof = 0.
__device__ __forceinline__ void one_finish(const OneArgs& a, int64_t pos, int64_t n, double m, double s2, double d, bool nonfinite) {
#pragma clang fp contract(off)
  if (nonfinite) { one_write_nan(a.out, pos, NMOD_STATUS_NONFINITE); return; }
  const double mu = a.ref_mean[pos], sd = a.ref_sd[pos], dn = (double)n;
  const double en = sqrt(dn);
  const double ks_p = kolmogorov_sf((en + 0.12 + 0.11 / en) * d);
  const double nan = nan_f64();
  const double vx = s2 * dn / (dn - 1.0);                      // n == 1: 0 / 0
  double t = nan, t_p = nan;
  if (n >= 2) {
    const double vxn = vx / dn;
    if (a.ref_n) {
      const double nr = (double)a.ref_n[pos];
      const double vrn = sd * sd * nr / (nr - 1.0) / nr;
      const double se2 = vxn + vrn;
      if (se2 > 0.0) {
        const double df = se2 * se2 / (vxn * vxn / (dn - 1.0) + vrn * vrn / (nr - 1.0));
        t = (m - mu) / sqrt(se2);
        t_p = student_t_two_sided(t, df);
      }
    } else if (vx > 0.0) {
      t = (m - mu) / sqrt(vxn);
      t_p = student_t_two_sided(t, dn - 1.0);
    }
  }
  const nmod_one_out& o = a.out;
  if (o.ks_d) o.ks_d[pos] = clamp_stat(d);
  if (o.ks_p) o.ks_p[pos] = clamp_p(ks_p);
  if (o.t_t) o.t_t[pos] = clamp_stat(t);
  if (o.t_p) o.t_p[pos] = clamp_p(t_p);
  if (o.shift) o.shift[pos] = (m - mu) / sd;
  if (o.mean) o.mean[pos] = m;
  if (o.std) o.std[pos] = sqrt(s2);
  if (o.status) o.status[pos] = (uint8_t)(t_p != t_p ? NMOD_STATUS_T_NAN : 0);
}

template <int LG>
__device__ __forceinline__ double one_group_max(double v) {
  if constexpr (LG == 64) {
    return wave_max_f64(v);
  } else {
    v = fmax(v, dpp_f64_row(v, 0)); v = fmax(v, dpp_f64_row(v, 1)); v = fmax(v, dpp_f64_row(v, 2)); v = fmax(v, dpp_f64_row(v, 3));
    return v;
  }
}

// The register-resident form: LG lanes x R float32 keys per position (the samples, or k of an int16 sample: exact and
// order-preserving), 64 / LG positions per wave.  Everything between the loads and the stores runs with all lanes on.
template <int LG, int R, int DT>
__global__ __launch_bounds__(kOneThreads) void one_wave_kernel(OneArgs a) {
  constexpr int CLS = LG == 16 ? 0 : (R == 16 ? 1 : 2);
  constexpr int CAP = LG * R;
  __shared__ float keys[kOneThreads * R];                     // the sorted keys of every group: slot e of group g at g * CAP + e
  const float inf = __builtin_inff();
  const int64_t cnt = (int64_t)a.pl.count[CLS];
  const int lane = threadIdx.x & 63, gl = threadIdx.x & (LG - 1), gidx = threadIdx.x / LG;
  float* wkeys = keys + (threadIdx.x >> 6) * (64 * R);
  const float* gkeys = keys + gidx * CAP;
  LaneSel sel;
#pragma unroll
  for (int b = 0; b < 6; ++b) sel.s[b] = ((lane >> b) & 1) ? inf : -inf;

  // pos_walk.hpp's GroupWalk spelled out: through the struct these kernels, which sit at the register limit, compile to another
  // allocation, and the float32 forms lost up to 16 % (profiles/pos_walk.txt); as written they are the instructions they were
  for (int64_t w0 = (int64_t)blockIdx.x * (kOneThreads / LG); w0 < cnt; w0 += (int64_t)gridDim.x * (kOneThreads / LG)) {
    const int64_t w = w0 + gidx;
    const bool have = w < cnt;
    int64_t pos = 0, begin = 0, n64 = 0;
    if (have) {
      pos = (int64_t)a.pl.list[CLS][w];
      csr_row(a.off, a.stride, pos, begin, n64);
    }
    const int n = (int)n64;                                   // <= CAP by the class
    // keys, and the moments from them: two passes in fp64 (int16: in milli-units, the sum of the k is exact)
    float x[R];
    bool bad = false;
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int idx = r * LG + gl;
      const bool in = idx < n;
      x[r] = in ? load_sample<DT>(a.sig, begin + idx) : inf;
      bad |= in && !(fabsf(x[r]) <= 3.4028234663852886e38f);
      acc += in ? (double)x[r] : 0.0;
    }
    const double dn = (double)n;
    const double sum = seg_allsum_f64<LG>(acc);
    const double mk = sum / dn;
    acc = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const double dx = (double)x[r] - mk;
      acc += r * LG + gl < n ? dx * dx : 0.0;
    }
    const double m2 = seg_allsum_f64<LG>(acc);
    const double mean = DT == NMOD_DTYPE_F32 ? mk : sum / 1000.0 / dn;
    const double s2 = DT == NMOD_DTYPE_F32 ? m2 / dn : m2 / dn * 1e-6;
    bad = group_any<LG>(bad, lane);

    if constexpr (LG == 64) wave_sort<R>(x, sel, lane); else seg_sort<R, LG>(x, sel, lane);
    store_sorted<R>(wkeys, x, lane);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // slot e holds the order statistic of rank e + 1
    const double mu = have ? a.ref_mean[pos] : 0.0, sd = have ? a.ref_sd[pos] : 1.0;
    const double zs = 1.0 / (sd * 1.4142135623730951), rn = 1.0 / dn;
    double d = 0.0;
    if (!bad) {
#pragma unroll 1
      for (int e = gl; e < n; e += LG) {
        const double kx = (double)gkeys[e];
        const double xv = DT == NMOD_DTYPE_F32 ? kx : kx / 1000.0;
        d = fmax(d, one_d_terms(xv, e + 1, mu, zs, rn));
      }
    }
    d = one_group_max<LG>(d);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();                          // the keys are read before the next position's are stored
    if (have && gl == 0) one_finish(a, pos, n64, mean, s2, d, bad);
  }
}

// order-preserving unsigned image of a double and back
__device__ __forceinline__ unsigned long long one_image(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double one_unimage(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

template <int DT>
__device__ __forceinline__ double one_load(const void* p, int64_t i) {
  if constexpr (DT == NMOD_DTYPE_F32) return (double)static_cast<const float*>(p)[i];
  else if constexpr (DT == NMOD_DTYPE_I16_MILLI) return (double)static_cast<const int16_t*>(p)[i];   // milli-units
  else return static_cast<const double*>(p)[i];
}

// The workgroup form: a position's keys in LDS (64 KiB: NMOD_MAX_ONE float32 keys or NMOD_MAX_ONE_F64 64-bit images), padded
// with the largest key to a power of two and sorted by a bitonic network.  The reduction words share the LDS with the keys:
// they are used before the keys are loaded and after the last key was read.
template <int DT>
__global__ __launch_bounds__(kOneBlockThreads) void one_block_kernel(OneArgs a) {
  using Key = typename std::conditional<DT == NMOD_DTYPE_F64, unsigned long long, float>::type;
  __shared__ unsigned long long lds[NMOD_MAX_ONE_F64];
  Key* keys = reinterpret_cast<Key*>(lds);
  double* sh = reinterpret_cast<double*>(lds);
  const int tid = threadIdx.x;
  for (BlockWalk<3> it(a.pl); it.more(); it.next()) {
    const int64_t pos = it.pos();
    int64_t begin, n64;
    csr_row(a.off, a.stride, pos, begin, n64);
    const int n = (int)n64;                                   // <= the cap by the classifier
    const double dn = (double)n;
    int bad = 0;
    double acc = 0.0;
    for (int k = tid; k < n; k += kOneBlockThreads) {
      const double v = one_load<DT>(a.sig, begin + k);
      bad |= !(fabs(v) <= kDblMax);
      acc += v;
    }
    const double sum = block_sum_f64<kOneBlockWaves>(acc, sh);
    const double mk = sum / dn;
    acc = 0.0;
    for (int k = tid; k < n; k += kOneBlockThreads) {
      const double dx = one_load<DT>(a.sig, begin + k) - mk;
      acc += dx * dx;
    }
    const double m2 = block_sum_f64<kOneBlockWaves>(acc, sh);
    const double mean = DT == NMOD_DTYPE_I16_MILLI ? sum / 1000.0 / dn : mk;
    const double s2 = DT == NMOD_DTYPE_I16_MILLI ? m2 / dn * 1e-6 : m2 / dn;
    const bool nonfinite = block_sum_f64<kOneBlockWaves>(bad ? 1.0 : 0.0, sh) != 0.0;
    __syncthreads();                                          // every thread has read sh: the keys may come

    double d = 0.0;
    if (!nonfinite) {                                         // block-uniform
      int P = 64;
      while (P < n) P <<= 1;
      for (int k = tid; k < P; k += kOneBlockThreads) {
        if constexpr (DT == NMOD_DTYPE_F64) keys[k] = k < n ? one_image(static_cast<const double*>(a.sig)[begin + k]) : ~0ull;
        else if constexpr (DT == NMOD_DTYPE_F32) keys[k] = k < n ? static_cast<const float*>(a.sig)[begin + k] : __builtin_inff();
        else keys[k] = k < n ? (float)static_cast<const int16_t*>(a.sig)[begin + k] : __builtin_inff();
      }
      __syncthreads();
      for (int size = 2; size <= P; size <<= 1) {
        for (int j = size >> 1; j >= 1; j >>= 1) {
          for (int t = tid; t < (P >> 1); t += kOneBlockThreads) {
            const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
            const bool up = (lo & size) == 0;
            const Key x = keys[lo], y = keys[hi];
            if ((x > y) == up) { keys[lo] = y; keys[hi] = x; }
          }
          __syncthreads();
        }
      }
      const double mu = a.ref_mean[pos], sd = a.ref_sd[pos];
      const double zs = 1.0 / (sd * 1.4142135623730951), rn = 1.0 / dn;
      for (int e = tid; e < n; e += kOneBlockThreads) {
        double xv;
        if constexpr (DT == NMOD_DTYPE_F64) xv = one_unimage(keys[e]);
        else if constexpr (DT == NMOD_DTYPE_F32) xv = (double)keys[e];
        else xv = (double)keys[e] / 1000.0;
        d = fmax(d, one_d_terms(xv, e + 1, mu, zs, rn));
      }
      d = wave_max_f64(d);
      __syncthreads();                                        // every key was read: the LDS is the reduction's again
      if ((tid & 63) == 0) sh[tid >> 6] = d;
      __syncthreads();
      if (tid == 0) {
#pragma unroll
        for (int i = 0; i < kOneBlockWaves; ++i) d = fmax(d, sh[i]);
      }
    }
    if (tid == 0) one_finish(a, pos, n64, mean, s2, d, nonfinite);
    __syncthreads();
  }
}

template <int DT>
static hipError_t one_launch(const Slab& slab, const PosListSpace<kOneClasses>& lists, OneArgs& a, int num_cus, hipStream_t stream) {
  const hipError_t e = lists.fill<OneRule<DT>>(slab, a, num_cus, stream);
  if (e != hipSuccess) return e;
  if constexpr (DT != NMOD_DTYPE_F64) {
    launch_groups<16, kOneThreads>(one_wave_kernel<16, 16, DT>, a, num_cus, stream);
    launch_groups<64, kOneThreads>(one_wave_kernel<64, 16, DT>, a, num_cus, stream);
    launch_groups<64, kOneThreads>(one_wave_kernel<64, 32, DT>, a, num_cus, stream);
  }
  launch_blocks<kOneBlockThreads>(one_block_kernel<DT>, a, num_cus, stream);
  return hipSuccess;
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_one_sample(const nmod_params* prm, int64_t npos, const void* sig, const int64_t* off, const double* ref_mean,
                               const double* ref_sd, const int32_t* ref_n, const int32_t* run_id, const nmod_one_out* out) {
  if (check_prm_common(prm) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (npos < 0 || npos > (int64_t)UINT32_MAX - 1 || !out || out->struct_size != (int32_t)sizeof(nmod_one_out)) return NMOD_ERR_INVALID_ARG;
  if (prm->nb < 0 || prm->nb > NMOD_MAX_NB) return NMOD_ERR_INVALID_ARG;
  if (prm->method != NMOD_METHOD_KS && prm->method != NMOD_METHOD_STOUFFER && prm->method != NMOD_METHOD_FISHER) return NMOD_ERR_INVALID_ARG;
  const bool want_comb = prm->method != NMOD_METHOD_KS && (out->comb_st || out->comb_p);
  if (want_comb && prm->method == NMOD_METHOD_STOUFFER && !(prm->weights_dif > 0.0)) return NMOD_ERR_INVALID_ARG;
  if (npos == 0) return NMOD_OK;
  if (!sig || !ref_mean || !ref_sd) return NMOD_ERR_INVALID_ARG;
  if (!off && prm->stride0 <= 0) return NMOD_ERR_INVALID_ARG;
  if (want_comb && !run_id) return NMOD_ERR_INVALID_ARG;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  int num_cus = 0;
  int rc = rows_begin(prm, npos, off, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;
  const size_t np = (size_t)npos, esz = elem_bytes(prm->dtype);
  const size_t tot = host ? (size_t)(off ? off[npos] : npos * prm->stride0) : 0;

  OneArgs a;
  memset(&a, 0, sizeof(a));
  a.sig = sig; a.off = off; a.stride = off ? 0 : prm->stride0;
  a.ref_mean = ref_mean; a.ref_sd = ref_sd; a.ref_n = ref_n;
  a.npos = npos;
  a.out = *out;
  const int32_t* d_run = run_id;

  // one slab: the work lists and their count words, the KS track where the caller wants the combined pair without it; for the
  // host entry the inputs and outputs as well
  Slab slab(host);
  const PosListSpace<kOneClasses> lists(slab, np);
  const bool own_d = want_comb && !out->ks_d, own_p = want_comb && !out->ks_p;
  const size_t o_ksd = slab.take(own_d ? np * 8 : 0), o_ksp = slab.take(own_p ? np * 8 : 0);
  const bool own_c = want_comb && (!out->comb_st || !out->comb_p);             // a member of the combined pair the caller left out
  const size_t o_spare = slab.take(own_c ? np * 8 : 0);
  slab.in(a.sig, tot * esz); slab.in(a.off, (np + 1) * 8);
  slab.in(a.ref_mean, np * 8); slab.in(a.ref_sd, np * 8); slab.in(a.ref_n, np * 4);
  if (want_comb) slab.in(d_run, np * 4);
  double** const tracks[7] = {&a.out.ks_d, &a.out.ks_p, &a.out.t_t, &a.out.t_p, &a.out.shift, &a.out.mean, &a.out.std};
  for (double** t : tracks) slab.out(*t, np * 8);
  if (want_comb) { slab.out(a.out.comb_st, np * 8); slab.out(a.out.comb_p, np * 8); }
  slab.out(a.out.status, np);
  NMOD_HIP(slab.commit(stream, prm->device));
  if (own_d) a.out.ks_d = slab.at<double>(o_ksd);
  if (own_p) a.out.ks_p = slab.at<double>(o_ksp);

  NMOD_HIP(for_dtype(prm->dtype, [&](auto dt) { return one_launch<decltype(dt)::value>(slab, lists, a, num_cus, stream); }));
  NMOD_HIP(hipGetLastError());
  if (want_comb) {
    // the window combine of the KS track (K3): the code behind nmod_combine_track, on the same stream.  A member of the pair the
    // caller left out goes to a spare word of the slab
    nmod_params cp;
    memset(&cp, 0, sizeof(cp));
    cp.struct_size = (int32_t)sizeof(cp); cp.device = prm->device; cp.stream = prm->stream; cp.memspace = NMOD_MEM_DEVICE;
    cp.dtype = NMOD_DTYPE_F64; cp.method = prm->method; cp.nb = prm->nb; cp.weights_dif = prm->weights_dif;
    double* cst = a.out.comb_st; double* cpv = a.out.comb_p;
    if (!cst) cst = slab.at<double>(o_spare);
    if (!cpv) cpv = slab.at<double>(o_spare);
    rc = nmod_combine_track(&cp, npos, a.out.ks_d, a.out.ks_p, d_run, cst, cpv);
    if (rc != NMOD_OK) return rc;
  }
  NMOD_HIP(slab.finish(stream));
  return NMOD_OK;
}
