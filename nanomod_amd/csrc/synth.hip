// nmod_synth_fill*: the synthetic two-group signal generators (K5, K5b) — the benchmark's and the tests' input, made on the
// device as a counter-based function of (seed, position, group, read): reproducible, any launch shape.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "detect_internal.hpp"
#include "evtimer.hpp"

namespace nmod {

// ---------------------------------------------------------------------------
// K5 synthetic two-group signal generator (include/nanomod_hip.h: nmod_synth_fill)
__device__ __forceinline__ uint64_t synth_mix(uint64_t seed, int64_t pos, int32_t group, uint32_t read) {
  uint64_t x = seed + 0x9E3779B97F4A7C15ull * (uint64_t)(pos * 2 + group);
  x ^= (uint64_t)read * 0xD1B54A32D192ED03ull;
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

struct SynthArgs {
  uint64_t seed; int64_t pos_begin; int64_t npos; int32_t group; int32_t n_per_pos;
  int64_t plant_period; float plant_shift; int32_t dtype; void* out;
};

__global__ __launch_bounds__(256) void synth_kernel(SynthArgs a) {
  const int64_t total = a.npos * (int64_t)a.n_per_pos;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    int64_t rel = idx / a.n_per_pos;
    uint32_t read = (uint32_t)(idx - rel * a.n_per_pos);
    int64_t pos = a.pos_begin + rel;
    uint64_t h = synth_mix(a.seed, pos, a.group, read);
    int s = (int)((h & 0xffff) + ((h >> 16) & 0xffff) + ((h >> 32) & 0xffff) + (h >> 48));
    float x = __fmul_rn((float)(s - 131070), 2.6428997e-05f);
    asm volatile("" : "+v"(x));                         // (rounded here: never contracted with the planted shift)
    if (a.group == 1 && a.plant_period > 0) {
      int64_t m = pos % a.plant_period;
      if (m == 0 || m == 1 || m == a.plant_period - 1) x = __fadd_rn(x, a.plant_shift);
    }
    if (a.dtype == NMOD_DTYPE_F32) reinterpret_cast<float*>(a.out)[idx] = x;
    else reinterpret_cast<int16_t*>(a.out)[idx] = (int16_t)rintf(__fmul_rn(x, 1000.0f));
  }
}

// the same values for ragged rows: sample `read` of position pos_begin + i goes to sig[off[i] + read]; one wave per row
struct SynthCsrArgs {
  uint64_t seed; int64_t pos_begin; int64_t npos; int32_t group; int32_t dtype;
  int64_t plant_period; float plant_shift; const int64_t* off; void* out;
};

__global__ __launch_bounds__(256) void synth_csr_kernel(SynthCsrArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (int64_t rel = wave; rel < a.npos; rel += (int64_t)gridDim.x * 4) {
    const int64_t o = a.off[rel];
    const int n = (int)(a.off[rel + 1] - o);
    const int64_t pos = a.pos_begin + rel;
    bool planted = false;
    if (a.group == 1 && a.plant_period > 0) {
      const int64_t m = pos % a.plant_period;
      planted = (m == 0 || m == 1 || m == a.plant_period - 1);
    }
    for (int read = lane; read < n; read += 64) {
      const uint64_t h = synth_mix(a.seed, pos, a.group, (uint32_t)read);
      const int s = (int)((h & 0xffff) + ((h >> 16) & 0xffff) + ((h >> 32) & 0xffff) + (h >> 48));
      float x = __fmul_rn((float)(s - 131070), 2.6428997e-05f);
      asm volatile("" : "+v"(x));                       // (the product is rounded before the shift is added: no fused multiply-add)
      if (planted) x = __fadd_rn(x, a.plant_shift);
      if (a.dtype == NMOD_DTYPE_F32) reinterpret_cast<float*>(a.out)[o + read] = x;
      else reinterpret_cast<int16_t*>(a.out)[o + read] = (int16_t)rintf(__fmul_rn(x, 1000.0f));
    }
  }
}

// ---------------------------------------------------------------------------
// K5b synthetic EVENT rows (include/nanomod_hip.h: nmod_synth_fill_events): a level per position (both groups share it)
// plus a per-read spread, on the milli-unit grid of stored NanoMod events.  Integer-only up to the final quotient:
//   level(pos) = (mix(seed ^ kLevelSalt, pos, 0, 0) >> 40) % 6001 - 3000                       milli-units, +-3 units
//   k = level + floor((2 z spread_milli + 37837) / 75674)  [+ shift_milli: planted positions of group 1],  z = s - 131070
// (z has standard deviation 37837.2: k - level is z spread / sd rounded to the nearest milli-unit), clamped to int16;
// float32 output is the float64 quotient k / 1000.0 rounded to float32 — what a stored 3-decimal event value is.
constexpr uint64_t kLevelSalt = 0xA5A5A5A5DEADBEEFull;

__device__ __forceinline__ int synth_event_level(uint64_t seed, int64_t pos) {
  return (int)((synth_mix(seed ^ kLevelSalt, pos, 0, 0u) >> 40) % 6001ull) - 3000;
}
constexpr uint64_t kOutlierSalt = 0x0DDBA11C0FFEE123ull;
// (the quotient's floor in 64 bits: 2 z spread reaches 2.1e9 at spread 8 000)
__device__ __forceinline__ int synth_event_key(uint64_t seed, int64_t pos, int32_t group, uint32_t read, int level, int spread_milli, int shift,
                                               int outlier_permille) {
  const uint64_t h = synth_mix(seed, pos, group, read);
  const int z = (int)((h & 0xffff) + ((h >> 16) & 0xffff) + ((h >> 32) & 0xffff) + (h >> 48)) - 131070;
  constexpr long long kBias = 32768;                             // (floor division through a non-negative numerator)
  const int q = (int)((2ll * z * spread_milli + 37837 + kBias * 75674) / 75674 - kBias);
  int k = level + q + shift;
  if (outlier_permille > 0) {
    // a read in `outlier_permille` of 1 000 is a mis-segmented event: a uniform draw over the +-5 unit clip range of the raw
    // normalisation (myRefBaseSignalAnnotation.py:251-259), whatever the position's level
    const uint64_t o = synth_mix(seed ^ kOutlierSalt, pos, group, read);
    if ((int)((o >> 20) % 1000ull) < outlier_permille) k = (int)((o >> 32) % 10001ull) - 5000;
  }
  return min(max(k, -32767), 32767);
}

struct SynthEventArgs {
  uint64_t seed; int64_t pos_begin; int64_t npos; int32_t group; int32_t n_per_pos; const int64_t* off;
  int64_t plant_period; int32_t plant_shift_milli; int32_t spread_milli; int32_t dtype; int32_t outlier_permille; void* out;
};

// one wave per row (fixed stride or CSR)
__global__ __launch_bounds__(256) void synth_event_kernel(SynthEventArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  for (int64_t rel = wave; rel < a.npos; rel += (int64_t)gridDim.x * 4) {
    const int64_t o = a.n_per_pos > 0 ? rel * (int64_t)a.n_per_pos : a.off[rel];
    const int n = a.n_per_pos > 0 ? a.n_per_pos : (int)(a.off[rel + 1] - o);
    const int64_t pos = a.pos_begin + rel;
    int shift = 0;
    if (a.group == 1 && a.plant_period > 0) {
      const int64_t m = pos % a.plant_period;
      if (m == 0 || m == 1 || m == a.plant_period - 1) shift = a.plant_shift_milli;
    }
    const int level = synth_event_level(a.seed, pos);
    for (int read = lane; read < n; read += 64) {
      const int k = synth_event_key(a.seed, pos, a.group, (uint32_t)read, level, a.spread_milli, shift, a.outlier_permille);
      if (a.dtype == NMOD_DTYPE_F32) reinterpret_cast<float*>(a.out)[o + read] = (float)((double)k / 1000.0);
      else reinterpret_cast<int16_t*>(a.out)[o + read] = (int16_t)k;
    }
  }
}

}  // namespace nmod

using namespace nmod;

extern "C" {

int nmod_synth_fill(const nmod_params* prm, uint64_t seed, int64_t pos_begin, int64_t npos, int32_t group,
                    int32_t n_per_pos, int64_t plant_period, float plant_shift, void* sig_out) {
  int rc = check_params(prm);
  if (rc != NMOD_OK) return rc;
  if (npos < 0 || n_per_pos <= 0 || !sig_out || (group != 0 && group != 1)) return NMOD_ERR_INVALID_ARG;
  if (prm->memspace != NMOD_MEM_DEVICE) return NMOD_ERR_INVALID_ARG;
  if (nmod_device_count() <= prm->device || prm->device < 0) return NMOD_ERR_NO_DEVICE;
  NMOD_HIP(hipSetDevice(prm->device));
  if (npos == 0) return NMOD_OK;
  hipStream_t stream = (hipStream_t)prm->stream;
  SynthArgs sa;
  sa.seed = seed; sa.pos_begin = pos_begin; sa.npos = npos; sa.group = group; sa.n_per_pos = n_per_pos;
  sa.plant_period = plant_period; sa.plant_shift = plant_shift; sa.dtype = prm->dtype; sa.out = sig_out;
  int64_t total = npos * (int64_t)n_per_pos;
  unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 256 * 32);
  ScopedKernelTimer tm(prm->timer, NMOD_KERNEL_SYNTH, stream);
  hipLaunchKernelGGL(synth_kernel, dim3(blocks), dim3(256), 0, stream, sa);
  NMOD_HIP(hipGetLastError());
  return NMOD_OK;
}

int nmod_synth_fill_csr(const nmod_params* prm, uint64_t seed, int64_t pos_begin, int64_t npos, int32_t group,
                        const int64_t* off, int64_t plant_period, float plant_shift, void* sig_out) {
  int rc = check_params(prm);
  if (rc != NMOD_OK) return rc;
  if (npos < 0 || !off || !sig_out || (group != 0 && group != 1)) return NMOD_ERR_INVALID_ARG;
  if (prm->memspace != NMOD_MEM_DEVICE || (prm->dtype != NMOD_DTYPE_F32 && prm->dtype != NMOD_DTYPE_I16_MILLI)) return NMOD_ERR_INVALID_ARG;
  if (nmod_device_count() <= prm->device || prm->device < 0) return NMOD_ERR_NO_DEVICE;
  NMOD_HIP(hipSetDevice(prm->device));
  if (npos == 0) return NMOD_OK;
  hipStream_t stream = (hipStream_t)prm->stream;
  SynthCsrArgs sa;
  sa.seed = seed; sa.pos_begin = pos_begin; sa.npos = npos; sa.group = group; sa.dtype = prm->dtype;
  sa.plant_period = plant_period; sa.plant_shift = plant_shift; sa.off = off; sa.out = sig_out;
  unsigned blocks = (unsigned)std::min<int64_t>((npos + 3) / 4, 256 * 32);
  ScopedKernelTimer tm(prm->timer, NMOD_KERNEL_SYNTH, stream);
  hipLaunchKernelGGL(synth_csr_kernel, dim3(blocks), dim3(256), 0, stream, sa);
  NMOD_HIP(hipGetLastError());
  return NMOD_OK;
}

int nmod_synth_fill_events(const nmod_params* prm, uint64_t seed, int64_t pos_begin, int64_t npos, int32_t group,
                           int32_t n_per_pos, const int64_t* off, int64_t plant_period, int32_t plant_shift_milli,
                           int32_t spread_milli, int32_t outlier_permille, void* sig_out) {
  int rc = check_params(prm);
  if (rc != NMOD_OK) return rc;
  if (npos < 0 || !sig_out || (group != 0 && group != 1) || n_per_pos < 0 || (n_per_pos == 0 && !off)) return NMOD_ERR_INVALID_ARG;
  if (spread_milli < 0 || spread_milli > 8000 || plant_shift_milli < -16000 || plant_shift_milli > 16000 || outlier_permille < 0 || outlier_permille > 1000) return NMOD_ERR_INVALID_ARG;
  if (prm->memspace != NMOD_MEM_DEVICE || (prm->dtype != NMOD_DTYPE_F32 && prm->dtype != NMOD_DTYPE_I16_MILLI)) return NMOD_ERR_INVALID_ARG;
  if (nmod_device_count() <= prm->device || prm->device < 0) return NMOD_ERR_NO_DEVICE;
  NMOD_HIP(hipSetDevice(prm->device));
  if (npos == 0) return NMOD_OK;
  hipStream_t stream = (hipStream_t)prm->stream;
  SynthEventArgs sa;
  sa.seed = seed; sa.pos_begin = pos_begin; sa.npos = npos; sa.group = group; sa.n_per_pos = n_per_pos; sa.off = off;
  sa.plant_period = plant_period; sa.plant_shift_milli = plant_shift_milli; sa.spread_milli = spread_milli; sa.dtype = prm->dtype; sa.outlier_permille = outlier_permille; sa.out = sig_out;
  unsigned blocks = (unsigned)std::min<int64_t>((npos + 3) / 4, 256 * 32);
  ScopedKernelTimer tm(prm->timer, NMOD_KERNEL_SYNTH, stream);
  hipLaunchKernelGGL(synth_event_kernel, dim3(blocks), dim3(256), 0, stream, sa);
  NMOD_HIP(hipGetLastError());
  return NMOD_OK;
}

}  // extern "C"
