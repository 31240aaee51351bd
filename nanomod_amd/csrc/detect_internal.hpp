// What the detect unit (nanomod_hip.hip) shares with the other translation units: the parameter check, one device-resident
// batch (detect_device, detect_f64), the window combine and the dispatch-statistics reduction.  Declarations only: the K1 / K2 /
// K3 kernels and the workspace layout stay private to the detect unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nanomod_hip.h"

namespace nmod {

// the checks of nmod_params of the detect entries and of those that reuse its fields (synth, down-sampling)
int check_params(const nmod_params* prm);

// K3 over a KS track in device memory, on `stream`
int launch_combine(const nmod_params* prm, hipStream_t stream, int64_t npos, const double* ks_d, const double* ks_p,
                   const int32_t* run_id, double* comb_st, double* comb_p);

// ---------------------------------------------------------------- dispatch statistics (nmod_last_dispatch_stats)
// Which K1 form took how many positions of a batch is decided on the device (class lists, the probes' gates, the counting forms'
// per-position flags) and never leaves it on the hot path.  detect_device returns where those facts sit in the caller's
// workspace (StatsArgs); dispatch_stats_kernel reduces them to kStatsWords counters when somebody asks (device-resident batches: on request,
// nothing is launched otherwise; host-resident batches: once per chunk into a per-call accumulator, the path is PCIe-bound).
constexpr int kStatsWords = 256;
struct StatsArgs {
  int64_t npos; int32_t uniform_cls;             // >= 0: one class holds all npos positions (no class lists were built)
  const int32_t* meta; const int32_t* work_meta; const int32_t* gates; const uint8_t* cnt_done;
  int32_t cnt256_ran, cw_ran, f64;
  unsigned long long* acc;
};
hipError_t enqueue_dispatch_stats(const StatsArgs& a, hipStream_t stream);

struct F64Src;                                   // the float64 samples behind float32 keys: detect_f64's own, null for every other caller

// One batch in device memory on prm->stream.  stats (may be null): where the facts of nmod_last_dispatch_stats sit in `workspace`.
int detect_device(const nmod_params* prm, int64_t npos, const void* sig0, const int64_t* off0,
                  const void* sig1, const int64_t* off1, const int32_t* run_id, void* workspace,
                  int64_t workspace_bytes, nmod_out* out, StatsArgs* stats, const F64Src* f64 = nullptr);

// The float64 front end: order-preserving float32 keys per position, then detect_device on them.  bounds: the first and
// one-past-last element of each array in use, {b0, e0, b1, e1}, when the caller knows them (no round trip for the offsets).
int detect_f64(const nmod_params* prm, int64_t npos, const void* sig0, const int64_t* off0,
               const void* sig1, const int64_t* off1, const int32_t* run_id, void* workspace,
               int64_t workspace_bytes, nmod_out* out, StatsArgs* stats, const int64_t* bounds = nullptr);

}  // namespace nmod
