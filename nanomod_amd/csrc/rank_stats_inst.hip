// Instantiates K1 for every (R0, R1) size class of one (dtype, tests) pair.
// Built four times by the Makefile: -DNMOD_INST_DTYPE={0,1} -DNMOD_INST_ALL={0,1}.
#include <algorithm>
#include <atomic>
#include "rank_stats.hpp"
#include "rank_stats_packed.hpp"
#include "ks_rank.hpp"
#include "rank_all.hpp"
#include "rank_hist.hpp"
#include "rank_count.hpp"
#include "rank_count_wide.hpp"
#include "rank_count_value.hpp"
#include "rank_stats_launch.hpp"

#ifndef NMOD_INST_DTYPE
#error "define NMOD_INST_DTYPE and NMOD_INST_ALL"
#endif

namespace nmod {

namespace {
constexpr int DT = NMOD_INST_DTYPE;
constexpr bool ALL = NMOD_INST_ALL != 0;
using KernelFn = void (*)(RankStatsArgs);

#if NMOD_INST_ALL
// all-tests builds: rank_hist_kernel for same-class positions, rank_pair_kernel (one position per wave) for the rest
template <int C0, int C1>
constexpr KernelFn kernel_of() { return rank_pair_kernel<(1 << C0), (1 << C1), DT>; }

template <int C0>
KernelFn pick1(int c1) {
  switch (c1) {
    case 0: return kernel_of<C0, 0>();
    case 1: return kernel_of<C0, 1>();
    case 2: return kernel_of<C0, 2>();
    case 3: return kernel_of<C0, 3>();
    case 4: return kernel_of<C0, 4>();
    default: return kernel_of<C0, 5>();
  }
}
KernelFn pick(int c0, int c1) {
  switch (c0) {
    case 0: return pick1<0>(c1);
    case 1: return pick1<1>(c1);
    case 2: return pick1<2>(c1);
    case 3: return pick1<3>(c1);
    case 4: return pick1<4>(c1);
    default: return pick1<5>(c1);
  }
}
KernelFn pick_wide(int cmin) {
  switch (cmin) {
    case 0: return rank_hist_kernel<1, 64, DT, true>;
    case 1: return rank_hist_kernel<2, 64, DT, true>;
    default: return rank_hist_kernel<4, 64, DT, true>;
  }
}
KernelFn pick_packed(int cm, bool after_count) {
  if (after_count) return rank_hist_kernel<16, 16, DT, false, true>;     // (cm == 2: behind rank_count_kernel)
  switch (cm) {
    case 0: return rank_hist_kernel<8, 8, DT>;
    case 1: return rank_hist_kernel<16, 8, DT>;
    case 2: return rank_hist_kernel<16, 16, DT>;
    case 3: return rank_hist_kernel<16, 32, DT>;
    default: return rank_hist_kernel<16, 64, DT>;
  }
}
#else
// KS-only builds carry only the ks_rank kernels
// uniform: a fixed-stride batch without a position list — the instance that holds the sizes and the schedule as launch constants
KernelFn pick_ks(int cs, bool flags, bool uniform) {
#if NMOD_INST_DTYPE == 0
  if (flags) {                 // float32 images of float64 samples: report ties (ks_rank.hpp)
    switch (cs) {
      case 0: return ks_rank_kernel<8, 8, DT, true>;
      case 1: return ks_rank_kernel<16, 8, DT, true>;
      case 2: return ks_rank_kernel<16, 16, DT, true>;
      case 3: return ks_rank_kernel<16, 32, DT, true>;
      case 4: return ks_rank_kernel<16, 64, DT, true>;
      default: return ks_rank_kernel<32, 64, DT, true>;
    }
  }
#endif
  (void)flags;
  if (uniform) {
    switch (cs) {
      case 0: return ks_rank_kernel<8, 8, DT, false, true>;
      case 1: return ks_rank_kernel<16, 8, DT, false, true>;
      case 2: return ks_rank_kernel<16, 16, DT, false, true>;
      case 3: return ks_rank_kernel<16, 32, DT, false, true>;
      case 4: return ks_rank_kernel<16, 64, DT, false, true>;
      default: return ks_rank_kernel<32, 64, DT, false, true>;
    }
  }
  switch (cs) {
    case 0: return ks_rank_kernel<8, 8, DT>;
    case 1: return ks_rank_kernel<16, 8, DT>;
    case 2: return ks_rank_kernel<16, 16, DT>;
    case 3: return ks_rank_kernel<16, 32, DT>;
    case 4: return ks_rank_kernel<16, 64, DT>;
    default: return ks_rank_kernel<32, 64, DT>;
  }
}
#endif

// The dynamic-LDS attribute (lds_limit, else lds) and the occupancy of a kernel at `lds`, looked up once per device and kept in
// `slot` (atomics: concurrent first launches both run the queries and store the same number); slot null: looked up every time
hipError_t blocks_per_cu(std::atomic<int>* slot, const void* fn, size_t lds, int* per_cu, size_t lds_limit = 0) {
  int pc = slot ? slot->load(std::memory_order_relaxed) : 0;
  if (pc <= 0) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(lds_limit ? lds_limit : lds));
    if (e != hipSuccess) return e;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&pc, fn, 64 * kWavesPerBlock, lds);
    if (e != hipSuccess) return e;
    if (pc < 1) return hipErrorLaunchOutOfResources;     // (never launch a block that cannot get its LDS: its table walks would not end)
    if (slot) slot->store(pc, std::memory_order_relaxed);
  }
  *per_cu = pc;
  return hipSuccess;
}
constexpr int kCacheDevices = 64;
int cache_device() {                                     // index of the per-device caches, -1: not cacheable
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < kCacheDevices ? dev : -1;
}
int64_t grid_of(int64_t work_items, int num_cus, int per_cu) {
  return std::max<int64_t>(1, std::min<int64_t>((work_items + kWavesPerBlock - 1) / kWavesPerBlock, (int64_t)num_cus * per_cu));
}

hipError_t launch_rank_stats(int cls, int num_cus, int64_t work_items, hipStream_t stream, const RankStatsArgs& args) {
  const bool ks = cls >= kKsClassBase && cls < kNumClasses;
  const bool packed = cls >= kNumGeneralClasses && cls < kKsClassBase;
  KernelFn fn = nullptr;
#if NMOD_INST_ALL
  if (ks) return hipErrorInvalidValue;
  const bool wide = wide_class(cls);
  // capacity-256 positions with all tests: the counting form first (rank_count.hpp) when the caller provided its gate and flags
  const bool counting = packed && cls - kNumGeneralClasses == 2 && args.cnt_gate != nullptr && args.cnt_done != nullptr;
  fn = packed ? pick_packed(cls - kNumGeneralClasses, counting)
       : wide ? pick_wide(wide_class_of_s(cls))
              : pick(cls / kNumSizeClasses, cls % kNumSizeClasses);
#else
  if (!ks) return hipErrorInvalidValue;
  const bool ks_uniform = args.tied == nullptr && args.stride0 > 0 && args.stride1 > 0 && args.pos_list == nullptr && args.alt_gates == nullptr;
  fn = pick_ks(cls - kKsClassBase, args.tied != nullptr, ks_uniform);
#endif
  const size_t lds = rank_stats_lds_bytes(cls, ALL, DT);
  if (ks || packed) {
    const int pw = ks ? ksonly_positions_per_wave(cls - kKsClassBase) : packed_positions_per_wave(cls - kNumGeneralClasses);
    work_items = (work_items + pw - 1) / pw;
  }
  // [class], [kClassStride + class] for the FLAGS instances, [2 * kClassStride + class] for the fixed-stride KS instances
  static std::atomic<int> per_cu_cache[kCacheDevices][3 * kClassStride];
  const int dev = cache_device();
#if NMOD_INST_ALL
  const int slot_id = cls + (counting ? kClassStride : 0);
  // (one WIDE instance serves every class of the larger group: its limit is that of the largest)
  const size_t lds_limit = wide ? rank_stats_lds_bytes(kWideBigBase + wide_class_of_s(cls), ALL, DT) : lds;
#else
  const int slot_id = cls + ((ks && args.tied) ? kClassStride : ks_uniform ? 2 * kClassStride : 0);
  const size_t lds_limit = lds;
#endif
  int per_cu = 0;
  hipError_t e = blocks_per_cu(dev >= 0 ? &per_cu_cache[dev][slot_id] : nullptr, reinterpret_cast<const void*>(fn), lds, &per_cu, lds_limit);
  if (e != hipSuccess) return e;
#if NMOD_INST_ALL
  if (counting) {
    // probe (one block: is the batch event-like?) -> rank_count_kernel (exits at once when it is not) -> the AFTER instance below
    CntProbeArgs pa;
    pa.sig0 = args.sig0; pa.sig1 = args.sig1; pa.off0 = args.off0; pa.off1 = args.off1; pa.stride0 = args.stride0; pa.stride1 = args.stride1;
    pa.npos = args.npos; pa.pos_list = args.pos_list; pa.class_meta = args.class_meta; pa.class_id = args.class_id; pa.dtype = DT; pa.gate = args.cnt_gate;
    // (float32 keys of float64 samples — args.tied is set — are whole numbers where the samples sit on the 0.001 grid: DTYPE 2)
#if NMOD_INST_DTYPE == 0
    const bool int_keys = args.tied != nullptr;
    if (int_keys) hipLaunchKernelGGL(cnt_probe_kernel<2>, dim3(1), dim3(1024), 0, stream, pa);
    else hipLaunchKernelGGL(cnt_probe_kernel<0>, dim3(1), dim3(1024), 0, stream, pa);
    static std::atomic<int> cnt_per_cu[kCacheDevices][2];
    KernelFn cfn = int_keys ? (KernelFn)rank_count_kernel<2> : (KernelFn)rank_count_kernel<0>;
    std::atomic<int>* cslot = dev >= 0 ? &cnt_per_cu[dev][int_keys ? 1 : 0] : nullptr;
#else
    hipLaunchKernelGGL(cnt_probe_kernel<DT>, dim3(1), dim3(1024), 0, stream, pa);
    static std::atomic<int> cnt_per_cu[kCacheDevices][1];
    KernelFn cfn = rank_count_kernel<DT>;
    std::atomic<int>* cslot = dev >= 0 ? &cnt_per_cu[dev][0] : nullptr;
#endif
    const size_t clds = rank_count_lds_bytes();
    int cpc = 0;
    e = blocks_per_cu(cslot, reinterpret_cast<const void*>(cfn), clds, &cpc);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(cfn, dim3((unsigned)grid_of(work_items, num_cus, cpc)), dim3(64 * kWavesPerBlock), clds, stream, args);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
#endif
  const int64_t blocks = grid_of(work_items, num_cus, per_cu);
#if NMOD_INST_ALL
  if (counting) {
    // gate clear: the plain instance over the whole list; gate set: the AFTER instance over what the counting form left
    RankStatsArgs a2 = args;
    a2.cnt_mode = 1;
    KernelFn plain = pick_packed(cls - kNumGeneralClasses, false);
    static std::atomic<int> plain_per_cu[kCacheDevices];
    int ppc = 0;                                         // (the plain instance runs on the AFTER instance's grid)
    e = blocks_per_cu(dev >= 0 ? &plain_per_cu[dev] : nullptr, reinterpret_cast<const void*>(plain), lds, &ppc);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(plain, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), lds, stream, a2);
    a2.cnt_mode = 2;
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), lds, stream, a2);
    return hipGetLastError();
  }
#endif
  hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), lds, stream, args);
  return hipGetLastError();
}

hipError_t count_wide_prepare(const int* classes, int nclasses, hipStream_t stream, const RankStatsArgs& a, const CountWideWs& w) {
  if (nclasses <= 0) return hipSuccess;
  if (nclasses > kClassStride) return hipErrorInvalidValue;        // (cls[] / max_s[] / the segs area hold one entry per class)
  CntWideProbeArgs pa;
  pa.sig0 = a.sig0; pa.sig1 = a.sig1; pa.off0 = a.off0; pa.off1 = a.off1; pa.stride0 = a.stride0; pa.stride1 = a.stride1; pa.npos = a.npos;
  pa.pos_list = a.pos_list; pa.class_meta = a.class_meta; pa.nclasses = nclasses; pa.gate = w.gates; pa.segs = w.gates + kClassStride; pa.work_meta = w.work_meta; pa.min_q = NMOD_INST_ALL ? 0 : kCwKsMinQ;
  for (int i = 0; i < nclasses && i < kClassStride; ++i) { pa.cls[i] = classes[i]; pa.max_s[i] = 64 << count_wide_rs_index(classes[i]); }
  hipError_t e = hipMemsetAsync(w.gates, 0, kClassStride * 4, stream);
  if (e != hipSuccess) return e;
#if NMOD_INST_DTYPE == 0
  if (a.tied != nullptr) hipLaunchKernelGGL(HIP_KERNEL_NAME(cnt_wide_probe_kernel<2, NMOD_INST_ALL == 0>), dim3((unsigned)nclasses), dim3(1024), 0, stream, pa);
  else hipLaunchKernelGGL(HIP_KERNEL_NAME(cnt_wide_probe_kernel<0, NMOD_INST_ALL == 0>), dim3((unsigned)nclasses), dim3(1024), 0, stream, pa);
#else
  hipLaunchKernelGGL(HIP_KERNEL_NAME(cnt_wide_probe_kernel<1, NMOD_INST_ALL == 0>), dim3((unsigned)nclasses), dim3(1024), 0, stream, pa);
#endif
  return hipGetLastError();
}

hipError_t count_wide_run(int num_cus, int64_t work_items, hipStream_t stream, const RankStatsArgs& a, const CountWideWs& w, bool value_class) {
  typedef void (*CwFn)(CntWideArgs);
#if NMOD_INST_DTYPE == 0
  const bool int_keys = a.tied != nullptr;
  CwFn fn = int_keys ? (CwFn)rank_count_wide_kernel<2, NMOD_INST_ALL == 0> : (CwFn)rank_count_wide_kernel<0, NMOD_INST_ALL == 0>;
  CwFn vfn = int_keys ? (CwFn)rank_count_value_kernel<2, NMOD_INST_ALL == 0> : (CwFn)rank_count_value_kernel<0, NMOD_INST_ALL == 0>;
  const int slot = int_keys ? 1 : 0;
#else
  CwFn fn = (CwFn)rank_count_wide_kernel<1, NMOD_INST_ALL == 0>;
  CwFn vfn = (CwFn)rank_count_value_kernel<1, NMOD_INST_ALL == 0>;
  const int slot = 0;
#endif
  static std::atomic<int> per_cu[kCacheDevices][2], vper_cu[kCacheDevices][2];
  const int dev = cache_device();
  const size_t lds = rank_count_wide_lds_bytes();
  int pc = 0;
  hipError_t e = blocks_per_cu(dev >= 0 ? &per_cu[dev][slot] : nullptr, reinterpret_cast<const void*>(fn), lds, &pc);
  if (e != hipSuccess) return e;
  CntWideArgs ca;
  ca.rs = a; ca.gates = w.gates; ca.segs = w.gates + kClassStride; ca.work_list = w.work_list; ca.work_meta = w.work_meta;
  hipLaunchKernelGGL(fn, dim3((unsigned)grid_of(work_items, num_cus, pc)), dim3(64 * kWavesPerBlock), lds, stream, ca);
  if (value_class) {
    // the class whose groups both hold more than 1 024 samples: the value-domain form (rank_count_value.hpp), a launch of its own
    const size_t vlds = rank_count_value_lds_bytes();
    int vpc = 0;
    e = blocks_per_cu(dev >= 0 ? &vper_cu[dev][slot] : nullptr, reinterpret_cast<const void*>(vfn), vlds, &vpc);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(vfn, dim3((unsigned)grid_of(work_items, num_cus, vpc)), dim3(64 * kWavesPerBlock), vlds, stream, ca);
  }
  return hipGetLastError();
}
}  // namespace

#define NMOD_CAT2(a, b) a##b
#define NMOD_CAT(a, b) NMOD_CAT2(a, b)
#define NMOD_K1_NAME NMOD_CAT(NMOD_CAT(k1_d, NMOD_INST_DTYPE), NMOD_CAT(_a, NMOD_INST_ALL))
const K1Launcher& NMOD_K1_NAME() {
  static const K1Launcher k1 = {launch_rank_stats, count_wide_prepare, count_wide_run};
  return k1;
}

}  // namespace nmod
