// The HIP-event timer behind nmod_params::timer (nmod_evtimer_*, evtimer.hip): the record and the scope that the units which
// time their launches put around them.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

#include "entry_common.hpp"

namespace nmod {

struct EvTimer {
  int capacity;
  std::vector<hipEvent_t> start[NMOD_KERNEL_COUNT], stop[NMOD_KERNEL_COUNT];
  int used[NMOD_KERNEL_COUNT];
};

// A slot counts only when BOTH of its events were recorded: a failed hipEventRecord drops the sample (and is
// remembered in g_last_hip) instead of leaving an event pair that nmod_evtimer_read would fail on.
struct ScopedKernelTimer {
  EvTimer* t; int k; hipStream_t s; int slot;
  ScopedKernelTimer(void* timer, int kernel, hipStream_t stream) : t((EvTimer*)timer), k(kernel), s(stream), slot(-1) {
    if (t && t->used[k] < t->capacity) {
      const hipError_t e = hipEventRecord(t->start[k][t->used[k]], s);
      if (e == hipSuccess) slot = t->used[k]; else g_last_hip = e;
    }
  }
  ~ScopedKernelTimer() {
    if (slot >= 0) {
      const hipError_t e = hipEventRecord(t->stop[k][slot], s);
      if (e == hipSuccess) t->used[k] = slot + 1; else g_last_hip = e;
    }
  }
};

}  // namespace nmod
