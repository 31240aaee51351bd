// nmod_evtimer_*: creating, resetting, reading and destroying the HIP-event timer of evtimer.hpp.
#include <hip/hip_runtime.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "evtimer.hpp"

using namespace nmod;

extern "C" {

int nmod_evtimer_create(int32_t capacity_per_kernel, void** timer) {
  if (!timer || capacity_per_kernel <= 0) return NMOD_ERR_INVALID_ARG;
  EvTimer* t = new EvTimer();
  t->capacity = capacity_per_kernel;
  for (int k = 0; k < NMOD_KERNEL_COUNT; ++k) {
    t->used[k] = 0;
    t->start[k].assign(capacity_per_kernel, nullptr); t->stop[k].assign(capacity_per_kernel, nullptr);
  }
  for (int k = 0; k < NMOD_KERNEL_COUNT; ++k) {
    for (int i = 0; i < capacity_per_kernel; ++i) {
      hipError_t e = hipEventCreate(&t->start[k][i]);
      if (e == hipSuccess) e = hipEventCreate(&t->stop[k][i]);
      if (e != hipSuccess) {                       // free what was created so far
        g_last_hip = e;
        for (int kk = 0; kk < NMOD_KERNEL_COUNT; ++kk)
          for (int ii = 0; ii < capacity_per_kernel; ++ii) {
            if (t->start[kk][ii]) hipEventDestroy(t->start[kk][ii]);
            if (t->stop[kk][ii]) hipEventDestroy(t->stop[kk][ii]);
          }
        delete t;
        return NMOD_ERR_HIP;
      }
    }
  }
  *timer = t;
  return NMOD_OK;
}

int nmod_evtimer_reset(void* timer) {
  if (!timer) return NMOD_ERR_INVALID_ARG;
  EvTimer* t = (EvTimer*)timer;
  for (int k = 0; k < NMOD_KERNEL_COUNT; ++k) t->used[k] = 0;
  return NMOD_OK;
}

int nmod_evtimer_read(void* timer, int32_t kernel, double* total_ms, int32_t* launches) {
  if (!timer || kernel < 0 || kernel >= NMOD_KERNEL_COUNT || !total_ms || !launches) return NMOD_ERR_INVALID_ARG;
  EvTimer* t = (EvTimer*)timer;
  double tot = 0.0;
  for (int i = 0; i < t->used[kernel]; ++i) {
    float ms = 0.f;
    NMOD_HIP(hipEventSynchronize(t->stop[kernel][i]));
    NMOD_HIP(hipEventElapsedTime(&ms, t->start[kernel][i], t->stop[kernel][i]));
    tot += ms;
  }
  *total_ms = tot; *launches = t->used[kernel];
  return NMOD_OK;
}

int nmod_evtimer_destroy(void* timer) {
  if (!timer) return NMOD_ERR_INVALID_ARG;
  EvTimer* t = (EvTimer*)timer;
  for (int k = 0; k < NMOD_KERNEL_COUNT; ++k)
    for (int i = 0; i < t->capacity; ++i) { hipEventDestroy(t->start[k][i]); hipEventDestroy(t->stop[k][i]); }
  delete t;
  return NMOD_OK;
}

}  // extern "C"
