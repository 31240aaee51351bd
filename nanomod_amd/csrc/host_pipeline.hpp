// The host-resident entry (NMOD_MEM_HOST, host_pipeline.hip) as the rest of the library sees it.
#pragma once
#include <stdint.h>

#include "../../include/nanomod_hip.h"

namespace nmod {

// nmod_detect_batch of a batch in host memory, chunked through pinned slots on the unit's own three streams.  stats_totals:
// kStatsWords (detect_internal.hpp) dispatch counters of the whole call, read back before it returns.
int detect_host_pipelined(const nmod_params* prm, int64_t npos, const void* sig0, const int64_t* off0,
                          const void* sig1, const int64_t* off1, const int32_t* run_id, nmod_out* out,
                          unsigned long long* stats_totals);

// frees the device's cached pinned ring and streams unless a call is using them (nmod_trim_scratch); 0 <= dev < kMaxDevices
void hp_trim(int dev);

}  // namespace nmod
