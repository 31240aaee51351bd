// nmod_strerror and the per-thread records its text is made from: the last HIP error (NMOD_HIP, entry_common.hpp) and the
// last RCCL error (comm.hip).
#include <hip/hip_runtime.h>
#include <stdio.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"

namespace nmod {

thread_local hipError_t g_last_hip = hipSuccess;
thread_local int g_last_rccl = 0;
thread_local const char* g_last_rccl_text = nullptr;
static thread_local char g_errbuf[256];

}  // namespace nmod

using namespace nmod;

extern "C" const char* nmod_strerror(int rc) {
  switch (rc) {
    case NMOD_OK: return "ok";
    case NMOD_ERR_INVALID_ARG: return "invalid argument";
    case NMOD_ERR_HIP:
      snprintf(g_errbuf, sizeof(g_errbuf), "HIP runtime error: %s", hipGetErrorString(g_last_hip));
      return g_errbuf;
    case NMOD_ERR_TOO_LARGE: return "a position has more samples in a group than NMOD_MAX_RANKED (65535; NMOD_MAX_DEEP with NMOD_FLAG_DEEP)";
    case NMOD_ERR_WORKSPACE: return "workspace missing or smaller than nmod_workspace_bytes()";
    case NMOD_ERR_NO_DEVICE: return "no HIP device";
    case NMOD_ERR_NO_RCCL: return "librccl.so could not be bound (neither loaded in this process nor on the loader path)";
    case NMOD_ERR_RCCL:
      snprintf(g_errbuf, sizeof(g_errbuf), "RCCL error %d: %s", g_last_rccl, g_last_rccl_text ? g_last_rccl_text : "?");
      return g_errbuf;
    default: return "unknown error code";
  }
}
