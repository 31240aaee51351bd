// nmod_comm_* and nmod_allgather_tracks: the torch-free all-gather of result tracks over RCCL, bound at run time.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <stdint.h>
#include <string.h>
#include <mutex>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"

namespace nmod {

// No link-time dependency: a PyTorch process already holds torch's librccl.so (its "nccl" backend) and a second copy beside it
// would be a second set of communicator state; a process without one takes librccl.so.1 from the loader path.
struct IdByValue { char internal[NMOD_COMM_ID_BYTES]; };      // ncclUniqueId is passed by value
struct RcclApi {
  void* handle = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, IdByValue, int) = nullptr;
  int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
static RcclApi* rccl_api() {
  static std::once_flag once;
  static RcclApi api;
  static bool ok = false;
  std::call_once(once, [] {
    const char* names[] = {"librccl.so", "librccl.so.1"};
    for (const char* n : names) { api.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD); if (api.handle) break; }     // a copy the process already holds
    if (!api.handle) for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { api.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL); if (api.handle) break; }
    if (!api.handle) return;
    auto sym = [&](const char* n) { return dlsym(api.handle, n); };
    api.GetUniqueId = (int (*)(void*))sym("ncclGetUniqueId");
    api.CommInitRank = (int (*)(void**, int, IdByValue, int))sym("ncclCommInitRank");
    api.AllGather = (int (*)(const void*, void*, size_t, int, void*, hipStream_t))sym("ncclAllGather");
    api.GroupStart = (int (*)())sym("ncclGroupStart");
    api.GroupEnd = (int (*)())sym("ncclGroupEnd");
    api.CommDestroy = (int (*)(void*))sym("ncclCommDestroy");
    api.GetErrorString = (const char* (*)(int))sym("ncclGetErrorString");
    ok = api.GetUniqueId && api.CommInitRank && api.AllGather && api.GroupStart && api.GroupEnd && api.CommDestroy;
  });
  return ok ? &api : nullptr;
}
// (g_last_rccl, g_last_rccl_text: errors.hip, for nmod_strerror)
#define NMOD_RCCL(api, call)                                                                         \
  do {                                                                                               \
    const int r_ = (call);                                                                           \
    if (r_ != 0) { g_last_rccl = r_; g_last_rccl_text = (api)->GetErrorString ? (api)->GetErrorString(r_) : nullptr; return NMOD_ERR_RCCL; } \
  } while (0)
constexpr int kNcclFloat64 = 8;                  // ncclDataType_t: ncclFloat64 / ncclDouble

}  // namespace nmod

using namespace nmod;

struct nmod_comm { void* comm; int nranks, rank, device; };

extern "C" {

int nmod_comm_unique_id(void* id_out) {
  if (!id_out) return NMOD_ERR_INVALID_ARG;
  RcclApi* api = rccl_api();
  if (!api) return NMOD_ERR_NO_RCCL;
  NMOD_RCCL(api, api->GetUniqueId(id_out));
  return NMOD_OK;
}

int nmod_comm_init_rank(const void* unique_id, int32_t nranks, int32_t rank, int32_t device, nmod_comm** comm_out) {
  if (!unique_id || !comm_out || nranks < 1 || rank < 0 || rank >= nranks) return NMOD_ERR_INVALID_ARG;
  *comm_out = nullptr;
  if (nmod_device_count() <= device || device < 0) return NMOD_ERR_NO_DEVICE;
  RcclApi* api = rccl_api();
  if (!api) return NMOD_ERR_NO_RCCL;
  NMOD_HIP(hipSetDevice(device));
  IdByValue id;
  memcpy(id.internal, unique_id, NMOD_COMM_ID_BYTES);
  void* c = nullptr;
  NMOD_RCCL(api, api->CommInitRank(&c, nranks, id, rank));
  nmod_comm* h = new nmod_comm();
  h->comm = c; h->nranks = nranks; h->rank = rank; h->device = device;
  *comm_out = h;
  return NMOD_OK;
}

int nmod_allgather_tracks(nmod_comm* comm, void* stream, int64_t block_len, int32_t ntracks, const double* const* local, double* const* full) {
  if (!comm || !comm->comm || block_len < 0 || ntracks < 0 || ntracks > 64 || (ntracks > 0 && (!local || !full))) return NMOD_ERR_INVALID_ARG;
  for (int t = 0; t < ntracks; ++t) if (!local[t] || !full[t]) return NMOD_ERR_INVALID_ARG;
  if (block_len == 0 || ntracks == 0) return NMOD_OK;
  RcclApi* api = rccl_api();
  if (!api) return NMOD_ERR_NO_RCCL;
  NMOD_HIP(hipSetDevice(comm->device));
  // one group: the tracks' gathers are fused into one launch on the caller's stream; nothing is synchronised here
  NMOD_RCCL(api, api->GroupStart());
  int first_bad = 0;
  for (int t = 0; t < ntracks; ++t) {
    const int r = api->AllGather(local[t], full[t], (size_t)block_len, kNcclFloat64, comm->comm, (hipStream_t)stream);
    if (r != 0 && first_bad == 0) first_bad = r;
  }
  const int rend = api->GroupEnd();
  if (first_bad != 0 || rend != 0) { g_last_rccl = first_bad ? first_bad : rend; g_last_rccl_text = api->GetErrorString ? api->GetErrorString(g_last_rccl) : nullptr; return NMOD_ERR_RCCL; }
  return NMOD_OK;
}

int nmod_comm_destroy(nmod_comm* comm) {
  if (!comm) return NMOD_ERR_INVALID_ARG;
  RcclApi* api = rccl_api();
  int rc = NMOD_OK;
  if (api && comm->comm) { const int r = api->CommDestroy(comm->comm); if (r != 0) { g_last_rccl = r; g_last_rccl_text = api->GetErrorString ? api->GetErrorString(r) : nullptr; rc = NMOD_ERR_RCCL; } }
  delete comm;
  return rc;
}

}  // extern "C"
