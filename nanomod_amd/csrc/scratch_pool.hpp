// The library's per-device scratch pool (nanomod_hip.hip: scratch_pool) and the stream-ordered slab taken from it, shared by
// the translation units that need large temporary buffers (the large-position and deep passes, the read pivot).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace nmod {

hipMemPool_t scratch_pool(int dev);      // created on first use; nmod_trim_scratch returns its cached slabs to the driver

struct DevScratch {
  void* p = nullptr; bool async = false; hipStream_t owner = nullptr;
  hipError_t alloc(size_t bytes, hipStream_t s, int dev) {
    owner = s;
    hipMemPool_t pool = scratch_pool(dev);
    if (pool && hipMallocFromPoolAsync(&p, bytes ? bytes : 4, pool, s) == hipSuccess) { async = true; return hipSuccess; }
    (void)hipGetLastError();
    p = nullptr;
    return hipMalloc(&p, bytes ? bytes : 4);
  }
  hipError_t release(hipStream_t s) {
    hipError_t e = hipSuccess;
    if (p) e = async ? hipFreeAsync(p, s) : (hipStreamSynchronize(s), hipFree(p));
    p = nullptr;
    return e;
  }
  // an early return (error path) with kernels of the allocation stream still queued: the slab goes back to the pool
  // ordered behind them on THAT stream — freeing on the null stream does not order against a non-blocking stream
  ~DevScratch() { if (p) { if (async) hipFreeAsync(p, owner); else { hipStreamSynchronize(owner); hipFree(p); } } }
};

}  // namespace nmod
