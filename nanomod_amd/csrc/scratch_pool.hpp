// The library's per-device scratch pool (scratch_pool.hip) and the stream-ordered slab taken from it, shared by
// the translation units that need large temporary buffers (the large-position and deep passes, the read pivot).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace nmod {

hipMemPool_t scratch_pool(int dev);      // created on first use; nmod_trim_scratch returns its cached slabs to the driver

// Slabs parked per stream (scratch_pool.hip).  The entries that promise not to synchronise do not give their slab back to the pool at
// the end of a call: hipFreeAsync of a block that the pool handed out again while its previous free was still pending on the stream
// waits on the host for that free (measured on ROCm 7: the second of two equal calls on a busy stream returned only when the first had
// run, whatever the pool's reuse attributes).  Such a slab is parked under its (device, stream) instead, and the next call on that
// stream takes it from there: ordered by the stream itself, no pool call in the steady state.  At most kParkSlots slabs per stream (the
// smallest gives way, stream-ordered) and kParkStreams streams (a stream all of whose parked slabs are idle — an event recorded behind
// each says so — gives way to a new one; with none idle the slab is freed to the pool as before).  nmod_trim_scratch frees them all.
constexpr int kParkStreams = 32, kParkSlots = 2;
void* parked_take(int dev, hipStream_t s, size_t need, size_t* bytes);   // a parked slab of (dev, s) of at least `need` bytes (*bytes: its size), or null
hipError_t parked_put(int dev, hipStream_t s, void* p, size_t bytes);    // parks p behind the work queued on s, or frees it stream-ordered
hipError_t parked_trim(int dev, size_t* freed_bytes, size_t* free_before);  // frees every parked slab of the device (their bytes; the device's free memory before); synchronises it

struct DevScratch {
  void* p = nullptr; bool async = false; hipStream_t owner = nullptr;
  bool park = false; int dev = 0; size_t bytes = 0;                      // park: set before alloc by the callers that must not wait (see above)
  hipError_t alloc(size_t b, hipStream_t s, int d) {
    owner = s; dev = d; bytes = b ? b : 4;
    if (park && (p = parked_take(d, s, bytes, &bytes)) != nullptr) { async = true; return hipSuccess; }
    hipMemPool_t pool = scratch_pool(d);
    if (pool && hipMallocFromPoolAsync(&p, bytes, pool, s) == hipSuccess) { async = true; return hipSuccess; }
    (void)hipGetLastError();
    p = nullptr;
    return hipMalloc(&p, bytes);
  }
  hipError_t release(hipStream_t s) {
    hipError_t e = hipSuccess;
    if (p) e = async ? give_back(s) : (hipStreamSynchronize(s), hipFree(p));
    p = nullptr;
    return e;
  }
  // an early return (error path) with kernels of the allocation stream still queued: the slab goes back
  // ordered behind them on THAT stream — freeing on the null stream does not order against a non-blocking stream
  ~DevScratch() { if (p) { if (async) (void)give_back(owner); else { hipStreamSynchronize(owner); hipFree(p); } } }

 private:
  hipError_t give_back(hipStream_t s) { return park ? parked_put(dev, s, p, bytes) : hipFreeAsync(p, s); }
};

}  // namespace nmod
