// The library's per-device scratch pool and the slabs parked per stream (scratch_pool.hpp), and nmod_trim_scratch, which hands
// all of it (and the host-resident entry's pinned ring) back to the driver.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <chrono>
#include <mutex>
#include <thread>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "host_pipeline.hpp"
#include "scratch_pool.hpp"

namespace nmod {

// Scratch slab of the large-position pass: stream-ordered allocation from a memory pool the LIBRARY owns (one per
// device, created on first use).  Freed slabs stay in that pool (release threshold = max: with the default
// threshold every batch would return its slab to the OS at the next synchronisation and map it again — measured
// 20 ms per 1.3 GB); the device's default pool, which the caller's own hipMallocAsync traffic uses, is never
// touched.  nmod_trim_scratch() returns the cached slabs to the driver.
static std::mutex g_pool_mutex;
static hipMemPool_t g_pool[kMaxDevices] = {nullptr};        // guarded by g_pool_mutex

hipMemPool_t scratch_pool(int dev) {
  if (dev < 0 || dev >= kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> lock(g_pool_mutex);
  if (!g_pool[dev]) {
    hipMemPoolProps props;
    memset(&props, 0, sizeof(props));
    props.allocType = hipMemAllocationTypePinned;
    props.handleTypes = hipMemHandleTypeNone;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &props) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    uint64_t keep = UINT64_MAX;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    g_pool[dev] = pool;
  }
  return g_pool[dev];
}

// The slabs parked per stream (scratch_pool.hpp says why).  One small table under one mutex; no HIP call that can wait is made
// while it is held.
namespace {
struct ParkedBlock { void* p = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; };
struct ParkedStream { bool live = false; int dev = 0; hipStream_t s = nullptr; uint64_t used = 0; ParkedBlock b[kParkSlots]; };
std::mutex g_park_mutex;
ParkedStream g_park[kParkStreams];                            // guarded by g_park_mutex
uint64_t g_park_clock = 0;

ParkedStream* parked_find(int dev, hipStream_t s) {
  for (ParkedStream& e : g_park) if (e.live && e.dev == dev && e.s == s) return &e;
  return nullptr;
}
bool parked_idle(const ParkedStream& e) {
  for (const ParkedBlock& b : e.b) if (b.p && hipEventQuery(b.done) != hipSuccess) { (void)hipGetLastError(); return false; }
  return true;
}
}  // namespace

void* parked_take(int dev, hipStream_t s, size_t need, size_t* bytes) {
  std::lock_guard<std::mutex> lock(g_park_mutex);
  ParkedStream* e = parked_find(dev, s);
  if (!e) return nullptr;
  ParkedBlock* best = nullptr;
  for (ParkedBlock& b : e->b) if (b.p && b.bytes >= need && (!best || b.bytes < best->bytes)) best = &b;
  if (!best) return nullptr;
  e->used = ++g_park_clock;
  void* p = best->p;
  *bytes = best->bytes;
  best->p = nullptr;                                          // (the slot keeps its event for the next slab)
  return p;
}

hipError_t parked_put(int dev, hipStream_t s, void* p, size_t bytes) {
  void* to_free[kParkSlots + 1]; int nfree = 0;               // freed on s after the table is released: all of them are idle or were last used on s
  {
    std::lock_guard<std::mutex> lock(g_park_mutex);
    ParkedStream* e = parked_find(dev, s);
    if (!e) {
      ParkedStream* lru = nullptr;
      for (ParkedStream& c : g_park) {
        if (!c.live) { e = &c; break; }
        if ((!lru || c.used < lru->used) && parked_idle(c)) lru = &c;
      }
      if (!e && lru) {
        for (ParkedBlock& b : lru->b) if (b.p) { to_free[nfree++] = b.p; b.p = nullptr; }
        e = lru;
      }
      if (e) { e->live = true; e->dev = dev; e->s = s; }
    }
    if (!e) to_free[nfree++] = p;                             // every stream of the table is busy
    else {
      e->used = ++g_park_clock;
      ParkedBlock* slot = nullptr;
      for (ParkedBlock& b : e->b) if (!b.p) { slot = &b; break; }
      if (!slot) for (ParkedBlock& b : e->b) if (b.bytes < bytes && (!slot || b.bytes < slot->bytes)) slot = &b;
      if (slot && !slot->done && hipEventCreateWithFlags(&slot->done, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); slot->done = nullptr; slot = nullptr; }
      if (slot && hipEventRecord(slot->done, s) == hipSuccess) {
        if (slot->p) to_free[nfree++] = slot->p;              // the smallest gives way
        slot->p = p; slot->bytes = bytes;
      } else {
        (void)hipGetLastError();
        to_free[nfree++] = p;
      }
    }
  }
  hipError_t err = hipSuccess;
  for (int i = 0; i < nfree; ++i) { const hipError_t e = hipFreeAsync(to_free[i], s); if (e != hipSuccess) err = e; }
  return err;
}

hipError_t parked_trim(int dev, size_t* freed_bytes, size_t* free_before) {
  *freed_bytes = 0; *free_before = 0;
  void* blocks[kParkStreams * kParkSlots]; hipStream_t on[kParkStreams * kParkSlots]; int n = 0;
  {
    std::lock_guard<std::mutex> lock(g_park_mutex);
    for (ParkedStream& e : g_park) {
      if (!e.live || e.dev != dev) continue;
      for (ParkedBlock& b : e.b) {
        if (b.p) { on[n] = e.s; blocks[n++] = b.p; *freed_bytes += b.bytes; }
        if (b.done) (void)hipEventDestroy(b.done);
        b = ParkedBlock();
      }
      e.live = false;
    }
  }
  if (!n) return hipSuccess;
  int cur = 0;
  hipError_t err = hipGetDevice(&cur);
  if (err == hipSuccess) err = hipSetDevice(dev);
  if (err == hipSuccess) err = hipDeviceSynchronize();        // whatever was queued behind a parked slab has run
  { size_t total = 0; if (err == hipSuccess && hipMemGetInfo(free_before, &total) != hipSuccess) { (void)hipGetLastError(); *free_before = 0; *freed_bytes = 0; } }
  // Each slab is freed on the stream it was parked under, as a call used to free it, and the device is synchronised: measured, only
  // then does hipMemPoolTrimTo hand the block back (freed with hipFree, or on the null stream, it stayed in the pool).  A stream that
  // has been destroyed since is refused by the runtime: that slab goes back with hipFree.
  for (int i = 0; i < n; ++i) {
    hipError_t e = hipFreeAsync(blocks[i], on[i]);
    if (e != hipSuccess) { (void)hipGetLastError(); e = hipFree(blocks[i]); }
    if (e != hipSuccess && err == hipSuccess) err = e;
  }
  { const hipError_t e = hipDeviceSynchronize(); if (err == hipSuccess) err = e; }
  (void)hipSetDevice(cur);
  return err;
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_trim_scratch(int32_t device) {
  if (device < 0 || device >= kMaxDevices) return NMOD_ERR_INVALID_ARG;
  hp_trim(device);                                // the pinned ring + streams of the host-resident entry
  size_t parked_bytes = 0, free_before = 0;
  NMOD_HIP(parked_trim(device, &parked_bytes, &free_before));   // the slabs parked per stream go back to the pool first
  std::lock_guard<std::mutex> lock(g_pool_mutex);
  if (g_pool[device]) {
    // A block freed a moment ago (a parked slab) is not always the pool's to release at the first try, even after the device has been
    // synchronised: trim until the pool reserves no more than is in use, a bounded number of times
    for (int tries = 0;; ++tries) {
      NMOD_HIP(hipMemPoolTrimTo(g_pool[device], 0));
      uint64_t reserved = 0, used = 0;
      if (hipMemPoolGetAttribute(g_pool[device], hipMemPoolAttrReservedMemCurrent, &reserved) != hipSuccess ||
          hipMemPoolGetAttribute(g_pool[device], hipMemPoolAttrUsedMemCurrent, &used) != hipSuccess) { (void)hipGetLastError(); break; }
      if (reserved <= used || tries == 200) break;
      std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
  }
  // The runtime hands a block that was freed a moment ago back to the driver shortly AFTER hipMemPoolTrimTo has returned (measured:
  // within a millisecond).  A caller that reads hipMemGetInfo next should see it: wait, for at most a tenth of a second, until the
  // parked bytes show as free
  if (parked_bytes) {
    int cur = 0;
    if (hipGetDevice(&cur) == hipSuccess && hipSetDevice(device) == hipSuccess) {
      for (int tries = 0; tries < 100; ++tries) {
        size_t free_now = 0, total = 0;
        if (hipMemGetInfo(&free_now, &total) != hipSuccess) { (void)hipGetLastError(); break; }
        if (free_now >= free_before + parked_bytes - parked_bytes / 16) break;
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
      }
      (void)hipSetDevice(cur);
    } else (void)hipGetLastError();
  }
  return NMOD_OK;
}
