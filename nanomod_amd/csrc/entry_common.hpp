// The host half that the library's C entry points share: error recording, the checks of nmod_params, device selection with
// the cached CU count, the small size helpers, the dtype dispatcher, the slab of a call with its host-memspace staging, rows_begin and
// launches_end.  (Device-side helpers of K8 .. K14 and the q-values: entry_device.hpp; the walks: pos_walk.hpp, read_walk.hpp.)
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "../../include/nanomod_hip.h"
#include "scratch_pool.hpp"

namespace nmod {

// errors.hip; they only feed nmod_strerror's text: the last HIP error of the thread (NMOD_HIP below sets it), the last RCCL
// error and the library's words for it (comm.hip sets them)
extern thread_local hipError_t g_last_hip;
extern thread_local int g_last_rccl;
extern thread_local const char* g_last_rccl_text;

// return NMOD_ERR_HIP from the calling entry when a hipError_t-valued expression fails, remembering which error it was
#define NMOD_HIP(call)                                   \
  do {                                                   \
    hipError_t e_ = (call);                              \
    if (e_ != hipSuccess) { g_last_hip = e_; return NMOD_ERR_HIP; } \
  } while (0)

constexpr int kMaxDevices = 64;

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// a positive integer from the environment (the host-resident entry's and the down-sampling branch's sizes), else dflt
inline int64_t env_i64(const char* name, int64_t dflt) {
  const char* s = getenv(name);
  if (!s || !*s) return dflt;
  char* e = nullptr;
  const long long v = strtoll(s, &e, 10);
  return (e && *e == '\0' && v > 0) ? (int64_t)v : dflt;
}

// bytes of a sample; 0: not a dtype
inline size_t elem_bytes(int32_t dtype) {
  return dtype == NMOD_DTYPE_F32 ? 4 : dtype == NMOD_DTYPE_I16_MILLI ? 2 : dtype == NMOD_DTYPE_F64 ? 8 : 0;
}

// a host-resident CSR offset array: starts at or above 0 and never decreases
inline bool csr_offsets_ok(const int64_t* off, int64_t npos) {
  if (off[0] < 0) return false;
  for (int64_t i = 0; i < npos; ++i) if (off[i + 1] < off[i]) return false;
  return true;
}

// The checks of nmod_params every entry starts with: the struct itself, the memspace, the dtype.  An entry that never reads
// one of the two fields (the rankings, the q-values) says so and accepts any value there, as it always has.
enum : unsigned { kPrmAnyDtype = 1u, kPrmAnyMemspace = 2u };
inline int check_prm_common(const nmod_params* prm, unsigned any = 0u) {
  if (!prm || prm->struct_size != (int32_t)sizeof(nmod_params)) return NMOD_ERR_INVALID_ARG;
  if (!(any & kPrmAnyMemspace) && prm->memspace != NMOD_MEM_HOST && prm->memspace != NMOD_MEM_DEVICE) return NMOD_ERR_INVALID_ARG;
  if (!(any & kPrmAnyDtype) && !elem_bytes(prm->dtype)) return NMOD_ERR_INVALID_ARG;
  return NMOD_OK;
}

// CU count per device, looked up once (the attribute query is not cheap and this runs every batch); an atomic per device:
// concurrent first calls both query and store the same value
inline hipError_t device_cus(int dev, int* num_cus) {
  static std::atomic<int> cache[kMaxDevices];
  const bool cacheable = dev >= 0 && dev < kMaxDevices;
  int n = cacheable ? cache[dev].load(std::memory_order_relaxed) : 0;
  if (n <= 0) {
    const hipError_t e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    if (cacheable) cache[dev].store(n, std::memory_order_relaxed);
  }
  *num_cus = n;
  return hipSuccess;
}

// Makes prm->device the thread's device; its CU count where the caller wants it (num_cus may be null).  Without such a
// device: NMOD_ERR_NO_DEVICE, and the runtime's sticky error is cleared.
inline int select_device(const nmod_params* prm, int* num_cus) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || prm->device < 0 || prm->device >= ndev) { (void)hipGetLastError(); return NMOD_ERR_NO_DEVICE; }
  NMOD_HIP(hipSetDevice(prm->device));
  if (num_cus) NMOD_HIP(device_cus(prm->device, num_cus));
  return NMOD_OK;
}

// f(std::integral_constant<int, DT>) for the DT of a checked dtype: the one place a run-time dtype picks a template instance
template <class F>
inline auto for_dtype(int32_t dtype, F f) {
  if (dtype == NMOD_DTYPE_F32) return f(std::integral_constant<int, NMOD_DTYPE_F32>{});
  if (dtype == NMOD_DTYPE_I16_MILLI) return f(std::integral_constant<int, NMOD_DTYPE_I16_MILLI>{});
  return f(std::integral_constant<int, NMOD_DTYPE_F64>{});
}

// blocks of a persistent launch: one per `per_block` items of work, at least 1 and at most `cap`
inline unsigned persistent_grid(int64_t work, int64_t per_block, int64_t cap) {
  const int64_t b = (work + per_block - 1) / per_block;
  return (unsigned)(b < 1 ? 1 : (b < cap ? b : cap));
}

// The device slab of one call, planned before it is allocated: every take() reserves a 256-byte-aligned range, commit()
// allocates the sum (a slab of no bytes still allocates something) on the caller's stream, finish() gives it back (a device-memspace
// call parks it for the next call on the stream: scratch_pool.hpp).
// in() / out() stage one argument of a host-memspace call: the range, the copy to (in) or from (out) the device, and the
// repointing of the argument to its device copy are declared by that one statement.  For a device-memspace call, and for
// an argument the caller left null, they do nothing.
struct Slab {
  static constexpr int kMaxStaged = 24;
  struct Staged { void* ref; void* host; size_t at, bytes; bool download; };
  bool host; size_t bytes = 0; int n = 0; bool overflow = false;
  Staged staged[kMaxStaged];
  DevScratch mem;

  explicit Slab(bool host_memspace) : host(host_memspace) { mem.park = !host_memspace; }   // a device call must not wait: scratch_pool.hpp
  size_t take(size_t b) { const size_t o = bytes; bytes += (size_t)align256((int64_t)b); return o; }
  template <class T> T* at(size_t o) const { return reinterpret_cast<T*>(static_cast<char*>(mem.p) + o); }

  // ref: the pointer the kernels will read (in) or write (out) `b` bytes through; `tail`: bytes reserved beyond them
  template <class P> void in(P& ref, size_t b, size_t tail = 0) { stage(&ref, const_cast<void*>(static_cast<const void*>(ref)), b, tail, false); }
  template <class P> void out(P& ref, size_t b) { stage(&ref, static_cast<void*>(ref), b, 0, true); }

  // allocate, enqueue the uploads, repoint every staged argument
  hipError_t commit(hipStream_t s, int dev) {
    if (overflow) return hipErrorInvalidValue;
    hipError_t e = mem.alloc(bytes, s, dev);
    for (int k = 0; k < n && e == hipSuccess; ++k) {
      void* d = at<char>(staged[k].at);
      if (!staged[k].download && staged[k].bytes) e = hipMemcpyAsync(d, staged[k].host, staged[k].bytes, hipMemcpyHostToDevice, s);
      memcpy(staged[k].ref, &d, sizeof(d));
    }
    return e;
  }
  // enqueue the downloads and wait for them (host memspace), release the slab
  hipError_t finish(hipStream_t s) {
    hipError_t e = hipSuccess;
    for (int k = 0; k < n && e == hipSuccess; ++k)
      if (staged[k].download && staged[k].bytes) e = hipMemcpyAsync(staged[k].host, at<char>(staged[k].at), staged[k].bytes, hipMemcpyDeviceToHost, s);
    if (host && e == hipSuccess) e = hipStreamSynchronize(s);
    return e == hipSuccess ? mem.release(s) : e;
  }

 private:
  void stage(void* ref, void* host_ptr, size_t b, size_t tail, bool download) {
    if (!host || !host_ptr) return;
    if (n == kMaxStaged) { overflow = true; return; }
    staged[n++] = Staged{ref, host_ptr, take(b + tail), b, download};
  }
};

// After an entry's own checks: the offsets of a host call, then the device.  NMOD_OK with no rows: there is nothing to do
inline int rows_begin(const nmod_params* prm, int64_t nrows, const int64_t* off, int* num_cus) {
  if (prm->memspace == NMOD_MEM_HOST && off && nrows > 0 && !csr_offsets_ok(off, nrows)) return NMOD_ERR_INVALID_ARG;
  if (nrows == 0) return NMOD_OK;
  return select_device(prm, num_cus);
}
// the end of an entry: what the launches left behind, the downloads of a host call, the slab
inline int launches_end(Slab& slab, hipStream_t stream) {
  NMOD_HIP(hipGetLastError());
  NMOD_HIP(slab.finish(stream));
  return NMOD_OK;
}

}  // namespace nmod
