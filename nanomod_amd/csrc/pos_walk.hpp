// The scaffold that the kernels which walk classed positions share (K8 nmod_mix_fraction, K9 nmod_one_sample, K14 nmod_site_stoich, K15 nmod_site_diff, K18 nmod_pair_linkage).
// One copy of: the work lists per class and the kernel that fills them, the loop heads of the two persistent forms, the lists' share
// of the slab and the launches under their caps of workgroups per CU.  What differs — the rule that classes a position, the arithmetic
// on a row, its outputs — stays with each kernel.  Nothing here multiplies and adds: contraction is the callers' concern.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "entry_common.hpp"
#include "entry_device.hpp"

namespace nmod {

// the positions of each class, in the order the classify kernel's waves appended them; count[c]: the length of list[c]
template <int NC>
struct PosLists { uint32_t* list[NC]; uint32_t* count; };

// A thread per position.  Rule::cls(a, i, begin, n): the class of position i, or -1 after writing its NaN outputs and status; begin, n:
// its row of the per-sample track Rule::track(a) (of Rule::Track; void: the entry has none), which a left-out row gets NaN-filled
// here, a wave per row.  Args: npos and the lists `pl` next to whatever the rule reads.
template <class Rule, class Args>
static __global__ __launch_bounds__(256) void pos_classify_kernel(Args a) {
  const int lane = threadIdx.x & 63;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < a.npos; base += (int64_t)gridDim.x * 256) {
    const int64_t i = base + threadIdx.x;
    const bool in = i < a.npos;
    int cls = -1;
    int64_t begin = 0, n = 0;
    if (in) cls = Rule::cls(a, i, begin, n);
    compact_to_lists<Rule::NC>(cls, lane, a.pl.list, a.pl.count, i);
    if constexpr (!std::is_void<typename Rule::Track>::value) {
      typename Rule::Track* const track = Rule::track(a);
      if (track) {
        unsigned long long mask = __ballot(in && cls < 0);
        while (mask) {
          const int src = __ffsll((long long)mask) - 1;
          mask &= mask - 1ull;
          const int64_t b = __shfl((long long)begin, src), m = __shfl((long long)n, src);
          for (int64_t k = lane; k < m; k += 64) track[b + k] = (typename Rule::Track)nan_f64();   // (as float: 0x7FC00000)
        }
      }
    }
  }
}

// The loop heads of the two persistent forms over list CLS: `for (GroupWalk<CLS, ..> it(a.pl); it.more(); it.next())`, strided over the
// grid.  The register forms: a group of G lanes per position, THREADS / G positions per workgroup.  The body is reached by whole waves:
// a group beyond the end of the list has no position (have() false: pos() is not for it) and computes along.
template <int CLS, int G, int THREADS>
struct GroupWalk {
  const uint32_t* list; int64_t cnt, w0;                    // w0: the item of the workgroup's first group
  template <int NC>
  __device__ __forceinline__ explicit GroupWalk(const PosLists<NC>& pl) : list(pl.list[CLS]), cnt(pl.count[CLS]), w0((int64_t)blockIdx.x * (THREADS / G)) {}
  __device__ __forceinline__ bool more() const { return w0 < cnt; }
  __device__ __forceinline__ void next() { w0 += (int64_t)gridDim.x * (THREADS / G); }
  __device__ __forceinline__ bool have() const { return w0 + threadIdx.x / G < cnt; }
  __device__ __forceinline__ int64_t pos() const { return (int64_t)list[w0 + threadIdx.x / G]; }
};

// The workgroup forms: a workgroup per position
template <int CLS>
struct BlockWalk {
  const uint32_t* list; int64_t cnt, w;
  template <int NC>
  __device__ __forceinline__ explicit BlockWalk(const PosLists<NC>& pl) : list(pl.list[CLS]), cnt(pl.count[CLS]), w(blockIdx.x) {}
  __device__ __forceinline__ bool more() const { return w < cnt; }
  __device__ __forceinline__ void next() { w += gridDim.x; }
  __device__ __forceinline__ int64_t pos() const { return (int64_t)list[w]; }
};

// Host: the lists' share of a call's slab — taken before slab.commit — and, after it, the lists themselves: the pointers, the zeroed
// count words, and the classify launch on the call's stream (a.pl is set here).
template <int NC>
struct PosListSpace {
  size_t o_list, o_count;
  PosListSpace(Slab& slab, size_t npos) : o_list(slab.take(npos * 4 * NC)), o_count(slab.take(16)) {}
  template <class Rule, class Args>
  hipError_t fill(const Slab& slab, Args& a, int num_cus, hipStream_t stream) const {
    static_assert(Rule::NC == NC && NC <= 4, "the count words are 16 bytes");
    for (int c = 0; c < NC; ++c) a.pl.list[c] = slab.at<uint32_t>(o_list) + (size_t)c * (size_t)a.npos;
    a.pl.count = slab.at<uint32_t>(o_count);
    const hipError_t e = hipMemsetAsync(a.pl.count, 0, 16, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((pos_classify_kernel<Rule, Args>), dim3(persistent_grid(a.npos, 256, (int64_t)num_cus * 16)), dim3(256), 0, stream, a);
    return hipSuccess;
  }
};

// a register form (G lanes per position) under 8 workgroups per CU, a workgroup form (G == THREADS) under 2
template <int G, int THREADS, class Args>
static void launch_groups(void (*kernel)(Args), const Args& a, int num_cus, hipStream_t stream) {
  hipLaunchKernelGGL(kernel, dim3(persistent_grid(a.npos, THREADS / G, (int64_t)num_cus * (G < THREADS ? 8 : 2))), dim3(THREADS), 0, stream, a);
}
template <int THREADS, class Args>
static void launch_blocks(void (*kernel)(Args), const Args& a, int num_cus, hipStream_t stream) { launch_groups<THREADS, THREADS>(kernel, a, num_cus, stream); }

}  // namespace nmod
