// The detect unit of the C ABI (include/nanomod_hip.h): argument checking, workspace carving, size-class binning, the float64
// front end and the K1 / K2 / K3 launches of one device-resident batch on the caller's stream — nmod_detect_batch,
// nmod_combine_track, nmod_describe_dispatch, nmod_last_dispatch_stats and the small entries that describe the build.
// What the other units call is declared in detect_internal.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include <string>
#include <stdio.h>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "detect_internal.hpp"
#include "evtimer.hpp"
#include "host_pipeline.hpp"
#include "rank_stats.hpp"
#include "rank_stats_launch.hpp"
#include "item_claim.hpp"
#include "pvalue_kernels.hpp"
#include "big_rank.hpp"
#include "deep_rank.hpp"
#include "rank_all.hpp"
#include "scratch_pool.hpp"

namespace nmod {

// ---------------------------------------------------------------- workspace
struct Workspace {
  uint32_t* ks_num; uint64_t* mwu_s; uint64_t* tie; double* moments;
  double* tmp_ks_d; double* tmp_ks_p; double* ks_d_ref;
  int32_t* order; int32_t* redo; uint8_t* cls; uint8_t* tied; uint8_t* cnt_done; uint8_t* nonfinite; int32_t* meta;
  int32_t* work_list; int32_t* work_meta;      // counting form for any coverage (rank_count_wide.hpp)   // meta: [c] counts, [56 + c] offsets, [112 + c] cursors, [168..169] max n0/n1
  unsigned long long* stats;                                     // nmod_last_dispatch_stats: kStatsWords counters, written only on request
  int64_t bytes;
};
// raw counters of dispatch_stats_kernel: [0] the 256-capacity counting form's gate, [1] positions it produced, [2] float64 redo,
// [kStatsClass + c] positions of launch class c, [kStatsGate + c] the any-coverage counting form's gate of class c (summed over the
// chunks of a host-resident batch), [kStatsLeft + c] positions it left to the class's sorting form
constexpr int kStatsClass = 8, kStatsGate = 64, kStatsLeft = 128, kStatsTried = 192;   // (kStatsWords = 256: detect_internal.hpp)
constexpr int kMetaInts = 320;
constexpr int kMetaMax = 3 * kClassStride;      // [168..169] max n0 / n1
constexpr int kMetaBigTotal = kMetaMax + 2;     // [170..171] u64: scratch floats the large positions need
constexpr int kMetaBigCursor = kMetaMax + 4;    // [172..173] u64: bump allocator of big_rank_kernel
constexpr int kMetaWideRedo = kMetaMax + 8;     // [176] positions on the WIDE form's redo list (wide_redo_kernel)
constexpr int kMetaCntGate = kMetaMax + 10;     // [178] the counting form's gate (cnt_probe_kernel: 1 = the batch is event-like)
constexpr int kMetaDeepTiles = kMetaMax + 12;   // [180..181] u64: tiles of the deep positions (NMOD_FLAG_DEEP, deep_rank.hpp)
constexpr int kMetaRedo = 184;                  // float64 front end: [184] count of positions to redo, [184 + kClassStride] = 0 (their
                                                // offset in the list), [242..243] u64 scratch keys they need, [244..245] u64 bump allocator
constexpr int kMetaRedoTotal = 242, kMetaRedoCursor = 244;
constexpr int kMetaClaim = 256;                 // [256 + c] ticket counter of class c's ks_rank_kernel launch (item_claim.hpp): 0 when it starts
static_assert(kMetaRedoCursor + 2 <= kMetaClaim && kMetaClaim + kClassStride <= kMetaInts, "meta layout: claim counters");
static_assert(kMetaRedo + kClassStride < kMetaRedoTotal && kMetaRedoCursor + 2 <= kMetaInts && kMetaBigCursor + 2 <= kMetaWideRedo && kMetaWideRedo < kMetaCntGate && kMetaCntGate < kMetaDeepTiles && kMetaDeepTiles + 2 <= kMetaRedo, "meta layout");
// (kBigClass, kBigHistClass, kWideBigBase .., kNumPairs: rank_stats_launch.hpp)
static_assert(kNumPairs <= kClassStride && kStatsClass + kClassStride <= kStatsGate && kStatsGate + kClassStride <= kStatsLeft && kStatsLeft + kClassStride <= kStatsTried && kStatsTried + kClassStride <= kStatsWords, "class tables");

static Workspace carve(void* base, int64_t npos) {
  Workspace w;
  char* p = (char*)base;
  int64_t o = 0;
  auto take = [&](int64_t bytes) { char* r = p ? p + o : nullptr; o += align256(bytes); return r; };
  w.ks_num = (uint32_t*)take(4 * npos);
  w.mwu_s = (uint64_t*)take(8 * npos);
  w.tie = (uint64_t*)take(8 * npos);
  w.moments = (double*)take(32 * npos);
  w.tmp_ks_d = (double*)take(8 * npos);
  w.tmp_ks_p = (double*)take(8 * npos);
  w.ks_d_ref = (double*)take(8 * npos);
  w.order = (int32_t*)take(4 * npos);
  w.redo = (int32_t*)take(4 * npos);
  w.cls = (uint8_t*)take(npos);
  w.tied = (uint8_t*)take(npos);
  w.cnt_done = (uint8_t*)take(npos + 16);        // counting form (rank_count.hpp): one flag byte per entry of the work list, dword per item
  w.nonfinite = (uint8_t*)take(npos);             // NMOD_FLAG_CHECK_FINITE: nonfinite_scan_kernel's flags
  w.meta = (int32_t*)take(kMetaInts * 4);
  w.work_list = (int32_t*)take(4 * npos);          // rank_count_wide.hpp: what the sorting forms still have to do, per class
  w.work_meta = (int32_t*)take(kMetaInts * 4);      // [c] counts, [kClassStride + c] offsets, [2 kClassStride + c] the probes' gates, [3 kClassStride ...] the classes tried
  static_assert(3 * kClassStride + 1 + kClassStride <= kMetaInts, "work_meta: counts, offsets, gates, 1 + one class id per probe block");
  w.stats = (unsigned long long*)take(kStatsWords * 8);
  w.bytes = o;
  return w;
}

// ---------------------------------------------------------------- binning kernels
struct BinArgs {
  int64_t npos; const int64_t* off0; const int64_t* off1; int64_t stride0, stride1;
  ClassRule rule; uint8_t* cls; int32_t* meta; int32_t* order;
};


__global__ __launch_bounds__(256) void max_n_kernel(int64_t npos, const int64_t* off0, const int64_t* off1, int32_t* meta) {
  __shared__ int m0s, m1s;
  if (threadIdx.x == 0) { m0s = 0; m1s = 0; }
  __syncthreads();
  int m0 = 0, m1 = 0;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npos; p += (int64_t)gridDim.x * 256) {
    if (off0) m0 = max(m0, (int)min((int64_t)INT32_MAX, off0[p + 1] - off0[p]));
    if (off1) m1 = max(m1, (int)min((int64_t)INT32_MAX, off1[p + 1] - off1[p]));
  }
  atomicMax(&m0s, m0); atomicMax(&m1s, m1);
  __syncthreads();
  if (threadIdx.x == 0) { atomicMax(&meta[kMetaMax], m0s); atomicMax(&meta[kMetaMax + 1], m1s); }
}

__global__ __launch_bounds__(256) void classify_kernel(BinArgs a) {
  __shared__ int hist[kNumPairs];
  for (int i = threadIdx.x; i < kNumPairs; i += 256) hist[i] = 0;
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.npos; p += (int64_t)gridDim.x * 256) {
    int64_t n0 = a.stride0 > 0 ? a.stride0 : a.off0[p + 1] - a.off0[p];
    int64_t n1 = a.stride1 > 0 ? a.stride1 : a.off1[p + 1] - a.off1[p];
    const int cid = classify_position(n0, n1, a.rule);     // (255: beyond what the caller promised or the format allows, TOO_LARGE)
    if (cid == kBigClass)
      atomicAdd(reinterpret_cast<unsigned long long*>(a.meta + kMetaBigTotal),
                (unsigned long long)(big_pow2_ceil(n0) + big_pow2_ceil(n1)));
    if (cid == kDeepClass)
      atomicAdd(reinterpret_cast<unsigned long long*>(a.meta + kMetaDeepTiles), (unsigned long long)(deep_tiles(n0) + deep_tiles(n1)));
    a.cls[p] = (uint8_t)cid;
    if (cid != 255) atomicAdd(&hist[cid], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kNumPairs; i += 256) if (hist[i]) atomicAdd(&a.meta[i], hist[i]);
}

__global__ void class_offsets_kernel(int32_t* meta) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    int acc = 0;
    for (int i = 0; i < kNumPairs; ++i) { meta[kClassStride + i] = acc; meta[2 * kClassStride + i] = 0; acc += meta[i]; }
  }
}

// Every block owns kScatterSpan consecutive positions: it counts their classes, reserves its slots in every class
// list with ONE atomic per class present (all chunks hammering one counter was the whole cost of this kernel:
// 0.21 ms for 4.6 M positions of one class), and writes its positions in order.  Each wave walks the DISTINCT
// classes it holds: one ballot per class present (1-3 for real coverage), not one per class that exists.
constexpr int kScatterSpan = 16 * 256;

__global__ __launch_bounds__(256) void scatter_kernel(BinArgs a) {
  __shared__ int wave_cnt[4][kNumPairs];
  __shared__ int run[kNumPairs];                 // next free slot of this block in every class list
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t span0 = (int64_t)blockIdx.x * kScatterSpan;
  const int64_t span1 = span0 + kScatterSpan < a.npos ? span0 + kScatterSpan : a.npos;
  // pass 1: class counts of the span
  for (int i = threadIdx.x; i < kNumPairs; i += 256) run[i] = 0;
  __syncthreads();
  for (int64_t p0 = span0; p0 < span1; p0 += 256) {
    const int64_t p = p0 + threadIdx.x;
    const int cid = (p < span1) ? a.cls[p] : 255;
    unsigned long long todo = __ballot(cid != 255);
    while (todo != 0ull) {
      const int c = __builtin_amdgcn_readlane(cid, __ffsll((long long)todo) - 1);
      const unsigned long long same = __ballot(cid == c);
      if (lane == 0) atomicAdd(&run[c], __popcll(same));
      todo &= ~same;
    }
  }
  __syncthreads();
  if (threadIdx.x < kNumPairs) {
    const int c = threadIdx.x;
    const int tot = run[c];
    run[c] = a.meta[kClassStride + c] + (tot ? atomicAdd(&a.meta[2 * kClassStride + c], tot) : 0);
  }
  __syncthreads();
  // pass 2: the same walk, now writing; positions of a class keep their order inside the span
  for (int64_t p0 = span0; p0 < span1; p0 += 256) {
    const int64_t p = p0 + threadIdx.x;
    const int cid = (p < span1) ? a.cls[p] : 255;
    for (int i = threadIdx.x; i < 4 * kNumPairs; i += 256) (&wave_cnt[0][0])[i] = 0;
    __syncthreads();
    int rank = 0;
    unsigned long long todo = __ballot(cid != 255);
    while (todo != 0ull) {
      const int c = __builtin_amdgcn_readlane(cid, __ffsll((long long)todo) - 1);
      const unsigned long long same = __ballot(cid == c);
      if (cid == c) rank = __popcll(same & ((1ull << lane) - 1ull));
      if (lane == 0) wave_cnt[wave][c] = __popcll(same);
      todo &= ~same;
    }
    __syncthreads();
    if (cid != 255) {
      for (int w = 0; w < wave; ++w) rank += wave_cnt[w][cid];
      a.order[run[cid] + rank] = (int32_t)p;
    }
    __syncthreads();
    if (threadIdx.x < kNumPairs) {
      const int c = threadIdx.x;
      run[c] += wave_cnt[0][c] + wave_cnt[1][c] + wave_cnt[2][c] + wave_cnt[3][c];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- float64 input (NMOD_DTYPE_F64)
// The reference holds its samples as float64 (myDetect.py:124).  All the rank statistics depend on the ORDER of a
// position's samples only, so every position gets float32 keys that preserve its order and its ties:
//   class 1  every sample of the position is float32-exact                      key = (float)x         (exact)
//   class 2  every sample is k / 1000.0 with |k| <= 2^24 (NanoMod's 3-dp Events)  key = (float)k         (exact)
//   class 3  anything else                                                       key = (float)x, rounded to nearest
// Rounding is monotone (x <= y => key(x) <= key(y)) and keeps ties, so in class 3 the only possible damage is a FALSE
// tie between two different samples.  K1 reports the positions in which keys tie (RankStatsArgs::tied); those among
// the class-3 positions — rare for real-valued signals — are redone by big_rank_kernel<2> on the float64 samples
// themselves.  The Welch moments never come from the keys: f64_moments_kernel takes them from the samples.
struct F64Args {
  const double* d0; const double* d1;          // the caller's samples (index space of the offsets)
  const int64_t* off0; const int64_t* off1; int64_t stride0, stride1;
  int64_t npos;
  float* k0; float* k1;                        // keys, same index space
  uint8_t* cls3;                               // [npos] 1 = class 3
  const uint8_t* tied; const uint8_t* cls;     // K1's tie flags; the size-class byte of the binning (null: no binning ran)
  int32_t* order; int32_t* meta;               // redo list (ws.order) and its counters (ws.meta + kMetaRedo ...)
  double* moments;
  int32_t deep;                                // NMOD_FLAG_DEEP: positions with a group beyond NMOD_MAX_RANKED belong to deep_rank.hpp (fp64 keys, own moments)
};

__device__ __forceinline__ void f64_rows(const F64Args& a, int64_t p, int64_t& o0, int& n0, int64_t& o1, int& n1) {
  if (a.stride0 > 0) { o0 = p * a.stride0; n0 = (int)a.stride0; } else { o0 = a.off0[p]; n0 = (int)(a.off0[p + 1] - o0); }
  if (a.stride1 > 0) { o1 = p * a.stride1; n1 = (int)a.stride1; } else { o1 = a.off1[p]; n1 = (int)(a.off1[p + 1] - o1); }
}

// one wave per position: classify (first sweep), write the keys (second sweep: the samples come from L2)
__global__ __launch_bounds__(256) void f64_encode_kernel(F64Args a) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), ws = (int64_t)gridDim.x * 4;
  for (int64_t p = w0; p < a.npos; p += ws) {
    int64_t o0, o1; int n0, n1;
    f64_rows(a, p, o0, n0, o1, n1);
    bool f32_ok = true, grid_ok = true;
    for (int g = 0; g < 2; ++g) {
      const double* src = (g ? a.d1 + o1 : a.d0 + o0);
      const int n = g ? n1 : n0;
      for (int i = lane; i < n; i += 64) {
        const double v = src[i];
        f32_ok = f32_ok && ((double)(float)v == v);
        const double k = rint(v * 1000.0);
        grid_ok = grid_ok && (fabs(k) <= 16777216.0) && (k / 1000.0 == v);
      }
    }
    const bool all_f32 = __ballot(!f32_ok) == 0ull;
    const bool all_grid = __ballot(!grid_ok) == 0ull;
    const bool scale = !all_f32 && all_grid;
    for (int g = 0; g < 2; ++g) {
      const double* src = (g ? a.d1 + o1 : a.d0 + o0);
      float* dst = (g ? a.k1 + o1 : a.k0 + o0);
      const int n = g ? n1 : n0;
      for (int i = lane; i < n; i += 64) {
        const double v = src[i];
        dst[i] = scale ? (float)rint(v * 1000.0) : (float)v;
      }
    }
    if (lane == 0) a.cls3[p] = (!all_f32 && !all_grid) ? 1 : 0;
  }
}

// mean and sum of squared deviations of both groups from the float64 samples, two-pass like np.mean / np.var
__global__ __launch_bounds__(256) void f64_moments_kernel(F64Args a) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), ws = (int64_t)gridDim.x * 4;
  for (int64_t p = w0; p < a.npos; p += ws) {
    int64_t o0, o1; int n0, n1;
    f64_rows(a, p, o0, n0, o1, n1);
    if (a.deep && (n0 > NMOD_MAX_RANKED || n1 > NMOD_MAX_RANKED)) continue;
    for (int g = 0; g < 2; ++g) {
      const double* src = (g ? a.d1 + o1 : a.d0 + o0);
      const int n = g ? n1 : n0;
      double s = 0.0;
      for (int i = lane; i < n; i += 64) s += src[i];
      s = wave_sum_f64(s);
      const double mu = s / (double)n;
      double q = 0.0;
      for (int i = lane; i < n; i += 64) { const double d = src[i] - mu; q += d * d; }
      q = wave_sum_f64(q);
      if (lane == 0) { double* mo = a.moments + p * 4 + 2 * g; mo[0] = mu; mo[1] = q; }
    }
  }
}

// the class-3 positions whose keys tied (or that went to the large-position pass, which reports no ties) -> redo list
__global__ __launch_bounds__(256) void f64_redo_list_kernel(F64Args a) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < a.npos; p += (int64_t)gridDim.x * 256) {
    if (!a.cls3[p]) continue;
    const bool big = a.cls && (a.cls[p] == (uint8_t)kBigClass || a.cls[p] == (uint8_t)kBigHistClass);
    const bool skipped = a.cls && (a.cls[p] == 255 || a.cls[p] == (uint8_t)kDeepClass);
    if (skipped || !(a.tied[p] || big)) continue;
    int64_t o0, o1; int n0, n1;
    f64_rows(a, p, o0, n0, o1, n1);
    const int idx = atomicAdd(&a.meta[kMetaRedo], 1);
    a.order[idx] = (int32_t)p;
    atomicAdd(reinterpret_cast<unsigned long long*>(a.meta + kMetaRedoTotal), (unsigned long long)(big_pow2_ceil(n0) + big_pow2_ceil(n1)));
  }
}


// ---------------------------------------------------------------- dispatch statistics (nmod_last_dispatch_stats; StatsArgs: detect_internal.hpp)
__global__ __launch_bounds__(256) void dispatch_stats_kernel(StatsArgs a) {
  const int c256 = kNumGeneralClasses + 2;
  auto count_of = [&](int c) -> int64_t { return a.uniform_cls >= 0 ? (c == a.uniform_cls ? a.npos : 0) : (int64_t)a.meta[c]; };
  if (blockIdx.x == 0) {
    const int c = threadIdx.x;
    if (c < kNumPairs) {
      const int64_t n = count_of(c);
      if (n) atomicAdd(&a.acc[kStatsClass + c], (unsigned long long)n);
      if (a.cw_ran && n && a.gates[c] != 0) {
        atomicAdd(&a.acc[kStatsGate + c], 1ull);
        atomicAdd(&a.acc[kStatsTried + c], (unsigned long long)n);
        atomicAdd(&a.acc[kStatsLeft + c], (unsigned long long)a.work_meta[c]);
      }
    }
    if (c == 64 && a.cnt256_ran && a.meta[kMetaCntGate] != 0 && count_of(c256) > 0) { atomicAdd(&a.acc[0], 1ull); atomicAdd(&a.acc[kStatsTried + c256], (unsigned long long)count_of(c256)); }
    if (c == 65 && a.f64) atomicAdd(&a.acc[2], (unsigned long long)a.meta[kMetaRedo]);
  }
  if (a.cnt256_ran && a.meta[kMetaCntGate] != 0) {        // entries of the class list whose flag byte says "produced by rank_count_kernel"
    const int64_t n = count_of(c256);
    unsigned mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) mine += a.cnt_done[i] != 0 ? 1u : 0u;
    mine = (unsigned)wave_sum_u64((unsigned long long)mine);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&a.acc[1], (unsigned long long)mine);
  }
}
// the last successful nmod_detect_batch of the thread (written there and nowhere else)
struct DispatchRec {
  bool valid = false; bool host = false; int device = 0; hipStream_t stream = nullptr;
  StatsArgs args = {};                                // (acc = the workspace's own block for a device-resident batch)
  unsigned long long host_totals[kStatsWords] = {};   // a host-resident (or empty) batch: read back before the call returned
  int64_t npos = 0;
};
thread_local DispatchRec g_dispatch;
hipError_t enqueue_dispatch_stats(const StatsArgs& a, hipStream_t stream) {
  const unsigned blocks = a.cnt256_ran ? (unsigned)std::max<int64_t>(1, std::min<int64_t>((a.npos + 255) / 256, 512)) : 1u;
  hipLaunchKernelGGL(dispatch_stats_kernel, dim3(blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------- helpers
int check_params(const nmod_params* prm) {
  if (!prm || prm->struct_size != (int32_t)sizeof(nmod_params)) return NMOD_ERR_INVALID_ARG;
  if (prm->dtype != NMOD_DTYPE_F32 && prm->dtype != NMOD_DTYPE_I16_MILLI && prm->dtype != NMOD_DTYPE_F64) return NMOD_ERR_INVALID_ARG;
  if (prm->memspace != NMOD_MEM_HOST && prm->memspace != NMOD_MEM_DEVICE) return NMOD_ERR_INVALID_ARG;
  if (prm->method < NMOD_METHOD_KS || prm->method > NMOD_METHOD_FISHER) return NMOD_ERR_INVALID_ARG;
  if (prm->nb < 0 || prm->nb > NMOD_MAX_NB) return NMOD_ERR_INVALID_ARG;
  if ((prm->tests & ~NMOD_TEST_ALL) != 0) return NMOD_ERR_INVALID_ARG;
  if ((prm->flags & ~(NMOD_FLAG_KS_RATIONAL_D | NMOD_FLAG_CHECK_FINITE | NMOD_FLAG_NO_COUNTING | NMOD_FLAG_NO_COUNT_WIDE | NMOD_FLAG_NO_HOST_NARROW | NMOD_FLAG_DEEP | NMOD_FLAG_K1_STATIC_ITEMS)) != 0 || prm->reserved != 0) return NMOD_ERR_INVALID_ARG;
  return NMOD_OK;
}

static int fill_combine_args(const nmod_params* prm, CombineArgs& ca) {
  ca.nb = prm->nb; ca.method = prm->method;
  double dif = prm->weights_dif;
  if (prm->method == NMOD_METHOD_STOUFFER && !(dif > 0.0)) return NMOD_ERR_INVALID_ARG;
  // myDetect.py:396-400: 100 in the middle, each step outwards divides by WeightsDif
  int nb = prm->nb;
  ca.w[nb] = 100.0;
  for (int k = 1; k <= nb; ++k) { ca.w[nb - k] = ca.w[nb - k + 1] / dif; ca.w[nb + k] = ca.w[nb + k - 1] / dif; }
  double ss = 0.0;
  for (int k = 0; k <= 2 * nb; ++k) ss += ca.w[k] * ca.w[k];
  ca.wnorm = sqrt(ss);
  return NMOD_OK;
}

int launch_combine(const nmod_params* prm, hipStream_t stream, int64_t npos, const double* ks_d,
                   const double* ks_p, const int32_t* run_id, double* comb_st, double* comb_p) {
  CombineArgs ca;
  memset(&ca, 0, sizeof(ca));
  int rc = fill_combine_args(prm, ca);
  if (rc != NMOD_OK) return rc;
  ca.npos = npos; ca.ks_d = ks_d; ca.ks_p = ks_p; ca.run_id = run_id; ca.comb_st = comb_st; ca.comb_p = comb_p;
  unsigned blocks = (unsigned)((npos + kCombineTile - 1) / kCombineTile);
  if (blocks == 0) return NMOD_OK;
  ScopedKernelTimer tm(prm->timer, NMOD_KERNEL_COMBINE, stream);
  hipLaunchKernelGGL(combine_kernel, dim3(blocks), dim3(kCombineTile), 0, stream, ca);
  NMOD_HIP(hipGetLastError());
  return NMOD_OK;
}

// ---------------------------------------------------------------- the deep form (NMOD_FLAG_DEEP, deep_rank.hpp)
// Enqueues K1 of the ndeep positions of class kDeepClass (`tiles` tiles in all, from the classifier) on `stream`: the tile
// table, then round by round the tile sort, the moments, the merge passes and the ranking.  Leaves `da` describing the slab
// (in `scratch`) for deep_finalize_kernel; no host round trip of its own.
template <int DT>
static int enqueue_deep_rounds(DeepArgs& da, int64_t round_tiles, int64_t max_group, bool all, int num_cus, hipStream_t stream,
                               void* keys_a, void* keys_b) {
  typedef typename BigKey<DT>::type K;
  const size_t tile_lds = (size_t)kDeepTile * sizeof(K);
  NMOD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(deep_tile_kernel<DT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds));
  int passes = 0;
  for (int64_t w = kDeepTile; w < deep_tiles(max_group) * kDeepTile; w <<= 1) ++passes;     // the longest group's runs -> one
  const unsigned tb = (unsigned)std::min<int64_t>(round_tiles, (int64_t)num_cus * 8);
  const unsigned mb = (unsigned)std::min<int64_t>(round_tiles * (kDeepTile / kDeepChunk), (int64_t)num_cus * 16);
  const unsigned pb = (unsigned)std::min<int64_t>(da.ndeep, (int64_t)num_cus * 4);
  for (int r = 0; r < da.nrounds; ++r) {
    da.round = r;
    da.src = nullptr; da.dst = keys_a;
    hipLaunchKernelGGL(deep_tile_kernel<DT>, dim3(tb), dim3(kDeepThreads), tile_lds, stream, da);
    if (all) {
      hipLaunchKernelGGL(deep_mean_kernel, dim3(pb), dim3(kDeepThreads), 0, stream, da);
      da.src = keys_a;
      hipLaunchKernelGGL(deep_q_kernel<DT>, dim3(tb), dim3(kDeepThreads), 0, stream, da);
    }
    void* bufs[2] = {keys_a, keys_b};
    for (int p = 0; p < passes; ++p) {
      da.src = bufs[p & 1]; da.dst = bufs[(p + 1) & 1]; da.width = (int64_t)kDeepTile << p;
      hipLaunchKernelGGL(deep_merge_kernel<DT>, dim3(mb), dim3(kDeepThreads), 0, stream, da);
    }
    da.src = bufs[passes & 1]; da.dst = nullptr;
    hipLaunchKernelGGL(deep_rank_kernel<DT>, dim3(tb), dim3(kDeepThreads), 0, stream, da);
    NMOD_HIP(hipGetLastError());
  }
  da.src = nullptr; da.dst = nullptr;
  return NMOD_OK;
}

static int enqueue_deep(const nmod_params* prm, DeepArgs& da, DevScratch& scratch, int dtype, const void* sig0, const void* sig1,
                        const int64_t* off0, const int64_t* off1, int64_t stride0, int64_t stride1, const Workspace& ws,
                        int64_t ndeep, int64_t tiles, int64_t max_group, bool all, int num_cus, hipStream_t stream) {
  if (ndeep <= 0 || tiles < 2 * ndeep) return NMOD_ERR_INVALID_ARG;
  const int64_t nrounds = (tiles + kDeepRoundStride - 1) / kDeepRoundStride;
  const int64_t round_tiles = std::min<int64_t>(tiles, kDeepRoundTiles);
  const int64_t ksz = dtype == NMOD_DTYPE_F64 ? 8 : 4;
  int64_t o = 0;
  auto take = [&](int64_t bytes) { const int64_t r = o; o += align256(bytes); return r; };
  const int64_t o_ptile = take((ndeep + 1) * 8), o_round = take((nrounds + 1) * 8), o_acc = take(ndeep * (int64_t)sizeof(DeepAcc));
  const int64_t o_sum = take(tiles * 8), o_q = take(tiles * 8);
  const int64_t o_ka = take(round_tiles * kDeepTile * ksz), o_kb = take(round_tiles * kDeepTile * ksz);
  NMOD_HIP(scratch.alloc((size_t)o, stream, prm->device));
  char* base = (char*)scratch.p;
  NMOD_HIP(hipMemsetAsync(base + o_acc, 0, (size_t)ndeep * sizeof(DeepAcc), stream));
  da.sig0 = sig0; da.sig1 = sig1; da.off0 = off0; da.off1 = off1; da.stride0 = stride0; da.stride1 = stride1;
  da.pos_list = ws.order; da.class_meta = ws.meta; da.deep_class = kDeepClass;
  da.ndeep = ndeep; da.nrounds = (int32_t)nrounds;
  da.ptile = (int64_t*)(base + o_ptile); da.roundtab = (int64_t*)(base + o_round); da.acc = (DeepAcc*)(base + o_acc);
  da.tile_sum = (double*)(base + o_sum); da.tile_q = (double*)(base + o_q); da.all = all ? 1 : 0;
  hipLaunchKernelGGL(deep_plan_kernel, dim3(1), dim3(kDeepPlanThreads), 0, stream, da);
  NMOD_HIP(hipGetLastError());
  ScopedKernelTimer tm(prm->timer, NMOD_KERNEL_RANK_STATS, stream);
  if (dtype == NMOD_DTYPE_F64) return enqueue_deep_rounds<2>(da, round_tiles, max_group, all, num_cus, stream, base + o_ka, base + o_kb);
  if (dtype == NMOD_DTYPE_I16_MILLI) return enqueue_deep_rounds<1>(da, round_tiles, max_group, all, num_cus, stream, base + o_ka, base + o_kb);
  return enqueue_deep_rounds<0>(da, round_tiles, max_group, all, num_cus, stream, base + o_ka, base + o_kb);
}

// the float64 samples behind float32 keys (detect_f64): device pointers in the index space of the offsets
struct F64Src { const double* d0; const double* d1; uint8_t* cls3; };

// ---------------------------------------------------------------- one device-resident batch, stage by stage (detect_device)
// plan_batch decides what runs; enqueue_bins, enqueue_k1, enqueue_large, enqueue_f64_fixups and enqueue_outputs put it on the
// stream in that order.  Each stage reads and extends this record.
struct Batch {
  const nmod_params* prm; hipStream_t stream; int num_cus;
  int64_t npos; const void* sig0; const void* sig1; const int64_t* off0; const int64_t* off1;
  int64_t stride0, stride1;                    // (0: the group's offsets)
  const int32_t* run_id; nmod_out* out; const F64Src* f64; Workspace ws;
  // plan_batch
  int tests; bool all, want_comb, deep_flag, binned, big_possible, deep_possible, cw_on, wide_redo;
  int deep_dtype;                              // (float64 samples: the deep form sorts them as 64-bit keys)
  int64_t max0, max1;                          // the limits K1 covers: the promised or measured maxima, capped
  ClassRule rule;
  int uniform_cls;                             // an unbinned batch: the one class of all its positions
  bool wanted[kNumClasses];                    // the class lists K1 launches (and, with big_possible in all-tests mode, the WIDE large classes)
  // enqueue_k1 on
  RankStatsArgs ra;
  bool cw_ran;                                 // the counting form for any coverage was tried on some class
  DeepArgs da; DevScratch deep_scratch;        // the deep form's state between K1 and its finalize
};

// The maxima (their one host round trip when the caller promised none), the test mode, unbinned or binned, whether large or deep
// positions can exist, the counting forms on or off, the classes K1 launches; the workspace's counters are cleared here.
static int plan_batch(Batch& b) {
  const nmod_params* prm = b.prm;
  hipStream_t stream = b.stream;
  const Workspace& ws = b.ws;
  b.tests = prm->tests | (b.want_comb ? NMOD_TEST_KS : 0);
  b.all = (b.tests & (NMOD_TEST_MWU | NMOD_TEST_WELCH)) != 0 || prm->want_mstd;
  const bool uniform = prm->stride0 > 0 && prm->stride1 > 0;
  b.max0 = prm->stride0 > 0 ? prm->stride0 : prm->max_n0;
  b.max1 = prm->stride1 > 0 ? prm->stride1 : prm->max_n1;
  // the class counters / cursors / maxima in ws.meta: cleared once per batch, and not at all for a fixed-stride batch of
  // wave-resident positions (one launch, no lists: the common benchmark shape pays no memset per step)
  bool meta_cleared = false;
  if (b.max0 <= 0 || b.max1 <= 0) {
    NMOD_HIP(hipMemsetAsync(ws.meta, 0, kMetaInts * 4, stream));
    meta_cleared = true;
    hipLaunchKernelGGL(max_n_kernel, dim3(1024), dim3(256), 0, stream, b.npos,
                       prm->stride0 > 0 ? nullptr : b.off0, prm->stride1 > 0 ? nullptr : b.off1, ws.meta);
    NMOD_HIP(hipGetLastError());
    int32_t mx[2];
    NMOD_HIP(hipMemcpyAsync(mx, ws.meta + kMetaMax, 8, hipMemcpyDeviceToHost, stream));
    NMOD_HIP(hipStreamSynchronize(stream));
    if (b.max0 <= 0) b.max0 = mx[0];
    if (b.max1 <= 0) b.max1 = mx[1];
  }
  // a group beyond NMOD_MAX_RANKED: that position is skipped by the classifier and flagged NMOD_STATUS_TOO_LARGE by K2, the rest
  // of the batch is computed (the reference has no limit: myDetect.py:327-343) — unless NMOD_FLAG_DEEP sends it to the deep form
  // (deep_rank.hpp), which takes groups up to NMOD_MAX_DEEP
  b.deep_flag = (prm->flags & NMOD_FLAG_DEEP) != 0;
  const int64_t group_cap = b.deep_flag ? NMOD_MAX_DEEP : NMOD_MAX_RANKED;
  b.max0 = std::min<int64_t>(b.max0, group_cap); b.max1 = std::min<int64_t>(b.max1, group_cap);
  b.deep_possible = b.deep_flag && std::max(b.max0, b.max1) > NMOD_MAX_RANKED;
  b.deep_dtype = b.f64 ? NMOD_DTYPE_F64 : prm->dtype;
  int cmax0 = size_class_of(std::max<int64_t>(b.max0, 1)), cmax1 = size_class_of(std::max<int64_t>(b.max1, 1));
  // positions beyond the wave-resident kernels (both groups sorted in all-tests mode, the smaller one in KS-only
  // mode) go to big_rank_kernel; the maxima tell whether any can exist
  b.big_possible = b.all ? (cmax0 >= kNumSizeClasses || cmax1 >= kNumSizeClasses) : (std::min(cmax0, cmax1) >= kNumSizeClasses);
  cmax0 = std::min(cmax0, kNumSizeClasses - 1); cmax1 = std::min(cmax1, kNumSizeClasses - 1);
  b.binned = !(uniform && !b.big_possible && !b.deep_possible);
  if (!meta_cleared && (b.binned || b.f64)) {
    NMOD_HIP(hipMemsetAsync(ws.meta, 0, kMetaInts * 4, stream));
    meta_cleared = true;
  }
  b.rule.lim0 = std::max<int64_t>(b.max0, 1); b.rule.lim1 = std::max<int64_t>(b.max1, 1);
  b.rule.ks_only = b.all ? 0 : 1; b.rule.deep = b.deep_flag ? 1 : 0;
  b.uniform_cls = -1;
  if (!b.binned) {
    b.uniform_cls = classify_position(b.max0, b.max1, b.rule);
    if (b.uniform_cls != 255) b.wanted[b.uniform_cls] = true;
  } else {
    for (int c0 = 0; c0 <= cmax0; ++c0)
      for (int c1 = 0; c1 <= cmax1; ++c1) b.wanted[small_class_of(c0, c1, !b.all)] = true;
  }
  // all tests, classes other than the 256-capacity one: the counting form for any coverage (rank_count_wide.hpp) is tried per class
  // when its probe finds the class event-like; the sorting form of the class then runs over the work list that is left
  // (NMOD_FLAG_NO_COUNT_WIDE turns it off; KS-only batches too — the form without the tie term and the moments — when a group of
  // the batch can reach the size it takes)
  const bool counting_off = (prm->flags & NMOD_FLAG_NO_COUNTING) != 0, cw_off = (prm->flags & NMOD_FLAG_NO_COUNT_WIDE) != 0;
  b.cw_on = !counting_off && !cw_off && (b.all || std::max(b.max0, b.max1) >= kCwKsMinQ);
  // the WIDE float32 form may put positions on its redo list: wide_redo_kernel finishes them (count read on the device)
  const bool wide_f32 = b.all && prm->dtype == NMOD_DTYPE_F32;
  b.wide_redo = wide_f32 && b.big_possible;
  for (int cls = 0; cls < kNumClasses; ++cls) b.wide_redo = b.wide_redo || (wide_f32 && b.wanted[cls] && wide_class(cls));
  if (b.wide_redo && !meta_cleared) NMOD_HIP(hipMemsetAsync(ws.meta + kMetaWideRedo, 0, 4, stream));   // (the redo counter alone)
  // KS-only: ks_rank_kernel draws tickets from its class's counter unless the call asks for the strided walk (the counters alone)
  if (!b.all && !meta_cleared && !(prm->flags & NMOD_FLAG_K1_STATIC_ITEMS)) NMOD_HIP(hipMemsetAsync(ws.meta + kMetaClaim, 0, kClassStride * 4, stream));
  return NMOD_OK;
}

// binned batches: every position's class (and the large positions' scratch), then the class lists in ws.order
static int enqueue_bins(Batch& b) {
  BinArgs ba;
  ba.npos = b.npos; ba.off0 = b.off0; ba.off1 = b.off1; ba.stride0 = b.stride0; ba.stride1 = b.stride1;
  ba.rule = b.rule; ba.cls = b.ws.cls; ba.meta = b.ws.meta; ba.order = b.ws.order;
  const unsigned blocks = (unsigned)std::min<int64_t>((b.npos + 255) / 256, 4096);
  hipLaunchKernelGGL(classify_kernel, dim3(blocks), dim3(256), 0, b.stream, ba);
  hipLaunchKernelGGL(class_offsets_kernel, dim3(1), dim3(64), 0, b.stream, b.ws.meta);
  hipLaunchKernelGGL(scatter_kernel, dim3((unsigned)((b.npos + kScatterSpan - 1) / kScatterSpan)), dim3(256), 0, b.stream, ba);
  NMOD_HIP(hipGetLastError());
  return NMOD_OK;
}

// K1 of the wave-resident classes: the counting forms for any coverage (probe, then one run over every class), each class's
// sorting form, the WIDE classes of large positions, the WIDE float32 form's redo
static int enqueue_k1(Batch& b) {
  const nmod_params* prm = b.prm;
  const Workspace& ws = b.ws;
  RankStatsArgs& ra = b.ra;
  memset(&ra, 0, sizeof(ra));
  ra.sig0 = b.sig0; ra.sig1 = b.sig1; ra.off0 = b.off0; ra.off1 = b.off1; ra.stride0 = b.stride0; ra.stride1 = b.stride1;
  ra.npos = b.npos; ra.ks_num = ws.ks_num; ra.mwu_s = ws.mwu_s; ra.tie = ws.tie; ra.moments = ws.moments; ra.ks_d_ref = ws.ks_d_ref;
  ra.ks_rational_d = (!b.all && (prm->flags & NMOD_FLAG_KS_RATIONAL_D)) ? 1 : 0;
  ra.tied = b.f64 ? ws.tied : nullptr;          // float32 keys of float64 samples: K1 reports the positions whose keys tie
  ra.redo_list = ws.redo; ra.redo_count = ws.meta + kMetaWideRedo;
  ra.claim = reinterpret_cast<uint32_t*>(ws.meta + kMetaClaim); ra.strided_items = (prm->flags & NMOD_FLAG_K1_STATIC_ITEMS) ? 1 : 0;
  if (b.binned) { ra.pos_list = ws.order; ra.class_meta = ws.meta; }
  // all tests on capacity-256 positions: the counting form is tried first (rank_count.hpp; a device-side probe decides whether
  // the batch is event-like, positions it cannot take fall through to rank_hist_kernel).  The float32 images of float64 samples
  // qualify where they are whole numbers (positions on the 0.001 grid carry k as keys).  NMOD_FLAG_NO_COUNTING turns it off (A/B, parity tests).
  if (b.all && !(prm->flags & NMOD_FLAG_NO_COUNTING)) { ra.cnt_gate = ws.meta + kMetaCntGate; ra.cnt_done = ws.cnt_done; }
  const K1Launcher& k1 = k1_launcher(prm->dtype, b.all);
  CountWideWs cww;
  cww.gates = ws.work_meta + 2 * kClassStride; cww.work_list = ws.work_list; cww.work_meta = ws.work_meta;
  std::vector<int> counted;
  if (b.cw_on) {
    for (int cls = 0; cls < kNumClasses; ++cls) if (b.wanted[cls] && count_wide_class(cls)) counted.push_back(cls);
    if (b.big_possible && b.all) for (int cs = 0; cs < kNumWideBig; ++cs) counted.push_back(kWideBigBase + cs);
  }
  b.cw_ran = !counted.empty();
  if (b.cw_ran) {
    bool vc = false;                                          // (both groups above 1 024 samples: the value-domain form, all tests)
    for (int c : counted) vc = vc || class_forms(c).count == kCountValue;
    NMOD_HIP(k1.count_wide_prepare(counted.data(), (int)counted.size(), b.stream, ra, cww));
    NMOD_HIP(k1.count_wide_run(b.num_cus, b.npos, b.stream, ra, cww, vc));
  }
  // a class's sorting form; where the counting form was in play (its gate is set, on the device) it walks the work list
  auto launch_class = [&](int cls, bool cw) -> hipError_t {
    ra.class_id = cls; ra.alt_gates = cw ? cww.gates : nullptr; ra.alt_list = ws.work_list; ra.alt_meta = ws.work_meta;
    const hipError_t e = k1.rank_stats(cls, b.num_cus, b.npos, b.stream, ra);
    ra.alt_gates = nullptr;
    return e;
  };
  for (int cls = 0; cls < kNumClasses; ++cls) if (b.wanted[cls]) NMOD_HIP(launch_class(cls, b.cw_on && count_wide_class(cls)));
  // larger group of 2 049 .. 4 096 samples against at most 256: rank_hist_kernel WIDE as well
  if (b.big_possible && b.all) for (int cs = 0; cs < kNumWideBig; ++cs) NMOD_HIP(launch_class(kWideBigBase + cs, b.cw_on));
  if (b.wide_redo) {
    WideRedoArgs wr;
    wr.sig0 = b.sig0; wr.sig1 = b.sig1; wr.off0 = b.off0; wr.off1 = b.off1; wr.stride0 = b.stride0; wr.stride1 = b.stride1;
    wr.list = ws.redo; wr.count = ws.meta + kMetaWideRedo; wr.tie = ws.tie;
    hipLaunchKernelGGL(wide_redo_kernel, dim3((unsigned)std::min<int64_t>(b.npos, (int64_t)b.num_cus * 2)), dim3(kBigThreads), 0, b.stream, wr);
    NMOD_HIP(hipGetLastError());
  }
  return NMOD_OK;
}

// the arguments of a large-position launch over the list of class `big_class` (counts and offsets in `class_meta`, positions in
// ws.order), writing K1's outputs; scratch / cursor: the key slab and its bump allocator, where the form sorts in one
static BigArgs big_args(const Batch& b, const void* sig0, const void* sig1, const int32_t* class_meta, int big_class, bool all,
                        void* scratch, int32_t* cursor) {
  BigArgs bg;
  memset(&bg, 0, sizeof(bg));
  bg.sig0 = sig0; bg.sig1 = sig1; bg.off0 = b.off0; bg.off1 = b.off1; bg.stride0 = b.stride0; bg.stride1 = b.stride1;
  bg.pos_list = b.ws.order; bg.class_meta = class_meta; bg.big_class = big_class; bg.all = all ? 1 : 0;
  bg.scratch = scratch; bg.cursor = reinterpret_cast<unsigned long long*>(cursor);
  bg.ks_num = b.ws.ks_num; bg.mwu_s = b.ws.mwu_s; bg.tie = b.ws.tie; bg.moments = b.ws.moments; bg.ks_d_ref = b.ws.ks_d_ref;
  return bg;
}

// the large positions of a binned batch: the deep form, big_rank_kernel, big_hist_kernel
static int enqueue_large(Batch& b) {
  if (!b.big_possible && !b.deep_possible) return NMOD_OK;
  const nmod_params* prm = b.prm;
  hipStream_t stream = b.stream;
  const Workspace& ws = b.ws;
  // the only host round trip of this path: how many large (and deep) positions, how much scratch
  int32_t head[8];
  NMOD_HIP(hipMemcpyAsync(&head[0], ws.meta + kBigClass, 8, hipMemcpyDeviceToHost, stream));     // kBigClass, kBigHistClass
  NMOD_HIP(hipMemcpyAsync(&head[2], ws.meta + kMetaBigTotal, 8, hipMemcpyDeviceToHost, stream));
  if (b.deep_possible) {
    NMOD_HIP(hipMemcpyAsync(&head[4], ws.meta + kDeepClass, 4, hipMemcpyDeviceToHost, stream));
    NMOD_HIP(hipMemcpyAsync(&head[6], ws.meta + kMetaDeepTiles, 8, hipMemcpyDeviceToHost, stream));
  } else {
    head[4] = 0; head[6] = 0; head[7] = 0;
  }
  NMOD_HIP(hipStreamSynchronize(stream));
  if (head[4] > 0) {
    unsigned long long tiles;
    memcpy(&tiles, &head[6], 8);
    const int rc = enqueue_deep(prm, b.da, b.deep_scratch, b.deep_dtype, b.f64 ? (const void*)b.f64->d0 : b.sig0,
                                b.f64 ? (const void*)b.f64->d1 : b.sig1, b.off0, b.off1, b.stride0, b.stride1, ws, head[4], (int64_t)tiles,
                                std::max(b.max0, b.max1), b.all, b.num_cus, stream);
    if (rc != NMOD_OK) return rc;
  }
  const int64_t nbig = head[0], nbig_hist = head[1];
  unsigned long long total;
  memcpy(&total, &head[2], 8);
  if (nbig > 0) {
    DevScratch big_scratch;
    NMOD_HIP(big_scratch.alloc((size_t)total * 4, stream, prm->device));
    const BigArgs bg = big_args(b, b.sig0, b.sig1, ws.meta, kBigClass, b.all, big_scratch.p, ws.meta + kMetaBigCursor);
    const unsigned blocks = (unsigned)std::min<int64_t>(nbig, (int64_t)b.num_cus * 4);   // 4 x 33 KB of LDS per CU
    if (prm->dtype == NMOD_DTYPE_F32) hipLaunchKernelGGL(big_rank_kernel<0>, dim3(blocks), dim3(kBigThreads), 0, stream, bg);
    else hipLaunchKernelGGL(big_rank_kernel<1>, dim3(blocks), dim3(kBigThreads), 0, stream, bg);
    NMOD_HIP(hipGetLastError());
    NMOD_HIP(big_scratch.release(stream));
  }
  if (nbig_hist > 0) {
    const BigArgs bg = big_args(b, b.sig0, b.sig1, ws.meta, kBigHistClass, true, nullptr, nullptr);
    const unsigned blocks = (unsigned)std::min<int64_t>(nbig_hist, (int64_t)b.num_cus * 2);        // 80 KB of LDS per block
    auto kfn = prm->dtype == NMOD_DTYPE_F32 ? big_hist_kernel<0> : big_hist_kernel<1>;
    NMOD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBigHistLds));
    hipLaunchKernelGGL(kfn, dim3(blocks), dim3(kBigThreads), kBigHistLds, stream, bg);
    NMOD_HIP(hipGetLastError());
  }
  return NMOD_OK;
}

// float64 samples behind the keys: redo the positions whose keys tied with 64-bit keys, moments from the samples
static int enqueue_f64_fixups(Batch& b) {
  const F64Src* f64 = b.f64;
  const Workspace& ws = b.ws;
  hipStream_t stream = b.stream;
  F64Args fx;
  memset(&fx, 0, sizeof(fx));
  fx.d0 = f64->d0; fx.d1 = f64->d1; fx.off0 = b.off0; fx.off1 = b.off1; fx.stride0 = b.stride0; fx.stride1 = b.stride1;
  fx.npos = b.npos; fx.cls3 = f64->cls3; fx.tied = ws.tied; fx.cls = b.binned ? ws.cls : nullptr; fx.deep = b.deep_flag ? 1 : 0;
  fx.order = ws.order; fx.meta = ws.meta; fx.moments = ws.moments;
  const unsigned gb = (unsigned)std::min<int64_t>((b.npos + 255) / 256, 4096);
  hipLaunchKernelGGL(f64_redo_list_kernel, dim3(gb), dim3(256), 0, stream, fx);
  NMOD_HIP(hipGetLastError());
  int32_t nredo = 0; unsigned long long total = 0;
  NMOD_HIP(hipMemcpyAsync(&nredo, ws.meta + kMetaRedo, 4, hipMemcpyDeviceToHost, stream));
  NMOD_HIP(hipMemcpyAsync(&total, ws.meta + kMetaRedoTotal, 8, hipMemcpyDeviceToHost, stream));
  NMOD_HIP(hipStreamSynchronize(stream));
  if (nredo > 0) {
    DevScratch redo_scratch;
    NMOD_HIP(redo_scratch.alloc((size_t)total * 8, stream, b.prm->device));
    const BigArgs bg = big_args(b, f64->d0, f64->d1, ws.meta + kMetaRedo, 0, b.all, redo_scratch.p, ws.meta + kMetaRedoCursor);
    const unsigned blocks = (unsigned)std::min<int64_t>(nredo, (int64_t)b.num_cus * 4);
    ScopedKernelTimer tm(b.prm->timer, NMOD_KERNEL_RANK_STATS, stream);
    hipLaunchKernelGGL(big_rank_kernel<2>, dim3(blocks), dim3(kBigThreads), 0, stream, bg);
    NMOD_HIP(hipGetLastError());
    NMOD_HIP(redo_scratch.release(stream));
  }
  if (b.all) {
    const unsigned mb = (unsigned)std::min<int64_t>((b.npos + 3) / 4, (int64_t)b.num_cus * 16);
    hipLaunchKernelGGL(f64_moments_kernel, dim3(mb), dim3(256), 0, stream, fx);
    NMOD_HIP(hipGetLastError());
  }
  return NMOD_OK;
}

// the non-finite scan, the deep positions' outputs, K2 (p-values) and K3 (the combined track)
static int enqueue_outputs(Batch& b) {
  const nmod_params* prm = b.prm;
  const Workspace& ws = b.ws;
  const F64Src* f64 = b.f64;
  hipStream_t stream = b.stream;
  FinalizeArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.npos = b.npos; fa.off0 = b.off0; fa.off1 = b.off1; fa.stride0 = b.stride0; fa.stride1 = b.stride1;
  fa.ks_num = ws.ks_num; fa.mwu_s = ws.mwu_s; fa.tie = ws.tie; fa.moments = ws.moments; fa.ks_d_ref = b.ra.ks_rational_d ? nullptr : ws.ks_d_ref;   // every K1 form writes ks_2samp's float form of D (unless the caller opted out)
  fa.tests = b.tests; fa.want_mstd = prm->want_mstd; fa.out = *b.out;
  // what K1 covered: exactly the limits the classifier used (the promised / measured maxima), in every mode —
  // a position beyond them was skipped by K1 and must be flagged TOO_LARGE here, never read from the workspace
  fa.max_n0 = std::max<int64_t>(std::min<int64_t>(b.max0, NMOD_MAX_RANKED), 1);
  fa.max_n1 = std::max<int64_t>(std::min<int64_t>(b.max1, NMOD_MAX_RANKED), 1);
  fa.min_cap = 0;
  if (b.stride0 > 0 && b.stride1 > 0) fa.ks_scale = ks_size_scale(b.stride0, b.stride1);   // (else 0: K2 works it out per position)
  if (b.deep_possible) { fa.deep_lim0 = std::max<int64_t>(b.max0, 1); fa.deep_lim1 = std::max<int64_t>(b.max1, 1); }   // (K2 leaves them to the deep form)
  if ((prm->flags & NMOD_FLAG_CHECK_FINITE) && prm->dtype != NMOD_DTYPE_I16_MILLI) {
    // one pass over the samples: the float64 samples themselves where the keys are their float32 images
    NonfiniteArgs na;
    memset(&na, 0, sizeof(na));
    na.sig0 = f64 ? (const void*)f64->d0 : b.sig0; na.sig1 = f64 ? (const void*)f64->d1 : b.sig1; na.f64 = f64 ? 1 : 0;
    na.off0 = b.off0; na.off1 = b.off1; na.stride0 = b.stride0; na.stride1 = b.stride1; na.npos = b.npos;
    na.lim0 = fa.max_n0; na.lim1 = fa.max_n1; na.flag = ws.nonfinite;
    const unsigned nb_ = (unsigned)std::min<int64_t>((b.npos + 3) / 4, (int64_t)b.num_cus * 32);
    hipLaunchKernelGGL(nonfinite_scan_kernel, dim3(nb_), dim3(256), 0, stream, na);
    NMOD_HIP(hipGetLastError());
    fa.nonfinite = ws.nonfinite;
  }
  if (b.want_comb) {                     // the combine needs the KS track even if the caller does not
    if (!fa.out.ks_d) fa.out.ks_d = ws.tmp_ks_d;
    if (!fa.out.ks_p) fa.out.ks_p = ws.tmp_ks_p;
  }
  {
    ScopedKernelTimer tm(prm->timer, NMOD_KERNEL_FINALIZE, stream);
    if (b.da.ndeep > 0) {                // the deep positions' outputs (K2 skips them), then the slab goes back to the pool
      const unsigned db = (unsigned)((b.da.ndeep + 255) / 256);
      const int32_t rat = b.ra.ks_rational_d, chk = (prm->flags & NMOD_FLAG_CHECK_FINITE) ? 1 : 0;
      if (b.deep_dtype == NMOD_DTYPE_I16_MILLI) hipLaunchKernelGGL(deep_finalize_kernel<1>, dim3(db), dim3(256), 0, stream, b.da, fa, rat, chk);
      else if (b.deep_dtype == NMOD_DTYPE_F64) hipLaunchKernelGGL(deep_finalize_kernel<2>, dim3(db), dim3(256), 0, stream, b.da, fa, rat, chk);
      else hipLaunchKernelGGL(deep_finalize_kernel<0>, dim3(db), dim3(256), 0, stream, b.da, fa, rat, chk);
      NMOD_HIP(hipGetLastError());
      NMOD_HIP(b.deep_scratch.release(stream));
    }
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((b.npos + 255) / 256)), dim3(256), 0, stream, fa);
    NMOD_HIP(hipGetLastError());
  }
  if (b.want_comb) return launch_combine(prm, stream, b.npos, fa.out.ks_d, fa.out.ks_p, b.run_id, b.out->comb_st, b.out->comb_p);
  return NMOD_OK;
}

// One batch in device memory on prm->stream.  stats (may be null): where the facts of nmod_last_dispatch_stats sit in `workspace`.
int detect_device(const nmod_params* prm, int64_t npos, const void* sig0, const int64_t* off0,
                  const void* sig1, const int64_t* off1, const int32_t* run_id, void* workspace,
                  int64_t workspace_bytes, nmod_out* out, StatsArgs* stats, const F64Src* f64) {
  if (npos == 0) return NMOD_OK;
  if (!sig0 || !sig1 || !out) return NMOD_ERR_INVALID_ARG;
  if ((prm->stride0 <= 0 && !off0) || (prm->stride1 <= 0 && !off1)) return NMOD_ERR_INVALID_ARG;
  if (npos > INT32_MAX) return NMOD_ERR_INVALID_ARG;
  const bool want_comb = prm->method != NMOD_METHOD_KS && (out->comb_st || out->comb_p);
  if (want_comb && (!out->comb_st || !out->comb_p)) return NMOD_ERR_INVALID_ARG;
  if (want_comb && prm->nb > 0 && !run_id) return NMOD_ERR_INVALID_ARG;
  Batch b{};
  b.ws = carve(workspace, npos);
  if (!workspace || workspace_bytes < b.ws.bytes) return NMOD_ERR_WORKSPACE;
  NMOD_HIP(device_cus(prm->device, &b.num_cus));
  b.prm = prm; b.stream = (hipStream_t)prm->stream; b.npos = npos; b.sig0 = sig0; b.sig1 = sig1; b.off0 = off0; b.off1 = off1;
  b.stride0 = prm->stride0 > 0 ? prm->stride0 : 0; b.stride1 = prm->stride1 > 0 ? prm->stride1 : 0;
  b.run_id = run_id; b.out = out; b.f64 = f64; b.want_comb = want_comb;
  int rc = plan_batch(b);
  if (rc == NMOD_OK && b.binned) rc = enqueue_bins(b);
  if (rc != NMOD_OK) return rc;
  {
    ScopedKernelTimer tm(prm->timer, NMOD_KERNEL_RANK_STATS, b.stream);
    rc = enqueue_k1(b);
    if (rc == NMOD_OK) rc = enqueue_large(b);
  }
  if (rc == NMOD_OK && f64) rc = enqueue_f64_fixups(b);
  if (rc == NMOD_OK) rc = enqueue_outputs(b);
  if (rc != NMOD_OK || !stats) return rc;
  memset(stats, 0, sizeof(*stats));
  stats->npos = npos; stats->uniform_cls = b.binned ? -1 : b.uniform_cls;
  stats->meta = b.ws.meta; stats->work_meta = b.ws.work_meta; stats->gates = b.ws.work_meta + 2 * kClassStride; stats->cnt_done = b.ws.cnt_done;
  stats->cnt256_ran = (b.wanted[kNumGeneralClasses + 2] && b.ra.cnt_gate) ? 1 : 0; stats->cw_ran = b.cw_ran ? 1 : 0;
  stats->f64 = f64 ? 1 : 0; stats->acc = b.ws.stats;
  return NMOD_OK;
}

// ---------------------------------------------------------------- host staging (nmod_combine_track's small buffers)
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
};

// ---------------------------------------------------------------- float64 front end
// Gives every position order-preserving float32 keys (f64_encode_kernel) and runs the batch on them; see F64Args.
// Device memory only (the host entry hands its chunks over as device memory, host_pipeline.hip).  bounds: the first and
// one-past-last element of each array in use, {b0, e0, b1, e1}, when the caller knows them (no round trip for the offsets).
int detect_f64(const nmod_params* prm, int64_t npos, const void* sig0, const int64_t* off0,
               const void* sig1, const int64_t* off1, const int32_t* run_id, void* workspace,
               int64_t workspace_bytes, nmod_out* out, StatsArgs* stats, const int64_t* bounds) {
  if (npos == 0) return NMOD_OK;
  if (!sig0 || !sig1 || !out) return NMOD_ERR_INVALID_ARG;
  if ((prm->stride0 <= 0 && !off0) || (prm->stride1 <= 0 && !off1)) return NMOD_ERR_INVALID_ARG;
  hipStream_t stream = (hipStream_t)prm->stream;
  // sample counts and the first sample of each array (offsets need not start at 0)
  int64_t b0 = 0, e0 = prm->stride0 * npos, b1 = 0, e1 = prm->stride1 * npos;
  if (bounds) { b0 = bounds[0]; e0 = bounds[1]; b1 = bounds[2]; e1 = bounds[3]; }
  else {
    if (prm->stride0 <= 0) {
      int64_t t[2]; NMOD_HIP(hipMemcpyAsync(&t[0], off0, 8, hipMemcpyDeviceToHost, stream));
      NMOD_HIP(hipMemcpyAsync(&t[1], off0 + npos, 8, hipMemcpyDeviceToHost, stream)); NMOD_HIP(hipStreamSynchronize(stream)); b0 = t[0]; e0 = t[1];
    }
    if (prm->stride1 <= 0) {
      int64_t t[2]; NMOD_HIP(hipMemcpyAsync(&t[0], off1, 8, hipMemcpyDeviceToHost, stream));
      NMOD_HIP(hipMemcpyAsync(&t[1], off1 + npos, 8, hipMemcpyDeviceToHost, stream)); NMOD_HIP(hipStreamSynchronize(stream)); b1 = t[0]; e1 = t[1];
    }
  }
  const int64_t n0 = e0 - b0, n1 = e1 - b1;
  if (n0 < 0 || n1 < 0) return NMOD_ERR_INVALID_ARG;
  DevScratch enc0, enc1, d_cls3;                    // stream-ordered, from the library's pool: no device-wide synchronisation per batch
  NMOD_HIP(enc0.alloc((size_t)n0 * 4, stream, prm->device)); NMOD_HIP(enc1.alloc((size_t)n1 * 4, stream, prm->device));
  NMOD_HIP(d_cls3.alloc((size_t)npos, stream, prm->device));
  // pointers in the index space of the offsets (sample i of the arrays sits at [i], whatever the first offset is)
  F64Src src;
  src.d0 = (const double*)sig0; src.d1 = (const double*)sig1; src.cls3 = (uint8_t*)d_cls3.p;
  F64Args fx;
  memset(&fx, 0, sizeof(fx));
  fx.d0 = src.d0; fx.d1 = src.d1; fx.off0 = off0; fx.off1 = off1;
  fx.stride0 = prm->stride0 > 0 ? prm->stride0 : 0; fx.stride1 = prm->stride1 > 0 ? prm->stride1 : 0;
  fx.npos = npos; fx.k0 = (float*)enc0.p - b0; fx.k1 = (float*)enc1.p - b1; fx.cls3 = src.cls3;
  int num_cus = 0;
  NMOD_HIP(device_cus(prm->device, &num_cus));
  const unsigned eb = (unsigned)std::min<int64_t>((npos + 3) / 4, (int64_t)num_cus * 16);
  hipLaunchKernelGGL(f64_encode_kernel, dim3(eb), dim3(256), 0, stream, fx);
  NMOD_HIP(hipGetLastError());
  nmod_params ep = *prm;
  ep.dtype = NMOD_DTYPE_F32;
  int rc = detect_device(&ep, npos, fx.k0, off0, fx.k1, off1, run_id, workspace, workspace_bytes, out, stats, &src);
  // the key buffers go back to the pool in stream order
  const hipError_t r0 = enc0.release(stream), r1 = enc1.release(stream), r2 = d_cls3.release(stream);
  if (rc == NMOD_OK && (r0 != hipSuccess || r1 != hipSuccess || r2 != hipSuccess)) { g_last_hip = r0 != hipSuccess ? r0 : (r1 != hipSuccess ? r1 : r2); rc = NMOD_ERR_HIP; }
  return rc;
}

}  // namespace nmod

// =================================================================== C ABI
using namespace nmod;

extern "C" {

int nmod_abi_version(void) { return NMOD_ABI_VERSION; }

int nmod_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int nmod_item_claim_plan(int64_t items, int64_t waves, int32_t flags, int64_t* plan) {
  if (items < 0 || waves < 1 || !plan) return NMOD_ERR_INVALID_ARG;
  const ItemClaimPlan p = item_claim_plan<int64_t>(items, waves, (flags & NMOD_FLAG_K1_STATIC_ITEMS) != 0);
  plan[0] = p.rounds; plan[1] = p.first; plan[2] = p.chunk; plan[3] = p.dynamic;
  return NMOD_OK;
}

int64_t nmod_workspace_bytes(const nmod_params* prm, int64_t npos) {
  (void)prm;
  if (npos < 0) return 0;
  return carve(nullptr, npos).bytes;
}

int nmod_detect_batch(const nmod_params* prm, int64_t npos, const void* sig0, const int64_t* off0,
                      const void* sig1, const int64_t* off1, const int32_t* run_id, void* workspace,
                      int64_t workspace_bytes, nmod_out* out) {
  g_dispatch.valid = false;                      // (a failed call leaves no record: it could point into memory handed back)
  int rc = check_params(prm);
  if (rc != NMOD_OK) return rc;
  if (npos < 0) return NMOD_ERR_INVALID_ARG;
  rc = select_device(prm, nullptr);
  if (rc != NMOD_OK) return rc;
  DispatchRec rec;                               // an empty batch: the totals of a host record, all zero
  rec.host = true; rec.npos = npos;
  if (prm->memspace == NMOD_MEM_HOST) {
    rc = detect_host_pipelined(prm, npos, sig0, off0, sig1, off1, run_id, out, rec.host_totals);
  } else {
    rc = prm->dtype == NMOD_DTYPE_F64 ? detect_f64(prm, npos, sig0, off0, sig1, off1, run_id, workspace, workspace_bytes, out, &rec.args)
                                      : detect_device(prm, npos, sig0, off0, sig1, off1, run_id, workspace, workspace_bytes, out, &rec.args);
    if (npos > 0) { rec.host = false; rec.device = prm->device; rec.stream = (hipStream_t)prm->stream; }
  }
  if (rc != NMOD_OK) return rc;
  rec.valid = true;
  g_dispatch = rec;
  return NMOD_OK;
}

int nmod_combine_track(const nmod_params* prm, int64_t npos, const double* ks_d, const double* ks_p,
                       const int32_t* run_id, double* comb_st, double* comb_p) {
  int rc = check_params(prm);
  if (rc != NMOD_OK) return rc;
  if (npos < 0 || prm->method == NMOD_METHOD_KS) return NMOD_ERR_INVALID_ARG;
  if (npos == 0) return NMOD_OK;
  if (!ks_p || !comb_st || !comb_p || (prm->nb == 0 && !ks_d) || (prm->nb > 0 && !run_id)) return NMOD_ERR_INVALID_ARG;
  if (nmod_device_count() <= prm->device || prm->device < 0) return NMOD_ERR_NO_DEVICE;
  NMOD_HIP(hipSetDevice(prm->device));
  hipStream_t stream = (hipStream_t)prm->stream;
  if (prm->memspace == NMOD_MEM_DEVICE)
    return launch_combine(prm, stream, npos, ks_d, ks_p, run_id, comb_st, comb_p);
  DevBuf d_d, d_p, d_r, d_o;
  NMOD_HIP(d_d.alloc(npos * 8)); NMOD_HIP(d_p.alloc(npos * 8)); NMOD_HIP(d_r.alloc(npos * 4)); NMOD_HIP(d_o.alloc(npos * 16));
  if (ks_d) NMOD_HIP(hipMemcpyAsync(d_d.p, ks_d, npos * 8, hipMemcpyHostToDevice, stream));
  NMOD_HIP(hipMemcpyAsync(d_p.p, ks_p, npos * 8, hipMemcpyHostToDevice, stream));
  if (run_id) NMOD_HIP(hipMemcpyAsync(d_r.p, run_id, npos * 4, hipMemcpyHostToDevice, stream));
  double* o = (double*)d_o.p;
  rc = launch_combine(prm, stream, npos, (const double*)d_d.p, (const double*)d_p.p, (const int32_t*)d_r.p, o, o + npos);
  if (rc != NMOD_OK) { hipStreamSynchronize(stream); return rc; }
  NMOD_HIP(hipMemcpyAsync(comb_st, o, npos * 8, hipMemcpyDeviceToHost, stream));
  NMOD_HIP(hipMemcpyAsync(comb_p, o + npos, npos * 8, hipMemcpyDeviceToHost, stream));
  NMOD_HIP(hipStreamSynchronize(stream));
  return NMOD_OK;
}

int nmod_describe_dispatch(const nmod_params* prm, int64_t n0, int64_t n1, char* buf, int32_t buflen) {
  int rc = check_params(prm);
  if (rc != NMOD_OK) return rc;
  if (!buf || buflen < 8 || n0 <= 0 || n1 <= 0) return NMOD_ERR_INVALID_ARG;
  const bool want_comb = prm->method != NMOD_METHOD_KS;
  const int tests = prm->tests | (want_comb ? NMOD_TEST_KS : 0);
  const bool all = (tests & (NMOD_TEST_MWU | NMOD_TEST_WELCH)) != 0 || prm->want_mstd;
  // the classifier of the device (NMOD_DTYPE_F64: the narrower dtype is a property of the data), under the format's limits
  const bool deep = (prm->flags & NMOD_FLAG_DEEP) != 0;
  const int64_t cap = deep ? NMOD_MAX_DEEP : NMOD_MAX_RANKED;
  const int cls = classify_position(n0, n1, ClassRule{cap, cap, all ? 0 : 1, deep ? 1 : 0});
  if (cls == 255) return NMOD_ERR_TOO_LARGE;
  // (NMOD_DTYPE_F64 runs on per-position float32 keys: the float32 instances; the deep form sorts the samples as 64-bit keys)
  const char* dt = prm->dtype == NMOD_DTYPE_I16_MILLI ? "i16" : "f32";
  const ClassForms f = class_forms(cls);
  char form[64];
  if (f.sort == kSortDeep) snprintf(form, sizeof(form), "deep_rank_kernel<%s>", prm->dtype == NMOD_DTYPE_F64 ? "f64" : dt);
  else if (f.sort == kSortBig) snprintf(form, sizeof(form), cls == kBigHistClass ? "big_hist_kernel<%s>" : "big_rank_kernel<%s>", dt);
  else if (f.sort == kSortHistWide) snprintf(form, sizeof(form), "rank_hist_kernel<%d,64,%s,wide>", 1 << wide_class_of_s(cls), dt);
  else if (f.sort == kSortPair) snprintf(form, sizeof(form), "rank_pair_kernel<%d,%d,%s>", 1 << (cls / kNumSizeClasses), 1 << (cls % kNumSizeClasses), dt);
  else {
    const bool ks = f.sort == kSortKs;
    const int c = ks ? cls - kKsClassBase : cls - kNumGeneralClasses;
    const int LG = ks ? ksonly_lanes_per_group(c) : packed_lanes_per_group(c), R = (64 << c) / LG;
    snprintf(form, sizeof(form), ks ? "ks_rank_kernel<%d,%d,%s>" : "rank_hist_kernel<%d,%d,%s>", R, LG, dt);
  }
  // the counting form first when the device-side probe finds the class (the batch, for the 256-capacity class) event-like — a
  // property of the data; in KS-only mode for a larger group of kCwKsMinQ .. kCwMaxQ samples
  const int64_t q = std::max(n0, n1);
  if (f.count == kCountNone || (!all && (q < kCwKsMinQ || q > kCwMaxQ))) { snprintf(buf, buflen, "%s", form); return NMOD_OK; }
  static const char* const counting[] = {"", "rank_count_kernel", "rank_count_wide_kernel", "rank_count_value_kernel"};
  snprintf(buf, buflen, "%s<%s%s> (event-like rows) | %s", counting[f.count], prm->dtype == NMOD_DTYPE_F64 ? "f32 keys" : dt, all ? "" : ",ks", form);
  return NMOD_OK;
}

static void assemble_dispatch_stats(const unsigned long long* raw, int64_t npos, nmod_dispatch_stats* st) {
  memset(st, 0, sizeof(*st));
  st->positions = npos;
  // the counter of each sorting form (K1Sort order)
  static int64_t nmod_dispatch_stats::* const sorting[] = {&nmod_dispatch_stats::ks_rank, &nmod_dispatch_stats::rank_hist,
      &nmod_dispatch_stats::rank_hist_wide, &nmod_dispatch_stats::rank_pair, &nmod_dispatch_stats::big, &nmod_dispatch_stats::deep};
  int64_t placed = 0;
  for (int c = 0; c < kNumPairs; ++c) {
    const int64_t n = (int64_t)raw[kStatsClass + c];
    if (n == 0) continue;
    placed += n;
    const ClassForms f = class_forms(c);
    const bool c256 = f.count == kCount256;
    const int64_t tried = (int64_t)raw[kStatsTried + c];
    const int64_t counted = c256 ? (int64_t)raw[1] : tried - (int64_t)raw[kStatsLeft + c];
    if (c256) st->rank_count += counted; else st->rank_count_wide += counted;
    st->*sorting[f.sort] += n - counted;
    st->count_tried += tried;
    st->count_rejected += tried - counted;
  }
  st->skipped = npos - placed;
  st->f64_redo = (int64_t)raw[2];
}

int nmod_last_dispatch_stats(nmod_dispatch_stats* st) {
  if (!st) return NMOD_ERR_INVALID_ARG;
  DispatchRec& d = g_dispatch;
  if (!d.valid) { memset(st, 0, sizeof(*st)); return NMOD_ERR_INVALID_ARG; }
  if (d.host) { assemble_dispatch_stats(d.host_totals, d.npos, st); return NMOD_OK; }
  unsigned long long raw[kStatsWords];
  NMOD_HIP(hipSetDevice(d.device));
  NMOD_HIP(hipMemsetAsync(d.args.acc, 0, kStatsWords * 8, d.stream));
  NMOD_HIP(enqueue_dispatch_stats(d.args, d.stream));
  NMOD_HIP(hipMemcpyAsync(raw, d.args.acc, kStatsWords * 8, hipMemcpyDeviceToHost, d.stream));
  NMOD_HIP(hipStreamSynchronize(d.stream));
  assemble_dispatch_stats(raw, d.npos, st);
  return NMOD_OK;
}

const char* nmod_build_info(void) {
  static const std::string info = "arch=gfx950 abi=" + std::to_string(NMOD_ABI_VERSION) + " hip=" + std::to_string(HIP_VERSION_MAJOR) + "." +
                                  std::to_string(HIP_VERSION_MINOR);
  return info.c_str();
}

}  // extern "C"
