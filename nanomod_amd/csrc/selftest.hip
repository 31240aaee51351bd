// nmod_selftest: the wave primitives (wave_ops.hpp), the register sort (rank_stats.hpp) and the run / tie bookkeeping
// (rank_all.hpp) on one wave, against the host.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "../../include/nanomod_hip.h"
#include "entry_common.hpp"
#include "rank_stats.hpp"
#include "rank_all.hpp"

namespace nmod {

__global__ void selftest_perm_kernel(int* out) {
  int lane = threadIdx.x & 63;
  float x = (float)lane;
  int k = 0;
  out[64 * k++ + lane] = (int)lane_xor<1>(x);
  out[64 * k++ + lane] = (int)lane_xor<2>(x);
  out[64 * k++ + lane] = (int)lane_xor<4>(x);
  out[64 * k++ + lane] = (int)lane_xor<8>(x);
  out[64 * k++ + lane] = (int)lane_xor<16>(x);
  out[64 * k++ + lane] = (int)lane_mirror<2>(x, lane);
  out[64 * k++ + lane] = (int)lane_mirror<4>(x, lane);
  out[64 * k++ + lane] = (int)lane_mirror<8>(x, lane);
  out[64 * k++ + lane] = (int)lane_mirror<16>(x, lane);
  out[64 * k++ + lane] = (int)lane_mirror<32>(x, lane);
  out[64 * k++ + lane] = (int)lane_mirror<64>(x, lane);
  out[64 * k++ + lane] = (int)lane_prev(x, -1.0f);
  out[64 * k++ + lane] = (int)lane_next(x, -1.0f);
  out[64 * k++ + lane] = wave_scan_max_i32((lane * 37) % 64 == 5 ? 1000 : (lane * 7) % 23);
  out[64 * k++ + lane] = (int)wave_max_u32((unsigned)((lane * 29) % 61));
  out[64 * k++ + lane] = (int)wave_sum_u64((unsigned long long)lane * 3ull + (1ull << 33)) ;
  out[64 * k++ + lane] = (int)(wave_sum_u64((unsigned long long)lane * 3ull + (1ull << 33)) >> 32);
  out[64 * k++ + lane] = (int)wave_sum_f64(0.5 * lane);
}

template <int R>
__global__ void selftest_sort_kernel(const float* in, float* out, int* runs) {
  int lane = threadIdx.x & 63;
  const float inf = __builtin_inff();
  LaneSel sel;
#pragma unroll
  for (int b = 0; b < 6; ++b) sel.s[b] = ((lane >> b) & 1) ? inf : -inf;
  float x[R];
#pragma unroll
  for (int r = 0; r < R; ++r) x[r] = in[r * 64 + lane];
  wave_sort<R>(x, sel, lane);
  store_sorted<R>(out, x, lane);
  unsigned pp;
  seg_runs_and_ties<R, 64, 1>(runs + lane * R, x, lane, false, pp);
}

template <int R>
static int selftest_sort(int code) {
  const int N = 64 * R;
  std::vector<float> h(N), sorted(N), got(N);
  std::vector<int> runs(N);
  uint32_t s = 12345u + R;
  for (int i = 0; i < N; ++i) { s = s * 1664525u + 1013904223u; h[i] = (float)((int)((s >> 8) % 97) - 48) * 0.25f; }   // many ties
  sorted = h; std::sort(sorted.begin(), sorted.end());
  float *din, *dout; int* druns;
  NMOD_HIP(hipMalloc(&din, N * 4)); NMOD_HIP(hipMalloc(&dout, N * 4)); NMOD_HIP(hipMalloc(&druns, N * 4));
  NMOD_HIP(hipMemcpy(din, h.data(), N * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(selftest_sort_kernel<R>, dim3(1), dim3(64), 0, 0, din, dout, druns);
  NMOD_HIP(hipMemcpy(got.data(), dout, N * 4, hipMemcpyDeviceToHost));
  NMOD_HIP(hipMemcpy(runs.data(), druns, N * 4, hipMemcpyDeviceToHost));
  hipFree(din); hipFree(dout); hipFree(druns);
  for (int i = 0; i < N; ++i) if (got[i] != sorted[i]) return code;
  for (int i = 0; i < N; ++i) {
    int st = i, en = i + 1;
    while (st > 0 && sorted[st - 1] == sorted[i]) --st;
    while (en < N && sorted[en] == sorted[i]) ++en;
    if (runs[i] != (st | (en << 16))) return code + 1;
  }
  return NMOD_OK;
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_selftest(int32_t device) {
  if (nmod_device_count() <= device || device < 0) return NMOD_ERR_NO_DEVICE;
  NMOD_HIP(hipSetDevice(device));
  const int NP = 18;
  int* d; std::vector<int> h(64 * NP);
  NMOD_HIP(hipMalloc(&d, 64 * NP * 4));
  hipLaunchKernelGGL(selftest_perm_kernel, dim3(1), dim3(64), 0, 0, d);
  NMOD_HIP(hipMemcpy(h.data(), d, 64 * NP * 4, hipMemcpyDeviceToHost));
  hipFree(d);
  int scan_in[64], run = 0, mx = 0;
  for (int l = 0; l < 64; ++l) { scan_in[l] = (l * 37) % 64 == 5 ? 1000 : (l * 7) % 23; mx = std::max(mx, (l * 29) % 61); }
  unsigned long long tot = 0; double ftot = 0;
  for (int l = 0; l < 64; ++l) { tot += (unsigned long long)l * 3ull + (1ull << 33); ftot += 0.5 * l; }
  for (int l = 0; l < 64; ++l) {
    run = std::max(run, scan_in[l]);
    const int expect[NP] = {l ^ 1, l ^ 2, l ^ 4, l ^ 8, l ^ 16, l ^ 1, l ^ 3, l ^ 7, l ^ 15, l ^ 31, l ^ 63,
                            l == 0 ? -1 : l - 1, l == 63 ? -1 : l + 1, run, mx, (int)(unsigned)tot, (int)(tot >> 32), (int)ftot};
    for (int k = 0; k < NP; ++k) if (h[64 * k + l] != expect[k]) return 1 + k;
  }
  int rc;
  if ((rc = selftest_sort<1>(100)) != NMOD_OK) return rc;
  if ((rc = selftest_sort<2>(110)) != NMOD_OK) return rc;
  if ((rc = selftest_sort<4>(120)) != NMOD_OK) return rc;
  if ((rc = selftest_sort<8>(130)) != NMOD_OK) return rc;
  if ((rc = selftest_sort<16>(140)) != NMOD_OK) return rc;
  if ((rc = selftest_sort<32>(150)) != NMOD_OK) return rc;
  return NMOD_OK;
}
