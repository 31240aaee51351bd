// nmod_read_class_rows / nmod_read_classes_step — a finite mixture of C classes over the reads, every class with its own modified share
// at every candidate site, fitted by EM: one step per call, the loop on the host (K22).  The reference project has no
// such step; the definition is the one in include/nanomod_hip.h (tests/classes_ref.py restates it).  The entries of a read are K19's
// (read_entries.hpp: the refusals and ChainCall's entries half for the rows; ReadDraw, ReadGeom and read_sum for the E-step), the walks
// are read_walk.hpp's and pos_walk.hpp's, the sort is radix_sort.hpp's and the offsets' scan site_search.hpp's; all on the caller's stream:
//   nmod_read_class_rows, once per data set
//     rh_entries_kernel<., 1>  (read_hmm.hip) entry j of read r writes its site and score to row hoff[r] + j
//     rc_rows_kernel           a wave per read: s and rread of its rows, the sort key (the site) and one integer atomic per row on
//                              the site's count
//     sp_scan_kernel           the counts' exclusive scan in place (soff)
//     rs_sort_pairs            the rows by their site, stable: within a site ascending row index (srow)
//   nmod_read_classes_step, once per EM step; the reads are not walked again
//     rc_read_kernel<C, 1>     E-step: a wave per read of up to NMOD_HMM_WAVE_MAX entries
//     rc_read_kernel<C, 4>     a workgroup of four waves per longer read
//     rc_site_kernel<C, G>     M-step: 16 lanes per site of up to NMOD_CLASSES_SMALL rows, a wave up to NMOD_CLASSES_WAVE
//     rc_site_block_kernel<C>  a workgroup per site beyond
//     rc_sums_kernel<C>        the weights and `sums`: one workgroup, a fixed order
// C is a template parameter: the C accumulators of a thread are registers.  Every sum is a fixed-order chain per thread followed by a
// fixed-order lane / wave reduction, no float atomics: a read's bits depend on the read, theta_in and w_in alone, a site's on its rows
// and their order alone.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "pos_walk.hpp"
#include "radix_sort.hpp"
#include "read_entries.hpp"
#include "read_walk.hpp"
#include "site_search.hpp"
#include "special_math.hpp"

namespace nmod {

constexpr double kRcLo = 1e-9, kRcHi = 1.0 - 1e-9;    // the range of theta (K19's of pi)
constexpr int kRcThreads = 256;

// ---------------------------------------------------------------------------------------------------------------- the rows

struct RcRowsArgs {
  int64_t nreads, nrows, nsites;
  const int64_t* hoff; const int32_t* site; const double* xs;
  double* s; int32_t* rread;
  uint64_t* keys; uint32_t* vals; unsigned long long* cnt;
};

// every row names itself, has no read and sorts behind every site (a row that no read owns keeps this)
static __global__ __launch_bounds__(256) void rc_init_kernel(RcRowsArgs a) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < a.nrows; i += (int64_t)gridDim.x * 256) {
    a.keys[i] = (uint64_t)a.nsites; a.vals[i] = (uint32_t)i;
    if (a.s) a.s[i] = 0.0;
    if (a.rread) a.rread[i] = -1;
  }
}

static __global__ __launch_bounds__(256) void rc_rows_kernel(RcRowsArgs a) {
  const int lane = threadIdx.x & 63;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.nreads; r += (int64_t)gridDim.x * 4) {
    const int64_t base = a.hoff[r], m = a.hoff[r + 1] - base;
    if (m <= 0 || base < 0 || base > a.nrows - m) continue;
    for (int64_t j = lane; j < m; j += 64) {
      const int64_t row = base + j;
      const int64_t st = a.site[row];
      if (a.rread) a.rread[row] = (int32_t)r;
      if (st >= 0 && st < a.nsites) {                           // (a row the fill left out keeps site -1 and s 0)
        if (a.s) a.s[row] = a.xs[2 * row + 1];
        a.keys[row] = (uint64_t)st;
        atomicAdd(&a.cnt[st], 1ull);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the E-step

struct RcArgs {
  int64_t nreads; const int64_t* hoff; int64_t nrows, nsites;
  ReadLists w;
  const int32_t* site; const double* s; const double* theta; const double* w_in;
  double* gamma; double* ll; int32_t* cls; uint8_t* status;
};

template <int C, int WAVES>
__global__ __launch_bounds__(kRwThreads) void rc_read_kernel(RcArgs a) {
  __shared__ unsigned sh_item;
  __shared__ double sh_sum[kRwWaves];
  const ReadGeom<WAVES> geo;
  const ReadDraw<WAVES> reads(a.w, sh_item);
  for (;;) {
    const ReadRows r = reads.next(a.hoff, a.nrows);
    if (!r.more) break;
    const int64_t read = r.read, base = r.base, m = r.m;
    if (r.none) {                                               // no entry
      if (geo.t == 0) {
        if (a.gamma) {
#pragma unroll
          for (int c = 0; c < C; ++c) a.gamma[read * C + c] = 0.0;
        }
        if (a.ll) a.ll[read] = 0.0;
        if (a.cls) a.cls[read] = -1;
        if (a.status) a.status[read] = NMOD_HMM_NO_SITE;
      }
      continue;
    }
    double l[C], s_pos = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) l[c] = 0.0;
    for (int64_t k = geo.t; k < m; k += geo.T) {
      const int64_t row = base + k;
      const int64_t st = a.site[row];
      const double sc = a.s[row];
      if (st < 0 || st >= a.nsites || !(fabs(sc) <= kDblMax)) continue;   // (rows that are not nmod_read_class_rows': skipped)
      const double tt = -expm1(-fabs(sc));
      const bool up = sc >= 0.0;
      const double* th = a.theta + st * C;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double x = th[c];
        l[c] += log1p(-((up ? 1.0 - x : x) * tt));
      }
      s_pos += fmax(sc, 0.0);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) l[c] = read_sum<WAVES>(l[c], sh_sum);
    s_pos = read_sum<WAVES>(s_pos, sh_sum);
    if (geo.t == 0) {
      double av[C];
      double mx = 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        av[c] = log(a.w_in[c]) + l[c];
        if (c == 0 || av[c] > mx) mx = av[c];                   // the first of equals
      }
      double z = 0.0;
#pragma unroll
      for (int c = 0; c < C; ++c) { av[c] = exp(av[c] - mx); z += av[c]; }
      double best = 0.0;
      int arg = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        av[c] = av[c] / z;
        if (c == 0 || av[c] > best) { best = av[c]; arg = c; }
        if (a.gamma) a.gamma[read * C + c] = av[c];
      }
      if (a.ll) a.ll[read] = (mx + log(z)) + s_pos;
      if (a.cls) a.cls[read] = arg;
      if (a.status) a.status[read] = 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the M-step

struct RmArgs {
  int64_t npos;                                   // the sites (pos_walk.hpp's name)
  int64_t nrows, nreads;
  const int64_t* soff; const int32_t* srow; const int32_t* rread; const double* s; const double* gamma; const double* theta;
  double* theta_out; double* n_site;
  PosLists<3> pl;
};

// the rows of site i (offsets that are not the rows': no row) and its class by their number
__device__ __forceinline__ void rm_span(const RmArgs& a, int64_t i, int64_t& begin, int64_t& n) {
  csr_row(a.soff, 0, i, begin, n);
  if (begin < 0 || begin > a.nrows - n) { begin = 0; n = 0; }
}
struct RmRule {
  static constexpr int NC = 3;
  using Track = void;
  static __device__ __forceinline__ int cls(const RmArgs& a, int64_t i, int64_t& begin, int64_t& n) {
    rm_span(a, i, begin, n);
    return n <= NMOD_CLASSES_SMALL ? 0 : (n <= NMOD_CLASSES_WAVE ? 1 : 2);
  }
};

// rows first, first + step, ... of a site added into N and Mo, ascending
template <int C>
__device__ __forceinline__ void rm_rows(const RmArgs& a, int64_t begin, int64_t n, const double (&th)[C], int first, int step, double (&N)[C],
                                        double (&Mo)[C]) {
  for (int64_t k = first; k < n; k += step) {
    const int64_t row = a.srow[begin + k];
    if (row < 0 || row >= a.nrows) continue;
    const int64_t r = a.rread[row];
    const double sc = a.s[row];
    if (r < 0 || r >= a.nreads || !(fabs(sc) <= kDblMax)) continue;
    const double tt = -expm1(-fabs(sc));
    const bool up = sc >= 0.0;
    const double* g = a.gamma + r * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double gm = g[c], x = th[c];
      const double post = up ? x / (1.0 - (1.0 - x) * tt) : x * (1.0 - tt) / (1.0 - x * tt);
      N[c] += gm;
      Mo[c] += gm * post;
    }
  }
}

template <int C>
__device__ __forceinline__ void rm_write(const RmArgs& a, int64_t pos, const double (&th)[C], const double (&N)[C], const double (&Mo)[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) {
    double x = th[c];
    if (N[c] > 0.0) { x = Mo[c] / N[c]; x = x < kRcLo ? kRcLo : (x > kRcHi ? kRcHi : x); }
    if (a.theta_out) a.theta_out[pos * C + c] = x;
    if (a.n_site) a.n_site[pos * C + c] = N[c];
  }
}

template <int C, int G>
__global__ __launch_bounds__(kRcThreads) void rc_site_kernel(RmArgs a) {
  const int gl = threadIdx.x & (G - 1);
  for (GroupWalk<G == 16 ? 0 : 1, G, kRcThreads> it(a.pl); it.more(); it.next()) {
    const bool have = it.have();
    int64_t pos = 0, begin = 0, n = 0;
    if (have) { pos = it.pos(); rm_span(a, pos, begin, n); }
    double th[C], N[C], Mo[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { th[c] = have ? a.theta[pos * C + c] : 0.5; N[c] = 0.0; Mo[c] = 0.0; }
    rm_rows<C>(a, begin, n, th, gl, G, N, Mo);
#pragma unroll
    for (int c = 0; c < C; ++c) { N[c] = group_sum_f64<G>(N[c]); Mo[c] = group_sum_f64<G>(Mo[c]); }
    if (have && gl == 0) rm_write<C>(a, pos, th, N, Mo);
  }
}

template <int C>
__global__ __launch_bounds__(kRcThreads) void rc_site_block_kernel(RmArgs a) {
  __shared__ double sh[kRcThreads / 64];
  for (BlockWalk<2> it(a.pl); it.more(); it.next()) {
    const int64_t pos = it.pos();
    int64_t begin, n;
    rm_span(a, pos, begin, n);
    double th[C], N[C], Mo[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { th[c] = a.theta[pos * C + c]; N[c] = 0.0; Mo[c] = 0.0; }
    rm_rows<C>(a, begin, n, th, (int)threadIdx.x, kRcThreads, N, Mo);
#pragma unroll
    for (int c = 0; c < C; ++c) { N[c] = block_sum_f64<kRcThreads / 64>(N[c], sh); Mo[c] = block_sum_f64<kRcThreads / 64>(Mo[c], sh); }
    if (threadIdx.x == 0) rm_write<C>(a, pos, th, N, Mo);
  }
}

// ---------------------------------------------------------------------------------------------------------------- the weights and sums

struct RsArgs {
  int64_t nreads, nrows, nsites;
  const int64_t* hoff; const double* ll; const double* gamma; const double* w_in;
  const double* theta; const double* theta_out; const double* n_site;
  double* w_out; double* sums;
};

// One workgroup of 256: thread t adds reads t, t + 256, ... in ascending order, then the block sum of every word.  The largest move
// of theta over the cells with N > 0 is a maximum: no order to fix
template <int C>
__global__ __launch_bounds__(256) void rc_sums_kernel(RsArgs a) {
  __shared__ double sh[4];
  double sl = 0.0, r1 = 0.0, ne = 0.0, g[C];
#pragma unroll
  for (int c = 0; c < C; ++c) g[c] = 0.0;
  for (int64_t r = threadIdx.x; r < a.nreads; r += 256) {
    const int64_t base = a.hoff[r], m = a.hoff[r + 1] - base;
    if (m <= 0 || base < 0 || base > a.nrows - m) continue;     // (a read without an entry takes no part in any sum)
    sl += a.ll[r]; r1 += 1.0; ne += (double)m;
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] += a.gamma[r * C + c];
  }
  double mv = 0.0;
  for (int64_t i = threadIdx.x; i < a.nsites * C; i += 256)
    if (a.n_site[i] > 0.0) mv = fmax(mv, fabs(a.theta_out[i] - a.theta[i]));
  sl = block_sum_f64<4>(sl, sh); r1 = block_sum_f64<4>(r1, sh); ne = block_sum_f64<4>(ne, sh);
#pragma unroll
  for (int c = 0; c < C; ++c) g[c] = block_sum_f64<4>(g[c], sh);
  // the maximum over the workgroup: the wave's by shuffles, the waves' through sh
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) mv = fmax(mv, __shfl_xor(mv, d));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = mv;
  __syncthreads();
  if (threadIdx.x == 0) {
    mv = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    if (a.sums) { a.sums[0] = sl; a.sums[1] = r1; a.sums[2] = ne; a.sums[3] = mv; }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (a.sums) a.sums[4 + c] = g[c];
      if (a.w_out) a.w_out[c] = r1 > 0.0 ? g[c] / r1 : a.w_in[c];
    }
  }
}

// f(std::integral_constant<int, C>) for a checked number of classes
template <class F>
static void for_classes(int n_classes, F f) {
  switch (n_classes) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    case 6: f(std::integral_constant<int, 6>{}); break;
    case 7: f(std::integral_constant<int, 7>{}); break;
    default: f(std::integral_constant<int, 8>{}); break;
  }
}

}  // namespace nmod

using namespace nmod;

extern "C" int nmod_read_class_rows(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                                    const double* score, int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows,
                                    const nmod_class_rows_out* out) {
  if (!rh_chain_args_ok(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_class_rows_out)) return NMOD_ERR_INVALID_ARG;
  ChainCall c(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows, !out->site, false);
  const size_t ns = c.ns, nw = c.nw;
  if (c.host && nreads == 0) {                                  // nothing to enqueue: the offsets of no row
    if (out->soff) memset(out->soff, 0, (ns + 1) * 8);
    return NMOD_OK;
  }
  const int rc = select_device(prm, &c.num_cus);
  if (rc != NMOD_OK) return rc;
  const int num_cus = c.num_cus; hipStream_t stream = c.stream;
  const int passes = nsites < 256 ? 1 : (nsites < 65536 ? 2 : (nsites < 16777216 ? 3 : 4));   // the largest key is nsites
  const bool odd = (passes & 1) != 0;

  const RhEntArgs& e = c.e;
  nmod_class_rows_out o = *out;

  // the call's slab (ChainCall's share: the read list, per row the position and the score, the site where the caller asked for none): the
  // row order where the caller asked for none, the sort's keys, second buffers and scratch, the counts without soff; a host entry's arguments
  Slab& slab = c.slab;
  const size_t o_srow = o.srow ? 0 : slab.take(nw * 4);
  const size_t o_keys = slab.take(nw * 8), o_keys2 = slab.take(nw * 8), o_vals2 = slab.take(nw * 4), o_sort = slab.take(rs_scratch_bytes(nrows));
  const size_t o_cnt = o.soff ? 0 : slab.take((ns + 1) * 8);
  c.stage();
  slab.out(o.site, nw * 4); slab.out(o.s, nw * 8); slab.out(o.rread, nw * 4); slab.out(o.soff, (ns + 1) * 8); slab.out(o.srow, nw * 4);
  NMOD_HIP(slab.commit(stream, prm->device));
  c.bind(o.site);
  int32_t* srow = o.srow ? o.srow : slab.at<int32_t>(o_srow);
  int64_t* soff = o.soff ? o.soff : slab.at<int64_t>(o_cnt);
  uint32_t* spare = slab.at<uint32_t>(o_vals2);
  // after an odd number of passes the sort leaves its result in the second buffers: srow is the buffer the result lands in
  uint32_t* vals = odd ? spare : (uint32_t*)srow;
  uint32_t* vals2 = odd ? (uint32_t*)srow : spare;

  RcRowsArgs a;
  memset(&a, 0, sizeof(a));
  a.nreads = nreads; a.nrows = nrows; a.nsites = nsites;
  a.hoff = e.hoff; a.site = e.site; a.xs = e.xs;
  a.s = o.s; a.rread = o.rread;
  a.keys = slab.at<uint64_t>(o_keys); a.vals = vals; a.cnt = (unsigned long long*)soff;

  NMOD_HIP(hipMemsetAsync(soff, 0, (ns + 1) * 8, stream));
  if (nrows > 0) {
    NMOD_HIP(hipMemsetAsync(e.site, 0xFF, nw * 4, stream));     // a row that no read fills: site -1
    hipLaunchKernelGGL(rc_init_kernel, dim3(persistent_grid(nrows, 256, (int64_t)num_cus * 16)), dim3(256), 0, stream, a);
    NMOD_HIP(c.entries());
    hipLaunchKernelGGL(rc_rows_kernel, dim3(persistent_grid(nreads, 4, (int64_t)num_cus * 16)), dim3(256), 0, stream, a);
  }
  hipLaunchKernelGGL(sp_scan_kernel, dim3(1), dim3(256), 0, stream, soff, nsites);
  if (nrows > 0) NMOD_HIP(rs_sort_pairs(a.keys, vals, slab.at<uint64_t>(o_keys2), vals2, nrows, slab.at<char>(o_sort), stream, passes));
  return launches_end(slab, stream);
}

extern "C" int nmod_read_classes_step(const nmod_params* prm, int64_t nreads, int64_t nsites, int64_t nrows, const int64_t* hoff,
                                      const int32_t* site, const double* s, const int32_t* rread, const int64_t* soff, const int32_t* srow,
                                      const nmod_classes_opts* opts, const double* theta_in, const double* w_in, const nmod_classes_out* out) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return NMOD_ERR_INVALID_ARG;
  if (!opts || opts->struct_size != (int32_t)sizeof(nmod_classes_opts)) return NMOD_ERR_INVALID_ARG;
  if (!out || out->struct_size != (int32_t)sizeof(nmod_classes_out)) return NMOD_ERR_INVALID_ARG;
  if (opts->n_classes < 1 || opts->n_classes > NMOD_CLASSES_MAX) return NMOD_ERR_INVALID_ARG;
  if (nreads < 0 || nreads > (int64_t)INT32_MAX || nsites < 0 || nsites > (int64_t)INT32_MAX - 1) return NMOD_ERR_INVALID_ARG;
  if (nrows < 0 || nrows > (int64_t)INT32_MAX) return NMOD_ERR_INVALID_ARG;
  if (nrows > 0 && (nreads == 0 || nsites == 0)) return NMOD_ERR_INVALID_ARG;
  if ((nreads > 0 && !hoff) || !soff || !w_in || (nsites > 0 && !theta_in)) return NMOD_ERR_INVALID_ARG;
  if (nrows > 0 && (!site || !s || !rread || !srow)) return NMOD_ERR_INVALID_ARG;
  const int nc = opts->n_classes;
  const bool host = prm->memspace == NMOD_MEM_HOST;
  if (host) {
    if (nreads > 0 && !rh_offsets_ok(hoff, nreads, nrows)) return NMOD_ERR_INVALID_ARG;
    if (!rh_offsets_ok(soff, nsites, nrows)) return NMOD_ERR_INVALID_ARG;
    double sum = 0.0;
    for (int c = 0; c < nc; ++c) {
      if (!rh_finite_in(w_in[c], kRcLo, kRcHi) && !(nc == 1 && w_in[c] == 1.0)) return NMOD_ERR_INVALID_ARG;
      sum += w_in[c];
    }
    if (!(fabs(sum - 1.0) <= 1e-9)) return NMOD_ERR_INVALID_ARG;
    for (int64_t i = 0; i < nsites * nc; ++i) if (!rh_finite_in(theta_in[i], kRcLo, kRcHi)) return NMOD_ERR_INVALID_ARG;
  }
  const size_t nr = (size_t)nreads, ns = (size_t)nsites, nw = (size_t)nrows, C8 = (size_t)nc * 8;
  int num_cus = 0;
  const int rc = select_device(prm, &num_cus);
  if (rc != NMOD_OK) return rc;
  hipStream_t stream = (hipStream_t)prm->stream;

  nmod_classes_out o = *out;
  const bool m_step = o.theta_out || o.n_site || o.sums;
  const bool tail = o.w_out || o.sums;
  RcArgs a;
  memset(&a, 0, sizeof(a));
  a.nreads = nreads; a.nrows = nrows; a.nsites = nsites;
  a.hoff = hoff; a.site = site; a.s = s; a.theta = theta_in; a.w_in = w_in;

  // one slab: the read lists and the site lists; gamma and ll where a later kernel reads them and the caller asked for none, theta_out
  // and N the same for the sums; for the host entry the inputs and outputs as well
  Slab slab(host);
  const ReadListSpace by_entries(slab, nr);
  const PosListSpace<3> by_rows(slab, ns);
  const size_t o_gamma = o.gamma || !(m_step || tail) ? 0 : slab.take(nr * C8), o_ll = o.ll || !tail ? 0 : slab.take(nr * 8);
  const size_t o_th = o.theta_out || !o.sums ? 0 : slab.take(ns * C8), o_n = o.n_site || !o.sums ? 0 : slab.take(ns * C8);
  slab.in(a.hoff, (nr + 1) * 8); slab.in(a.site, nw * 4); slab.in(a.s, nw * 8); slab.in(rread, nw * 4); slab.in(soff, (ns + 1) * 8);
  slab.in(srow, nw * 4); slab.in(a.theta, ns * C8); slab.in(a.w_in, C8);
  slab.out(o.gamma, nr * C8); slab.out(o.ll, nr * 8); slab.out(o.cls, nr * 4); slab.out(o.status, nr);
  slab.out(o.theta_out, ns * C8); slab.out(o.n_site, ns * C8); slab.out(o.w_out, C8); slab.out(o.sums, (size_t)(4 + nc) * 8);
  NMOD_HIP(slab.commit(stream, prm->device));
  a.gamma = o.gamma ? o.gamma : (m_step || tail ? slab.at<double>(o_gamma) : nullptr);
  a.ll = o.ll ? o.ll : (tail ? slab.at<double>(o_ll) : nullptr);
  a.cls = o.cls; a.status = o.status;

  RmArgs g;
  memset(&g, 0, sizeof(g));
  g.npos = nsites; g.nrows = nrows; g.nreads = nreads;
  g.soff = soff; g.srow = srow; g.rread = rread; g.s = a.s; g.gamma = a.gamma; g.theta = a.theta;
  g.theta_out = o.theta_out ? o.theta_out : (o.sums ? slab.at<double>(o_th) : nullptr);
  g.n_site = o.n_site ? o.n_site : (o.sums ? slab.at<double>(o_n) : nullptr);

  RsArgs z;
  memset(&z, 0, sizeof(z));
  z.nreads = nreads; z.nrows = nrows; z.nsites = o.sums ? nsites : 0;
  z.hoff = a.hoff; z.ll = a.ll; z.gamma = a.gamma; z.w_in = a.w_in; z.theta = a.theta; z.theta_out = g.theta_out; z.n_site = g.n_site;
  z.w_out = o.w_out; z.sums = o.sums;

  if (nreads > 0) NMOD_HIP(by_entries.fill(slab, a.hoff, nreads, num_cus, stream, a.w, NMOD_HMM_WAVE_MAX));
  if (m_step && nsites > 0) NMOD_HIP(by_rows.fill<RmRule>(slab, g, num_cus, stream));
  for_classes(nc, [&](auto tag) {
    constexpr int C = decltype(tag)::value;
    if (nreads > 0) rh_launch(a, rc_read_kernel<C, 1>, rc_read_kernel<C, kRwWaves>, num_cus, stream);
    if (m_step && nsites > 0) {
      launch_groups<16, kRcThreads>(rc_site_kernel<C, 16>, g, num_cus, stream);
      launch_groups<64, kRcThreads>(rc_site_kernel<C, 64>, g, num_cus, stream);
      launch_blocks<kRcThreads>(rc_site_block_kernel<C>, g, num_cus, stream);
    }
    if (tail) hipLaunchKernelGGL(rc_sums_kernel<C>, dim3(1), dim3(256), 0, stream, z);
  });
  return launches_end(slab, stream);
}
