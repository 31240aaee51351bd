// What the entries that run a chain over the candidate sites of a read share (K19 nmod_read_sites_count / nmod_read_hmm and K21
// nmod_read_hmm_grad in read_hmm.hip, K20 nmod_read_viterbi in read_viterbi.hip, K22 nmod_read_class_rows / nmod_read_classes_step in
// read_classes.hip).  Kernels: the threads of a read (ReadGeom), the sum over them (read_sum), and the loop over the reads of a class
// with their rows (ReadDraw: the entries kernel and K22's E-step; the chain kernels of K19 - K21 spell the same loop out, see there).
// Host: the arguments of the kernel that counts and fills the ENTRIES of a read and the call that enqueues it (read_hmm.hip's, compiled
// once), the launch of the two forms of a kernel, the refusals of a chain entry, and ChainCall: what it stages and enqueues.  The scans,
// the step of the chain and the count of runs stay with each translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/nanomod_hip.h"
#include "read_walk.hpp"
#include "site_search.hpp"

namespace nmod {

constexpr int kHmmChunk = NMOD_HMM_CHUNK;         // entries of a tile a thread owns
static_assert(NMOD_HMM_WAVE_MAX % (64 * NMOD_HMM_CHUNK) == 0, "the class step is a whole number of wave tiles");

// the entries of the reads (both entries): the reads, the scores, the sites, the lists of the reads by their events
struct RhEntArgs {
  int64_t nreads; const int32_t* cs; const int64_t* start; const int64_t* roff; const double* score;
  int64_t nsites; const int64_t* key;
  ReadLists w;
  int64_t* cnt;                                   // count: entries per read (hoff before its scan)
  const int64_t* hoff; int64_t nrows;             // fill: the rows of read r are hoff[r] .. hoff[r + 1] - 1
  int32_t* site; double* xs;                      // per row: the site's index; its position and the read's score there
};

// The threads of a read: a wave (WAVES == 1: list 0, thread t the lane) or the workgroup of WAVES waves (list 1)
template <int WAVES>
struct ReadGeom {
  static constexpr int CLS = WAVES == 1 ? 0 : 1;
  static constexpr int T = WAVES * 64;                          // threads a read
  static constexpr int64_t TS = (int64_t)T * kHmmChunk;         // entries a tile
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = WAVES == 1 ? lane : (int)threadIdx.x;
};

// A turn of a kernel's loop over the reads of its class.  more: false when the list is used up (nothing else is set).  The read and its
// rows base .. base + m - 1; none: no entry (or offsets that are not the rows'): thread 0 writes that kernel's outputs of such a read
struct ReadRows { bool more; int64_t read, base, m; bool none; };
// The reads of a kernel's class off the ticket (read_walk.hpp's draw_read: reached by whole waves / the whole workgroup; sh_item: a
// shared word of the kernel's).  A turn is returned by value: as members carried round the loop, base and m cost the kernels registers.
// rh_hmm_kernel, rh_grad_kernel and rv_viterbi_kernel keep the loop spelt out: through this struct they compile to other instructions
// (13 - 17 VGPRs fewer in K19 and K21, the same occupancy) that measured 0.5 - 2 % slower (profiles/chain_scaffold.txt)
template <int WAVES>
struct ReadDraw {
  const ReadLists& w; unsigned& sh_item; const unsigned cnt;
  __device__ __forceinline__ ReadDraw(const ReadLists& lists, unsigned& item) : w(lists), sh_item(item), cnt(lists.count[ReadGeom<WAVES>::CLS]) {}
  // the next read alone (the entries kernel: base, m and none unset)
  __device__ __forceinline__ ReadRows draw() const {
    const unsigned item = draw_read<WAVES>(w, sh_item);
    ReadRows r;
    if ((r.more = item < cnt)) r.read = (int64_t)w.list[ReadGeom<WAVES>::CLS][item];
    return r;
  }
  __device__ __forceinline__ ReadRows next(const int64_t* hoff, int64_t nrows) const {
    ReadRows r = draw();
    if (r.more) {
      r.base = hoff[r.read]; r.m = hoff[r.read + 1] - r.base;
      r.none = r.m <= 0 || r.base < 0 || r.base > nrows - r.m;
    }
    return r;
  }
};

// the sum of v over the threads of a read, in every thread: the wave's, or the waves' in order through sh_sum (kRwWaves words)
template <int WAVES>
__device__ __forceinline__ double read_sum(double v, double* sh_sum) {
  if constexpr (WAVES == 1) return wave_sum_f64(v); else return block_sum_f64<WAVES>(v, sh_sum);
}

// the two forms of a kernel under eight workgroups a CU
template <class A, class K1, class K4>
static void rh_launch(const A& a, K1 wave_form, K4 group_form, int num_cus, hipStream_t stream) {
  const int64_t cap = (int64_t)num_cus * 8;
  hipLaunchKernelGGL(wave_form, dim3(persistent_grid(a.nreads, kRwWaves, cap)), dim3(kRwThreads), 0, stream, a);
  hipLaunchKernelGGL(group_form, dim3(persistent_grid(a.nreads, 1, cap)), dim3(kRwThreads), 0, stream, a);
}

static void rh_ent_args(RhEntArgs& a, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff, const double* score,
                        int64_t nsites, const int64_t* key) {
  memset(&a, 0, sizeof(a));
  a.nreads = nreads; a.cs = cs; a.start = start; a.roff = roff; a.score = score; a.nsites = nsites; a.key = key;
}

static void rh_stage_reads(Slab& slab, RhEntArgs& a, size_t tot) {
  const size_t nr = (size_t)a.nreads, ns = (size_t)a.nsites;
  slab.in(a.cs, nr * 4); slab.in(a.start, nr * 8); slab.in(a.roff, (nr + 1) * 8); slab.in(a.score, tot * 8); slab.in(a.key, ns * 8);
}

// rh_entries_kernel<., true> in both forms on the stream (read_hmm.hip): e.w filled by the caller, rows hoff[r] + j written
void rh_fill_entries(const RhEntArgs& e, int num_cus, hipStream_t stream);

// The prior entries (K23).  rh_share_kernel behind the fill (read_hmm.hip): share[stride * row] = the share of e.site[row] from site_pi,
// clamped to these bounds, pi where that word is a NaN; with stride 3 the logarithms of 1 - share and of share follow it
constexpr double kSharePiLo = 1e-9, kSharePiHi = 1.0 - 1e-9;
void rh_fill_shares(const RhEntArgs& e, const double* site_pi, double pi, int stride, double* share, int num_cus, hipStream_t stream);

static bool rh_finite_in(double v, double lo, double hi) { return v >= lo && v <= hi; }   // (a NaN compares false)
static bool rh_chain_opts_ok(double pi, double length) { return rh_finite_in(pi, 1e-9, 1.0 - 1e-9) && rh_finite_in(length, 1e-3, 1e9); }

// host-resident offsets of rows: they start at 0, never decrease and end at nrows
static bool rh_offsets_ok(const int64_t* off, int64_t n, int64_t nrows) { return off[0] == 0 && csr_offsets_ok(off, n) && off[n] == nrows; }

// The refusals the chain entries share, all before any device work: the params, the counts, the reads and the sites, the offsets of
// a host call, rows without a read or a site to own them.  An entry adds the checks of its own opts and out structs
static bool rh_chain_args_ok(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                             const double* score, int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows) {
  if (check_prm_common(prm, kPrmAnyDtype) != NMOD_OK) return false;
  if (nrows < 0 || nrows > (int64_t)INT32_MAX || (nreads > 0 && !hoff)) return false;
  if (!sp_walk_args_ok(prm, nreads, cs, start, roff, score, nsites, key, nullptr, 0)) return false;
  if (prm->memspace == NMOD_MEM_HOST && nreads > 0 && !rh_offsets_ok(hoff, nreads, nrows)) return false;
  return !(nrows > 0 && (nreads == 0 || nsites == 0));
}

// What a chain entry stages and enqueues in front of its own kernel, for arguments rh_chain_args_ok has passed.  The entry sets num_cus
// (select_device), takes what else it needs, then: stage(), its slab.out lines, slab.commit, bind(), its memsets, entries() / lists()
struct ChainCall {
  const bool host; int num_cus = 0; const hipStream_t stream;
  const size_t nr, ns, nw, tot;                   // reads, sites, rows; the events of a host call
  RhEntArgs e; Slab slab;
  const ReadListSpace by_events, by_entries;      // the reads by their events (the fill) and by their entries (the chain)
  const size_t o_xs, o_site;
  const double* site_pi = nullptr; double pi0 = 0.0; int share_stride = 0; size_t o_share = 0;   // a prior entry's: prior()
  double* share = nullptr;                        // after bind(): per row share_stride words (NULL without a prior)

  // own_site: the caller asked for no per-row site, the slab holds it; chain: the entry runs a kernel over the reads by their entries
  ChainCall(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff, const double* score,
            int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows, bool own_site, bool chain = true)
      : host(prm->memspace == NMOD_MEM_HOST), stream((hipStream_t)prm->stream), nr((size_t)nreads), ns((size_t)nsites), nw((size_t)nrows),
        tot(host && nreads > 0 ? (size_t)roff[nreads] : 0), slab(host), by_events(slab, nr), by_entries(slab, chain ? nr : 0),
        o_xs(slab.take(nw * 16)), o_site(own_site ? slab.take(nw * 4) : 0) {
    rh_ent_args(e, nreads, cs, start, roff, score, nsites, key);
    e.hoff = hoff; e.nrows = nrows;
  }
  ChainCall(const ChainCall&) = delete;           // (the slab keeps the addresses of e's pointers)

  // a prior entry, before stage(): the shares of the sites (nsites words in the call's memspace), the share of a site whose word is a
  // NaN, the words a row (rh_fill_shares' stride)
  void prior(const double* sp, double pi, int stride) { site_pi = sp; pi0 = pi; share_stride = stride; o_share = slab.take(nw * 8 * (size_t)stride); }
  void stage() { rh_stage_reads(slab, e, tot); slab.in(e.hoff, (nr + 1) * 8); slab.in(site_pi, ns * 8); }
  // after the commit.  site: the caller's per-row site as the commit left it, NULL: the slab's
  void bind(int32_t* site) {
    e.xs = slab.at<double>(o_xs); e.site = site ? site : slab.at<int32_t>(o_site);
    if (share_stride) share = slab.at<double>(o_share);
  }
  hipError_t entries() {                          // the rows of the reads written: site, position and score
    const hipError_t err = e.nrows ? by_events.fill(slab, e.roff, e.nreads, num_cus, stream, e.w) : hipSuccess;
    if (e.nrows && err == hipSuccess) rh_fill_entries(e, num_cus, stream);
    if (e.nrows && err == hipSuccess && share_stride) rh_fill_shares(e, site_pi, pi0, share_stride, share, num_cus, stream);
    return err;
  }
  hipError_t lists(ReadLists& w) {                // entries(), then w: the reads by their entries, for a kernel under rh_launch
    const hipError_t err = entries();
    return err != hipSuccess ? err : by_entries.fill(slab, e.hoff, e.nreads, num_cus, stream, w, NMOD_HMM_WAVE_MAX);
  }
};

}  // namespace nmod
