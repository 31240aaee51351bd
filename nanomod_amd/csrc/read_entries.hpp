// What the entries that run a chain over the candidate sites of a read share (K19 nmod_read_sites_count / nmod_read_hmm in read_hmm.hip,
// K20 nmod_read_viterbi in read_viterbi.hip): the arguments of the kernel that counts and fills the ENTRIES of a read, their staging,
// the host call that enqueues the fill (the kernel itself is read_hmm.hip's, compiled once), the launch of the two forms of a kernel,
// and the range check of the options.  The scans stay with each translation unit.
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

static bool rh_finite_in(double v, double lo, double hi) { return v >= lo && v <= hi; }   // (a NaN compares false)

}  // namespace nmod
