/* nanomod_hip.h — C ABI of the MI355X (gfx950) implementation of NanoMod's
 * per-base two-sample testing hot path.
 *
 * The reference (WGLab/NanoMod) has no FFI / plugin layer: its boundary for
 * this path is the Python function level of bin/scripts/myDetect.py
 * (SURVEY.md §8b).  Each entry point below names the reference lines it
 * replaces.  Plain pointers and sizes only; no exceptions cross the ABI; the
 * library never retains caller buffers.  Process-wide state it does keep, all
 * of it thread-safe and none of it result-affecting: per-device caches of the
 * CU count and of each kernel's occupancy (atomics, idempotent), and one HIP
 * memory pool per device, owned by the library, from which the scratch of the
 * large-position pass is allocated stream-ordered (freed slabs stay cached in
 * that pool until nmod_trim_scratch(); the device's default pool is not touched) — the NMOD_MEM_DEVICE entries that promise not
 * to synchronise keep the slab of a call parked under its (device, stream) for the next call on that stream instead of freeing it,
 * up to 2 slabs for each of up to 32 streams, a stream whose parked slabs are idle giving way to a new one (giving a reused block
 * back to a HIP pool while its previous free is still queued makes hipFreeAsync wait on the host; with 32 other streams all busy a
 * slab is freed that way all the same, and a call may then wait for the stream's previous call of the same scratch size) —
 * and the four tunables of nmod_host_pipeline_config (atomics; they change how a
 * host-resident batch is chunked and copied, never a result).  The library
 * reads no environment variable that changes which kernel runs: the choice
 * between kernel forms that produce the same numbers is per call
 * (NMOD_FLAG_NO_COUNTING / NMOD_FLAG_NO_COUNT_WIDE below).
 *
 * Data layout: the tested positions, in the
 * reference's iteration order (sorted (chrom,strand), then ascending
 * position, myDetect.py:421,427-431), are rows of two CSR arrays
 *     sig0[off0[i] .. off0[i+1])   samples of group 1 (--wrkBase1) at position i
 *     sig1[off1[i] .. off1[i+1])   samples of group 2 (--wrkBase2)
 * plus run_id[i]: equal ids <=> same chrom, same strand and consecutive
 * positions (restates pos_check, myDetect.py:366-371).
 * Samples are expected to be finite: NanoMod's normalised event means always
 * are.  The kernels order keys with bare v_min / v_max and pad with +inf, so a
 * position with a NaN or an infinite sample gets unspecified statistics (never
 * a fault, never another position's) — and NMOD_STATUS_NONFINITE: whenever the
 * Welch moments are computed (tests & NMOD_TEST_WELCH, or want_mstd: every call
 * the reference-shaped entry points make) a non-finite moment sets the bit at
 * no cost; NMOD_FLAG_CHECK_FINITE adds one pass over the samples that sets it
 * exactly in every mode (KS-only included).
 */
#ifndef NANOMOD_HIP_H
#define NANOMOD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NMOD_ABI_VERSION 4

/* sample dtype of sig0 / sig1 */
enum {
  NMOD_DTYPE_F32 = 0,       /* canonical: float32 (values up-cast exactly to the fp64 the reference sees) */
  NMOD_DTYPE_I16_MILLI = 1, /* int16 = round(norm_mean*1000): NanoMod's Events are 3-dp rounded
                               (myRefBaseSignalAnnotation.py:1108); value = k/1000.0 in fp64 */
  NMOD_DTYPE_F64 = 2        /* float64 as the reference holds it (lists of numpy.float64, myDetect.py:124).  The rank
                               statistics depend on the order of a position's samples only, so the library gives every
                               POSITION order- and tie-preserving float32 keys on the device: the samples themselves if all
                               of them are float32-exact, k if all are k/1000.0 with |k| <= 2^24 (NanoMod's 3-dp Events),
                               else their float32 roundings — monotone, so the only possible damage is a false tie between
                               two different doubles; the kernels report the positions whose keys tie and those (rare for
                               real-valued signals) are redone on the float64 samples with 64-bit keys (big_rank.hpp).  The
                               Welch moments always come from the float64 samples.  One extra pass over the samples, one
                               host round trip (the count of positions to redo).  ~3.5e8 positions/s KS-only, 2e8 with all
                               tests at 200 v 200; a batch made of doubles with exact ties that are neither float32-exact
                               nor on the 0.001 grid runs at the 64-bit-key rate, ~4e7 positions/s. */
};

/* where the caller's buffers live */
enum { NMOD_MEM_HOST = 0, NMOD_MEM_DEVICE = 1 };

/* --testMethod (NanoMod.py:359; consumed at myDetect.py:392,395,443) */
enum { NMOD_METHOD_KS = 0, NMOD_METHOD_STOUFFER = 1, NMOD_METHOD_FISHER = 2 };

/* which per-position tests to compute.  The reference always computes all
 * three (myDetect.py:331-343); the mask exists for the KS+combine benchmark
 * configuration of BASELINE.json. */
enum { NMOD_TEST_KS = 1, NMOD_TEST_MWU = 2, NMOD_TEST_WELCH = 4, NMOD_TEST_ALL = 7 };

/* per-position status bits (data-dependent conditions that make the
 * reference raise or return NaN; reported instead of aborting) */
enum {
  NMOD_STATUS_MWU_ALL_IDENTICAL = 1, /* scipy 1.2.1 mannwhitneyu raises ValueError (T == 0), uncaught at myDetect.py:331 */
  NMOD_STATUS_T_NAN = 2,             /* zero variance in both groups: ttest_ind returns (nan, nan), myDetect.py:335 */
  NMOD_STATUS_EMPTY = 4,             /* n0 == 0 or n1 == 0 (cannot occur after mfilter_coverage, myDetect.py:301-314) */
  NMOD_STATUS_TOO_LARGE = 8,         /* more samples in a group than the max_n0 / max_n1 the caller promised, or than NMOD_MAX_RANKED
                                        (NMOD_MAX_DEEP with NMOD_FLAG_DEEP):
                                        the position is skipped, its outputs are NaN, the rest of the batch is computed */
  NMOD_STATUS_NONFINITE = 16,        /* a NaN or infinite sample (see the header comment): the position's statistics are unspecified */
  NMOD_STATUS_BAD_REFERENCE = 32     /* nmod_one_sample only: the position's reference is unusable (mean or sd not finite, sd <= 0, ref_n < 2);
                                        no other entry point sets it */
};

/* return codes */
enum {
  NMOD_OK = 0,
  NMOD_ERR_INVALID_ARG = -1,
  NMOD_ERR_HIP = -2,          /* a HIP runtime call failed; see nmod_strerror */
  NMOD_ERR_TOO_LARGE = -3,    /* nmod_describe_dispatch / nmod_downsample_ks: a group beyond NMOD_MAX_RANKED (nmod_detect_batch reports
                                 such positions per position: NMOD_STATUS_TOO_LARGE) */
  NMOD_ERR_WORKSPACE = -4,    /* workspace missing or too small (device-memory mode) */
  NMOD_ERR_NO_DEVICE = -5
};

#define NMOD_MAX_GROUP 2048   /* largest group the wave-resident kernels sort (both groups in all-tests mode, the
                                 smaller one in KS-only mode); positions beyond it take the workgroup-per-position
                                 pass (big_rank.hpp), slower but unlimited up to NMOD_MAX_RANKED */
#define NMOD_MAX_RANKED 65535 /* max samples per group per position in any mode (16-bit ranks, 32-bit KS numerator); a position
                                 beyond it gets NMOD_STATUS_TOO_LARGE — unless NMOD_FLAG_DEEP is set */
#define NMOD_MAX_DEEP 16777215 /* 2^24 - 1: max samples per group with NMOD_FLAG_DEEP (deep_rank.hpp: n0 n1 < 2^48, so the KS
                                  numerator is exact in uint64 / fp64; twice the rank sum < 2^51, exact in fp64; the tie term
                                  sum (t^3 - t) < 2^75 is summed in 128 bits and rounded once) */
#define NMOD_MAX_NB 64        /* max --neighborPvalues */

typedef struct nmod_params {
  int32_t struct_size;    /* sizeof(nmod_params), for ABI evolution */
  int32_t device;         /* HIP device ordinal */
  void*   stream;         /* hipStream_t to launch on (NULL = default stream) */
  int32_t memspace;       /* NMOD_MEM_*: where sig/off/run_id/out pointers live */
  int32_t dtype;          /* NMOD_DTYPE_* */
  int32_t tests;          /* NMOD_TEST_* mask */
  int32_t method;         /* NMOD_METHOD_* */
  int32_t nb;             /* --neighborPvalues (NanoMod.py:357), window = 2*nb+1 */
  int32_t want_mstd;      /* --mstd: also mean / std (ddof=0) per group (myDetect.py:437-438) */
  double  weights_dif;    /* --WeightsDif (NanoMod.py:358; weights myDetect.py:396-400) */
  int64_t stride0;        /* >0: fixed-stride layout, off0 may be NULL: n0 = stride0 for every position */
  int64_t stride1;        /* >0: same for group 2 */
  int32_t max_n0;         /* upper bound of samples per position in group 1 (0 = unknown: the library
                             reduces off0 on the device and synchronises once to read it) */
  int32_t max_n1;         /* same for group 2 */
  void*   timer;          /* optional nmod_evtimer handle: HIP events are recorded around each kernel */
  int32_t flags;          /* NMOD_FLAG_* (0 = the reference's numbers bit for bit wherever it defines them) */
  int32_t reserved;       /* 0 */
} nmod_params;

/* tests == NMOD_TEST_KS only (a mode the reference never runs: getKStest always computes all three tests): report D as the
 * correctly rounded exact rational max|c0*n1 - c1*n0| / (n0*n1) instead of ks_2samp's float form max|fl(c0/n0) - fl(c1/n1)|
 * (they differ by <= 2 ulp, <= 4.5e-16 absolute; p-values agree to ~1e-15 relative).  Skips the pass that evaluates the float
 * form at the pooled points reaching the integer maximum (~10 % of the KS-only kernel).  Ignored with any other test in the mask. */
#define NMOD_FLAG_KS_RATIONAL_D 1
/* One extra pass over the samples (float32 / float64 input; ~0.2 ms per GB) that sets NMOD_STATUS_NONFINITE for every position
 * holding a NaN or an infinite sample, in every mode.  Without it the bit comes from the Welch moments alone (free, whenever they
 * are computed): that catches every NaN and -inf, and +inf except in the group a kernel form sorts with +inf pads. */
#define NMOD_FLAG_CHECK_FINITE 2
/* Kernel-form switches for A/B measurements and parity tests; the numbers are the same with and without them.  Event-like
 * rows (every sample on the milli-unit grid, a position's samples within a window of 2 048 milli-units apart from a few
 * outliers) are taken by counting forms of K1 instead of sorting forms when a device-side probe finds a size class of the
 * batch event-like.  NMOD_FLAG_NO_COUNTING keeps every position on the sorting forms;
 * NMOD_FLAG_NO_COUNT_WIDE only those outside the 256-capacity class. */
#define NMOD_FLAG_NO_COUNTING 4
#define NMOD_FLAG_NO_COUNT_WIDE 8
/* NMOD_MEM_HOST with NMOD_DTYPE_F64: the threads that fill the pinned bounce slots write a chunk as int16 milli-units where every
 * sample of it is k / 1000.0 with |k| <= 32 767 (what NanoMod's stored events are: myRefBaseSignalAnnotation.py:1108) — 2 bytes
 * per sample over PCIe instead of 8, the chunk then runs as NMOD_DTYPE_I16_MILLI; any other chunk is sent as float64.  The rank
 * statistics are the same bit for bit, the Welch moments come from exact integer sums instead of the two-pass float64 sums
 * (both within 1e-11 of the reference's t).  This flag sends every chunk as float64 (A/B, parity tests). */
#define NMOD_FLAG_NO_HOST_NARROW 16
/* Deep coverage (amplicon / plasmid runs: NanoMod's own examples put more than 65 535 reads on a base, and the reference tests
 * whatever it is given): a position with a group beyond NMOD_MAX_RANKED, both groups within NMOD_MAX_DEEP, is computed in every
 * mode (all tests, KS-only, NMOD_FLAG_KS_RATIONAL_D, want_mstd; every dtype — float64 samples are sorted as 64-bit keys; CSR or
 * fixed stride; both memspaces; nmod_downsample_ks) by the multi-workgroup deep form (deep_rank.hpp) instead
 * of being skipped with NMOD_STATUS_TOO_LARGE.  Its scratch comes from the library's pool (rounds of at most 2^27 keys; the
 * workspace size does not change); the host round trip is the one the large-position pass makes.  Without the flag a position
 * beyond NMOD_MAX_RANKED is NMOD_STATUS_TOO_LARGE as before; beyond NMOD_MAX_DEEP it is with the flag too. */
#define NMOD_FLAG_DEEP 32
/* Kernel-form switch for A/B measurements and parity tests; the numbers are the same bit for bit with and without it.  The
 * persistent waves of the KS-only K1 kernel take a fixed, strided part of their items and draw the rest in small chunks from a
 * per-launch counter, so that the waves of a launch end together (DESIGN_NOTES.md A.10).  With this flag every wave walks its
 * equal, strided share as before (no counter, no atomic). */
#define NMOD_FLAG_K1_STATIC_ITEMS 128

/* Caller-allocated SoA outputs, npos elements each; a NULL member is skipped.
 * One (stat, p) pair per test = the tuples getKStest returns
 * (myDetect.py:363) after the m_min_float / m_max_float clamps (:317-325),
 * then the combined pair appended by combin_pvalues (:373-377,403-406). */
typedef struct nmod_out {
  double* mwu_u;   double* mwu_p;     /* myDetect.py:331-333 */
  double* t_t;     double* t_p;       /* myDetect.py:335-337 */
  double* ks_d;    double* ks_p;      /* myDetect.py:341-343 */
  double* comb_st; double* comb_p;    /* myDetect.py:379-414 (not written when method == KS) */
  double* mean0;   double* std0;      /* myDetect.py:438 (want_mstd) */
  double* mean1;   double* std1;
  uint8_t* status;
} nmod_out;

int nmod_abi_version(void);
int nmod_device_count(void);                 /* number of HIP devices (0 if none) */
const char* nmod_strerror(int rc);

/* How a K1 launch of `items` work items on `waves` resident waves hands its items out (host arithmetic only, no device needed):
 * plan[0] = strided rounds r — wave w takes items w + k * waves, k < r; plan[1] = first item handed out by chunk (r * waves);
 * plan[2] = items per chunk c — chunk j holds items plan[1] + j * c .. + c - 1 (those below `items`), chunk w belongs to wave
 * w and chunk waves + t to the wave that draws ticket t from the launch's counter; plan[3] = 1 when such tickets are drawn at
 * all.  flags: NMOD_FLAG_K1_STATIC_ITEMS gives the plan of the strided walk (r = ceil(items / waves), nothing left to claim). */
int nmod_item_claim_plan(int64_t items, int64_t waves, int32_t flags, int64_t* plan);

/* Device scratch needed by nmod_detect_batch for `npos` positions (bytes). */
int64_t nmod_workspace_bytes(const nmod_params* prm, int64_t npos);

/* Replaces the two hot loops of mtest2 (myDetect.py:427-436 per-position
 * getKStest, :443 combin_pvalues).  NMOD_MEM_DEVICE: all pointers are device
 * pointers, `workspace` must hold nmod_workspace_bytes(), everything is
 * enqueued on prm->stream and the call returns without synchronising — except
 * for one host round trip each when (i) max_n0 / max_n1 are unknown for CSR
 * inputs, (ii) the maxima allow groups beyond NMOD_MAX_GROUP (the scratch of the
 * large-position pass is sized from the classifier's totals and allocated
 * stream-ordered), (iii) dtype is NMOD_DTYPE_F64 (the probe's verdict).
 * NMOD_MEM_HOST (what a drop-in mtest2 hands over: everything on this path is host
 * memory in the reference, myDetect.py:416-445): pointers are host memory, workspace
 * may be NULL, prm->stream is not used and the call returns after the results are
 * back.  The batch is cut into chunks of positions that go through pinned bounce
 * slots (skipped for arrays that are already page-locked) and three library-owned
 * streams: the H2D copy of chunk k+1, K1 + K2 of chunk k and the D2H copy of chunk
 * k-1 overlap; the KS track stays on the device and ONE K3 runs over the whole
 * batch at the end, so chunk cuts never change a window.  Device footprint:
 * slots x (chunk + workspace + results) + 36 B per position, from the library's
 * pool; the pinned ring and the streams are cached per device until
 * nmod_trim_scratch().  See nmod_host_pipeline_config / nmod_last_host_stats. */
int nmod_detect_batch(const nmod_params* prm, int64_t npos,
                      const void* sig0, const int64_t* off0,
                      const void* sig1, const int64_t* off1,
                      const int32_t* run_id,
                      void* workspace, int64_t workspace_bytes,
                      nmod_out* out);

/* Tunables of the NMOD_MEM_HOST pipeline, process-wide; 0 keeps / restores the default.  chunk_bytes: sample bytes per
 * chunk (default min(64 MiB, batch / 32), at least 1 MiB; env NMOD_HOST_CHUNK_BYTES); slots: ring depth 2..8 (default 3; env
 * NMOD_HOST_SLOTS); threads: host threads filling a bounce slot (default 4, capped by the cgroup CPU quota; env
 * NMOD_HOST_THREADS); mode: 0 = copy straight from arrays that are page-locked, bounce the rest; 2 = always bounce. */
int nmod_host_pipeline_config(int64_t chunk_bytes, int32_t slots, int32_t threads, int32_t mode);

/* What the calling thread's last NMOD_MEM_HOST nmod_detect_batch did. */
typedef struct nmod_host_stats {
  int64_t chunks;            /* chunks the batch was cut into */
  int64_t slots;             /* ring depth used */
  int64_t copy_threads;      /* host threads that filled the bounce slots (1 when the input was page-locked) */
  int64_t pinned_input;      /* 1: sig0 / sig1 were page-locked and copied from where they are */
  int64_t chunk_positions;   /* positions of the largest chunk */
  int64_t device_bytes;      /* device memory held during the call (ring + per-batch tracks) */
  int64_t pinned_bytes;      /* pinned host ring */
  int64_t h2d_bytes;         /* bytes copied host -> device */
  int64_t d2h_bytes;         /* bytes copied device -> host */
  int64_t narrowed_chunks;   /* NMOD_DTYPE_F64: chunks sent as int16 milli-units (see NMOD_FLAG_NO_HOST_NARROW) */
} nmod_host_stats;
int nmod_last_host_stats(nmod_host_stats* st);

/* Which K1 form computed the positions of the last successful nmod_detect_batch of the calling thread; a failed call clears
 * it (nmod_downsample_ks leaves it alone, an empty batch reports no positions).  The forms produce the same numbers
 * (tests/test_gpu_parity.py runs batches through both and compares); which one runs is decided on the device — size classes,
 * and for the counting forms a probe per class plus a per-position check — so the split is a property of the data the caller
 * can only learn here.  NMOD_MEM_DEVICE: the counters are reduced on request from facts the call left in `workspace` (one
 * small kernel on the call's stream, one synchronisation): ask before the workspace is reused or freed.  NMOD_MEM_HOST: they
 * were read back with the results.  NMOD_ERR_INVALID_ARG when there is no such call. */
typedef struct nmod_dispatch_stats {
  int64_t positions;        /* positions of the batch */
  int64_t ks_rank;          /* ks_rank_kernel: KS only, the smaller group sorted */
  int64_t rank_hist;        /* rank_hist_kernel: all tests, both groups sorted (groups of similar size) */
  int64_t rank_hist_wide;   /* rank_hist_kernel, WIDE form: the smaller group sorted, the larger one streamed */
  int64_t rank_pair;        /* rank_pair_kernel: all tests, both groups beyond 256 samples and of different capacity */
  int64_t rank_count;       /* rank_count_kernel: the counting form of the 256-capacity class (event-like rows) */
  int64_t rank_count_wide;  /* rank_count_wide_kernel: the counting form for any coverage (event-like rows); rank_count_value_kernel's too */
  int64_t big;              /* big_rank_kernel / big_hist_kernel: a group beyond NMOD_MAX_GROUP */
  int64_t skipped;          /* no K1 form (NMOD_STATUS_EMPTY / NMOD_STATUS_TOO_LARGE) */
  int64_t count_tried;      /* positions of the classes whose probe let a counting form run */
  int64_t count_rejected;   /* ... that the counting form handed on to the class's sorting form (counted there above) */
  int64_t f64_redo;         /* NMOD_DTYPE_F64: positions done again on 64-bit keys (their first form counts them as well) */
  int64_t deep;             /* the deep form (NMOD_FLAG_DEEP): a group beyond NMOD_MAX_RANKED */
  int64_t reserved[3];
} nmod_dispatch_stats;
int nmod_last_dispatch_stats(nmod_dispatch_stats* st);

/* "arch=gfx950 abi=4 hip=M.m": the target, the ABI version and the HIP version (major.minor) this binary was built with. */
const char* nmod_build_info(void);

/* KS statistic: ks_d is ks_2samp's own float form max|fl(c0/n0) - fl(c1/n1)| bit for bit in every mode (myDetect.py:341 ->
 * scipy 1.2.1), tests == NMOD_TEST_KS included: the kernels find the exact integer maximum of |c0*n1 - c1*n0| and evaluate the
 * float form for the pooled points that reach it. */

/* Name of the K1 kernel instance a position with n0 / n1 samples is dispatched to under prm's dtype / tests / method
 * (e.g. "ks_rank_kernel<16,16,f32>"), from the same size-class functions the dispatcher uses: what bench.py prints as
 * roofline.kernel and what the rocprofv3 kernel trace shows.  No device work.  A group beyond NMOD_MAX_RANKED:
 * NMOD_ERR_TOO_LARGE, or with NMOD_FLAG_DEEP and both groups within NMOD_MAX_DEEP "deep_rank_kernel<f32|i16|f64>". */
int nmod_describe_dispatch(const nmod_params* prm, int64_t n0, int64_t n1, char* buf, int32_t buflen);

/* Returns the slabs cached in the library's scratch pool of `device` to the driver (see the header comment), those parked per stream
 * included, and frees the pinned ring + streams the NMOD_MEM_HOST pipeline caches for it.  Synchronises the device when a slab is
 * parked, and returns once the parked bytes show as free in hipMemGetInfo (it waits at most 0.1 s for that): call it when no other
 * thread has work of the library in flight on the device. */
int nmod_trim_scratch(int32_t device);

/* Replaces combin_pvalues / get_combin_pvalue on a whole KS track
 * (myDetect.py:373-414).  ks_d is only read when nb == 0 (:413).
 * Conventions (the reference's, through numpy's IEEE arithmetic; pinned by tests/test_tails_gpu.py):
 *   - a neighbour outside the track or in another run (run_id differs) is a pad, p = 1: a Stouffer window that touches a pad is
 *     (Z, p) = (-inf, 1.0) exactly; to a Fisher window a pad contributes nothing;
 *   - a NaN p makes (NaN, NaN) of exactly the windows of its own run that contain it;
 *   - p = 0 gives (DBL_MAX, DBL_MIN) (m_max_float / m_min_float of (+inf, 0)); in a Stouffer window that also holds a pad or a
 *     p = 1 the sum is (+inf) + (-inf): (NaN, NaN);
 *   - comb_p is clamped to DBL_MIN from below, comb_st to DBL_MAX from above. */
int nmod_combine_track(const nmod_params* prm, int64_t npos,
                       const double* ks_d, const double* ks_p, const int32_t* run_id,
                       double* comb_st, double* comb_p);

/* Replaces the down-sampling branch of getKStest (myDetect.py:345-361; taken when --coverages > 0 and a group exceeds the
 * threshold) for `nflag` positions of a HOST-resident CSR batch (prm->memspace == NMOD_MEM_HOST): `iters` (--downsampling, 100)
 * times, a group of position positions[i] with more than cov[i] samples is resampled WITH replacement to cov[i] samples
 * (np.random.choice(x, cov)), KS runs on each resample, and the (D, p) pair at index int(iters * quantile)
 * (--downsampling_quantile, 0.25) of the p-sorted resamples is written to ks_d[i] / ks_p[i].  The reference draws from numpy's
 * unseeded global generator; here the draws are a counter-based function of (seed, i, iteration, group, draw) on the device —
 * reproducible, statistically equivalent, not bit-comparable (SURVEY.md 8a row A3').  The resampled rows are materialised in
 * HBM chunk by chunk (2^27 samples) and go through the same KS kernel as everything else.  Groups (and cov) beyond
 * NMOD_MAX_RANKED need NMOD_FLAG_DEEP in prm->flags (NMOD_ERR_TOO_LARGE otherwise); the flag is passed on to the KS batch.  Synchronises. */
int nmod_downsample_ks(const nmod_params* prm, int64_t nflag, const void* sig0, const int64_t* off0, const void* sig1, const int64_t* off1,
                       const int64_t* positions, const int64_t* cov, int32_t iters, double quantile, uint64_t seed,
                       double* ks_d, double* ks_p);

/* Benchmark input generator (no reference counterpart).
 * Counter-based and integer-only, so tests restate it bit-exactly on the CPU:
 *   h = mix64(seed, group, pos, read);  s = sum of the four 16-bit fields of h;
 *   x = float(s - 131070) * (1/37837.2f)  [ + shift  at planted positions of group 1 ]
 * Fills sig[(pos - pos_begin) * n_per_pos + read] for pos in [pos_begin, pos_begin+npos).
 * A position is planted iff plant_period > 0 and (pos % plant_period) is 0, 1 or plant_period-1. */
int nmod_synth_fill(const nmod_params* prm, uint64_t seed, int64_t pos_begin, int64_t npos,
                    int32_t group, int32_t n_per_pos, int64_t plant_period, float plant_shift,
                    void* sig_out);

/* The same generator for ragged rows (BASELINE.json configs[4]): sample `read` of position pos_begin + i goes to
 * sig_out[off[i] + read], read < off[i+1] - off[i]; `off` is a DEVICE array of npos + 1 element offsets into sig_out.
 * float32 or int16 milli-unit output (prm->dtype). */
int nmod_synth_fill_csr(const nmod_params* prm, uint64_t seed, int64_t pos_begin, int64_t npos,
                        int32_t group, const int64_t* off, int64_t plant_period, float plant_shift,
                        void* sig_out);

/* Synthetic EVENT rows the way NanoMod stores them (benchmark input, no reference counterpart): every position has a signal
 * LEVEL shared by both groups (+-3 normalised units: the k-mer under the pore) and each read spreads around it with standard
 * deviation spread_milli / 1000 units; values sit on the 3-decimal grid (myRefBaseSignalAnnotation.py:1108 rounds norm_mean to
 * 3 decimals), so most of a position's samples tie with another one — the unit-variance rows of nmod_synth_fill tie ~11 times
 * per 200 v 200 position.  Integer-only up to the last quotient, so tests restate it bit for bit:
 *   level(pos) = (mix64(seed ^ 0xA5A5A5A5DEADBEEF, pos, 0, 0) >> 40) % 6001 - 3000                          [milli-units]
 *   z = (sum of the four 16-bit fields of mix64(seed, group, pos, read)) - 131070     (as nmod_synth_fill; sd 37837.2)
 *   k = level + floor((2 z spread_milli + 37837) / 75674)  [+ plant_shift_milli at planted positions of group 1]
 *   o = mix64(seed ^ 0x0DDBA11C0FFEE123, group, pos, read);  if ((o >> 20) % 1000 < outlier_permille) k = (o >> 32) % 10001 - 5000
 *       (a mis-segmented event: uniform over the +-5 unit clip range of the raw normalisation, myRefBaseSignalAnnotation.py:251-259)
 *   |k| <= 32767
 * int16 output: k.  float32 output: (float)((double)k / 1000.0), the float32 image of the stored 3-decimal value.
 * Rows: n_per_pos > 0 fixed stride (off ignored), else `off` = DEVICE array of npos + 1 element offsets into sig_out.
 * 0 <= spread_milli <= 8000, 0 <= outlier_permille <= 1000. */
int nmod_synth_fill_events(const nmod_params* prm, uint64_t seed, int64_t pos_begin, int64_t npos,
                           int32_t group, int32_t n_per_pos, const int64_t* off, int64_t plant_period,
                           int32_t plant_shift_milli, int32_t spread_milli, int32_t outlier_permille, void* sig_out);

/* HIP-event timer: records (start, stop) around every kernel the library
 * launches while prm->timer points to it; read it after synchronising. */
enum { NMOD_KERNEL_RANK_STATS = 0, NMOD_KERNEL_FINALIZE = 1, NMOD_KERNEL_COMBINE = 2,
       NMOD_KERNEL_SYNTH = 3, NMOD_KERNEL_COUNT = 4 };
int nmod_evtimer_create(int32_t capacity_per_kernel, void** timer);
int nmod_evtimer_reset(void* timer);
int nmod_evtimer_read(void* timer, int32_t kernel, double* total_ms, int32_t* launches);
int nmod_evtimer_destroy(void* timer);

/* Replaces save_test's table loop (myDetect.py:522-538) for array-shaped results: writes one line per
 * position, '%s %s %d %s %d %d %.3f %.3E %.3f %.3E %.3f %.3E' = chrom strand pos+1 base n0 n1 U pU t pt D pKS,
 * then ' %.3f %.3E' with the combined pair iff with_comb, then '\n'; non-finite values print as Python
 * prints them ('inf', '-inf', 'nan').  Host-only (no device work).  chrom_id[i] indexes chrom_names
 * (NUL-separated, n_chroms entries); strand[i] and base[i] are single characters.  Returns NMOD_OK or
 * NMOD_ERR_INVALID_ARG (also when the file cannot be opened). */
int nmod_write_sign_test(const char* path, int64_t npos, const int32_t* chrom_id, const char* chrom_names,
                         int32_t n_chroms, const char* strand, const int64_t* pos0, const char* base,
                         const int32_t* n0, const int32_t* n1, const double* mwu_u, const double* mwu_p,
                         const double* t_t, const double* t_p, const double* ks_d, const double* ks_p,
                         const double* comb_st, const double* comb_p, int32_t with_comb);

/* Test hook for the float64 -> int16 narrowing of the host-resident entry: out[i] = k where v[i] == k / 1000.0 with |k| <= 32 767;
 * returns 1 when every one of the n values narrowed, 0 when one refused (out is then unspecified), negative on bad arguments.
 * Host-only. */
int nmod_narrow_probe(const double* v, int64_t n, int16_t* out);

/* Test hook for the table writer's number formats: v[i] formatted as '%.3f' (sci = 0) or '%.3E' (sci = 1) the way
 * nmod_write_sign_test does, NUL-separated, into out (capacity cap bytes; at most 420 bytes per value). */
int nmod_format_probe(const double* v, int64_t n, int32_t sci, char* out, int64_t cap);

/* Replaces the ranking of the result records (myDetect.py:447-462): order_out[i] = index of the i-th record of
 * sorted(records, key = (key_primary, key_second, key_third)) — Python's stable tuple sort, ascending, -0.0 tied
 * with 0.0, NaN last — reversed as a whole when `descending` (rankUse == 'st': the reference reverses the sorted
 * list).  The reference's keys are (combined p, KS p, MWU p) or the three statistics.  Device radix sort (radix_sort.hpp),
 * three stable passes; synchronises before returning. */
int nmod_rank_order(const nmod_params* prm, int64_t npos, const double* key_primary, const double* key_second,
                    const double* key_third, int32_t descending, int32_t* order_out);

/* The stable ascending order of n signed 64-bit keys: order_out[i] = index of the i-th smallest key, equal keys in index
 * order (what numpy.argsort(kind='stable') returns).  keys / order_out: host or device memory by prm->memspace.  Behind the
 * grouping of events by (chrom, strand, position) that replaces getGenomeEvents' dict inserts for the simulation loops
 * (mySimulat2.py:127-171; nanomod_amd/simulate.py).  Synchronises before returning. */
int nmod_argsort_keys(const nmod_params* prm, int64_t n, const int64_t* keys, int32_t* order_out);

/* Replaces the window ranking of --RegionRankbyST 1 (myDetect.py:463-515) on array-shaped records in the
 * reference's record order (sorted (chrom, strand), ascending position).  strand_lo[i] / strand_hi[i]: index of the
 * first / last record of record i's (chrom, strand); value[i]: the p-value or statistic the ranking uses
 * (record[sorted_ind][use_pind]); w: the window half-width AFTER the reference's in-place increment (window + 1);
 * movesize: 1 when WindOvlp == 1, else w; na: base filter ('\0' = none); percentile: which of a window's sorted contributing
 * values is its key, 0 <= percentile <= 1 (anything else, NaN included, is NMOD_ERR_INVALID_ARG).  A window holding a NaN value
 * has no defined rank.  Writes the indices of the ranked window
 * centres to ranked_out (capacity npos) and their number to *n_ranked.  Host memory only; synchronises. */
int nmod_region_rank(const nmod_params* prm, int64_t npos, const int32_t* strand_lo, const int32_t* strand_hi,
                     const int64_t* pos, const char* base, const double* value, int32_t w, int32_t movesize,
                     char na, double percentile, int32_t wind_ovlp, int32_t* ranked_out, int64_t* n_ranked);

/* Multiple-testing correction of whole p-value tracks on the device: Benjamini-Hochberg or Benjamini-Yekutieli adjusted
 * p-values (q-values), one family per track, each of the `ntracks` (1..8) tracks on its own.  The reference has no such step;
 * the definition is that of scipy.stats.false_discovery_control on the VALID elements of a track, where an element is valid iff
 * 0 <= p <= 1 (so NaN — the p-values of positions flagged TOO_LARGE / T_NAN / NONFINITE — is not): with m valid elements
 * p_(1) <= ... <= p_(m), a_i = fl(p_(i) * fl(m / i)), for BY a_i = fl(a_i * c_m) with c_m = sum_{k<=m} 1/k, and
 * q_(i) = min(1, min_{j>=i} a_j), written at the element's own index; an invalid element gets q = NaN and takes no part.
 * BH is bit-equal to scipy 1.15; BY is within 1e-14 relative (c_m is summed differently).  summary[t] (may be NULL): tested = m,
 * excluded = n - m, rejected = #{q <= alpha}, p_crit = the largest valid p whose q <= alpha (NaN when nothing is rejected).
 * Reads struct_size, device, stream and memspace of prm and nothing else.  The arrays `p` and `q_out` themselves are host
 * memory; the tracks they point to and `summary` live where prm->memspace says; q_out[t] == p[t] (in place) is allowed.
 * NMOD_MEM_DEVICE: everything is enqueued on prm->stream and the call returns WITHOUT synchronising (m, c_m and the summary
 * stay on the device), so it can follow a detect call in a pipeline; scratch (about 24 bytes per element, tracks one after
 * another) comes stream-ordered from the library's pool.  NMOD_MEM_HOST: copy in, run, copy back, synchronise.  n == 0 is
 * NMOD_OK (summaries: zero counts, p_crit NaN).  NMOD_ERR_INVALID_ARG before any device work: n < 0 or n > 2^31 - 2, ntracks
 * outside 1..8, a NULL track, an unknown method, alpha outside (0, 1]. */
enum { NMOD_FDR_BH = 0, NMOD_FDR_BY = 1 };
typedef struct nmod_fdr_summary { int64_t tested, excluded, rejected; double p_crit; } nmod_fdr_summary;
int nmod_fdr_adjust(const nmod_params* prm, int64_t n, int32_t ntracks, const double* const* p,
                    int32_t method, double alpha, double* const* q_out, nmod_fdr_summary* summary /* ntracks, may be NULL */);

/* Per-position modified fraction: a two-component normal mixture fitted by EM on the device (K8; the reference has no such step —
 * its simulations mix modified and unmodified reads at known shares, mySimulate.py --Percentages).  One group is the reference
 * ("unmodified") group R, the other the mixed group Y: mix_group 0 = sig0 is mixed, 1 = sig1 is.  Samples as doubles (float32
 * up-cast, int16 k / 1000.0, float64 as is).  Per position mu = mean(R), s2 = var(R) (ddof = 0), s = sqrt(s2), n = |Y|,
 * d = mean(Y) - mu, and the model y ~ (1 - pi) N(mu, s2) + pi N(m, v) with v == s2 (NMOD_MIX_EQUAL_VAR) or v free and floored at
 * s2 / 16 (NMOD_MIX_FREE_VAR).  Start pi = 0.5, m = mu + 2 d, v = s2; iteration k = 1, 2, ...:
 *   t_i = ln((1 - pi) / pi) + 1/2 ln(v / s2) + (y_i - m)^2 / (2 v) - (y_i - mu)^2 / (2 s2)        r_i = 1 / (1 + exp(t_i))
 *   W = sum r_i,  pi' = W / n,  m' = sum r_i y_i / W,  free model: v' = max(sum r_i (y_i - m')^2 / W, s2 / 16)
 *   delta = max(|pi' - pi|, |m' - m| / s [, |sqrt(v') - sqrt(v)| / s]);  take the primed values
 * and stop when delta <= tol (tol > 0) or k == max_iter (1 .. 10 000); tol == 0 never stops early.  With the final parameters and
 * one more evaluation of t_i: llr = 2 sum_i [ln(1 - pi) + softplus(-t_i)], twice the log-likelihood gain over "all of Y is
 * unmodified", and resp = r_i per read.  llr is a SCORE: the null pi = 0 lies on the boundary of the parameter space with m
 * unidentified, so no chi-square law applies and no p-value is attached.
 * Outputs, npos elements each, a NULL member skipped: pi, mu_mod (= m), sd_mod (= sqrt v), llr, iters (iterations run), status
 * (NMOD_MIX_* bits below); resp (optional): float32 in the mixed group's own sample layout (its CSR offsets or stride).
 *   NMOD_MIX_NOT_CONVERGED  max_iter iterations ran and the last delta was above tol; the estimates are written
 *   NMOD_MIX_DEGENERATE     |R| < 2, |Y| < 2, s2 == 0 (every sample of R equal), a non-finite sample, or W underflowed to 0: NaN outputs, iters 0, NaN resp
 *   NMOD_MIX_SKIPPED        the gate left the position out: NaN outputs and resp
 *   NMOD_MIX_VAR_FLOORED    the variance floor was active in the last iteration
 *   NMOD_MIX_TOO_LARGE      a group beyond NMOD_MAX_DEEP: NaN outputs and resp
 * Gate: gate (npos doubles, may be NULL = every position) and gate_max: position i is computed iff gate[i] <= gate_max (NaN
 * compares false) — typically gate = the q track of nmod_fdr_adjust and gate_max = alpha, on the same stream, no host round trip.
 * Reads struct_size, device, stream, memspace, dtype, stride0 / stride1 of prm and nothing else; a group is CSR when its offsets
 * are given, else fixed stride.  NMOD_MEM_DEVICE: everything is enqueued on prm->stream and the call returns WITHOUT
 * synchronising; scratch (12 bytes per position) comes stream-ordered from the library's pool.  NMOD_MEM_HOST: copy in, run, copy
 * back, synchronise (one staged copy, not the pipelined host entry).  npos == 0 is NMOD_OK.  NMOD_ERR_INVALID_ARG before any
 * device work: mix_group not 0 / 1, an unknown model, max_iter outside 1 .. 10 000, tol negative or not finite, npos < 0 or
 * beyond 2^32 - 2, out NULL, a NULL signal array with npos > 0, a group with neither offsets nor a stride, an unknown dtype,
 * host offsets that decrease.  A position's results are the same bits whatever else is in the batch, in CSR or stride form. */
enum { NMOD_MIX_EQUAL_VAR = 0, NMOD_MIX_FREE_VAR = 1 };
enum { NMOD_MIX_NOT_CONVERGED = 1, NMOD_MIX_DEGENERATE = 2, NMOD_MIX_SKIPPED = 4, NMOD_MIX_VAR_FLOORED = 8, NMOD_MIX_TOO_LARGE = 16 };
typedef struct nmod_mix_out { double *pi, *mu_mod, *sd_mod, *llr; int32_t* iters; uint8_t* status; float* resp; } nmod_mix_out;
int nmod_mix_fraction(const nmod_params* prm, int64_t npos, const void* sig0, const int64_t* off0, const void* sig1, const int64_t* off1,
                      int32_t mix_group, int32_t model, int32_t max_iter, double tol,
                      const double* gate, double gate_max, const nmod_mix_out* out);

/* One-sample detection against a stored per-position reference (K9; the reference project has no such step — it always needs two
 * read groups).  Position i has the samples x_1..x_n of ONE group (as doubles: float32 up-cast, int16 k / 1000.0, float64 as is), a
 * reference level mu = ref_mean[i] and spread sd = ref_sd[i] (the ddof = 0 standard deviation, what want_mstd reports) and
 * optionally the reference's coverage nr = ref_n[i].
 *   Moments: m = mean(x), s2 = var(x) with ddof = 0 (two-pass fp64 about the mean; int16: in milli-units, the first sum exact),
 *     shift = (m - mu) / sd; outputs mean = m, std = sqrt(s2).
 *   KS against N(mu, sd^2): x_(1) <= ... <= x_(n) sorted, F_k = 0.5 erfc(-(x_(k) - mu) / (sd sqrt 2)),
 *     D = max_k max(k/n - F_k, F_k - (k-1)/n)  (ties need no special case: the largest k of a tie group attains the upper term,
 *     the smallest the lower one), ks_p = kolmogorov((sqrt n + 0.12 + 0.11 / sqrt n) D): the Stephens-corrected asymptotic tail,
 *     the one-sample form of what ks_2samp does with en = sqrt(n0 n1 / (n0 + n1)), by the same device function.  D within 1e-13
 *     absolute of the definition in exact arithmetic, ks_p within 1e-9 relative; both clamped as nmod_detect_batch clamps its pair.
 *   t, sign sample minus reference, clamped as the two-sample pair:
 *     ref_n given (a stored control): Welch from the statistics, vx = s2 n / (n - 1), vr = sd^2 nr / (nr - 1),
 *       se2 = vx / n + vr / nr, t = (m - mu) / sqrt(se2), df = se2^2 / ((vx/n)^2 / (n - 1) + (vr/nr)^2 / (nr - 1)) —
 *       scipy.stats.ttest_ind_from_stats(equal_var=False), so the t of the two-sample Welch test on the full data (1e-11 relative);
 *     ref_n == NULL (a model: the reference is taken as known): t = (m - mu) / sqrt(vx / n), df = n - 1 — scipy.stats.ttest_1samp;
 *     se2 == 0 (vx == 0 for a model) or n == 1: t and t_p are NaN with NMOD_STATUS_T_NAN (KS is computed).
 *   Combine: comb_st / comb_p are the window combine of this KS track under prm->nb / method / weights_dif and run_id — the code
 *     behind nmod_combine_track with all its pad / NaN / p = 0 conventions; not written when method == NMOD_METHOD_KS.
 *   Status per position: NMOD_STATUS_EMPTY (n == 0), NMOD_STATUS_TOO_LARGE (n beyond NMOD_MAX_ONE, NMOD_MAX_ONE_F64 for float64),
 *     NMOD_STATUS_BAD_REFERENCE, NMOD_STATUS_NONFINITE (a NaN or infinite sample; exact here: the kernels see every sample) — each
 *     of these four gives NaN in every output of the position, and its combine windows follow K3's NaN rule — and NMOD_STATUS_T_NAN.
 *     Deeper positions (the NMOD_FLAG_DEEP range) are not computed by this entry.
 * A NULL output member is skipped; out->struct_size = sizeof(nmod_one_out).  Rows: CSR when `off` is given, else the fixed stride
 * prm->stride0.  Reads struct_size, device, stream, memspace, dtype, stride0, nb, method, weights_dif of prm and nothing else.
 * NMOD_MEM_DEVICE: everything is enqueued on prm->stream and the call returns WITHOUT synchronising and without a host round trip;
 * scratch (16 bytes per position, 16 more when the combined pair is wanted without the KS pair) comes stream-ordered from the
 * library's pool.  NMOD_MEM_HOST: copy in, run, copy back, synchronise (one staged copy, not the pipelined host entry).  npos == 0
 * is NMOD_OK.  NMOD_ERR_INVALID_ARG before any device work: npos < 0 or beyond 2^32 - 2, out NULL (or of another struct_size), a
 * NULL sig / ref_mean / ref_sd with npos > 0, neither offsets nor a stride, an unknown dtype, nb outside 0 .. NMOD_MAX_NB, an
 * unknown method, host offsets that decrease, a NULL run_id (or a Stouffer weights_dif <= 0) when a combined track is requested.
 * A position's results are the same bits whatever else is in the batch, in CSR or stride form, from host or device memory. */
#define NMOD_MAX_ONE 16384      /* samples per position, float32 / int16: 64 KiB of keys in one workgroup's LDS */
#define NMOD_MAX_ONE_F64 8192   /* samples per position, float64 (64-bit keys) */
typedef struct nmod_one_out { int32_t struct_size; int32_t reserved;
  double *ks_d, *ks_p, *t_t, *t_p, *shift, *mean, *std, *comb_st, *comb_p; uint8_t* status; } nmod_one_out;
int nmod_one_sample(const nmod_params* prm, int64_t npos, const void* sig, const int64_t* off /* or prm->stride0 */,
                    const double* ref_mean, const double* ref_sd, const int32_t* ref_n /* may be NULL */,
                    const int32_t* run_id, const nmod_one_out* out);

/* K-mer level models from a control run (K10; the reference project has no such step).  The table nmod_one_sample's "model" kind of
 * reference comes from: every position of a read group carries the code of the k-mer it sits in (nanomod_amd.kmermodel.kmer_codes),
 * and the samples of all positions of a code are pooled into that code's level and spread.
 *   Position i belongs to code c = code[i].  Its samples are taken as doubles: float32 up-cast, int16 as k / 1000.0 (a division,
 *     as K9 does), float64 as is.
 *   A sample x of a position of code c is KEPT iff keep_lo[c] <= x && x <= keep_hi[c].  The bounds are inclusive; a NaN bound keeps
 *     nothing; without bounds (both NULL) everything is kept.
 *   A position is dropped whole, and flagged in pos_status, when it has
 *     NMOD_STATUS_NO_CODE     code[i] < 0 (device memory: outside [0, ncodes) — never an out-of-range write),
 *     NMOD_STATUS_EMPTY       n == 0,
 *     NMOD_STATUS_TOO_LARGE   n > NMOD_MAX_DEEP,
 *     NMOD_STATUS_NONFINITE   a NaN or infinite sample (exact: every sample is seen; kept or not makes no difference).
 *     The first three are set together where they apply together; the samples of a position they drop are not looked at, so it never
 *     carries NMOD_STATUS_NONFINITE.  A position that is not dropped has status 0.
 *   Per code, over the kept samples of its remaining positions: n_samples = N, n_clipped = the samples not kept, n_positions = the
 *     positions with at least one kept sample, mean, and sd with ddof = 0 over the POOLED SAMPLES — the total spread around the
 *     k-mer's level (within and between positions), which is what a per-position prediction from the table has to carry.  N == 0
 *     gives mean = sd = NaN.
 *   int16 is exact: S1 = sum k in int64, S2 = sum k^2 in uint64 (a row of 2^24 - 1 samples of +-32 767 fits), V = N S2 - S1^2 in 128
 *     bits, mean = ((double)S1 / (double)N) / 1000.0, sd = sqrt((double)V) / (double)N / 1000.0 with (double)V correctly rounded.
 *     Limit: fewer than 2^32 samples (kept plus clipped) per code.  Integer sums are order-free: the int16 result is bit-identical
 *     under any permutation of the positions.
 *   float32 / float64: per position (n, mean, M2) over its kept samples in fp64 (two passes about the mean, with the correction
 *     term), combined per code with the pairwise update of Chan, Golub and LeVeque in a fixed order: the code's positions in index
 *     order, rank r on lane r mod 64 chained over r, then a fixed tree over the lanes.  No float atomics: the bits of a code's
 *     outputs depend on that code's positions only (their samples and their relative order), not on the other positions of the
 *     batch, CSR versus stride, the memspace or the CU count.
 * A NULL member of `out` is skipped; out->struct_size = sizeof(nmod_kmer_out).  Rows: CSR when `off` is given, else the fixed stride
 * prm->stride0.  Reads struct_size, device, stream, memspace, dtype, stride0 of prm and nothing else.  NMOD_MEM_DEVICE: everything
 * is enqueued on prm->stream, the scratch (40 bytes per code for int16; 48 bytes per position for floats) comes stream-ordered from
 * the library's pool, and the call returns WITHOUT synchronising.  NMOD_MEM_HOST: copy in, run, copy back, synchronise (one staged
 * copy, like K8 / K9).  npos == 0 is NMOD_OK with zero counts and NaN mean / sd.  NMOD_ERR_INVALID_ARG before any device work: npos
 * < 0 or beyond 2^31 - 2, ncodes outside 1 .. NMOD_MAX_KMER_CODES, out NULL (or of another struct_size), a NULL sig / code with npos
 * > 0, neither offsets nor a stride, an unknown dtype, exactly one of keep_lo / keep_hi, host offsets that decrease, and (host memory
 * only) a code outside [-1, ncodes).  int16 is the streaming form (every sample byte read once); the float forms are not tuned. */
#define NMOD_MAX_KMER_CODES 65536          /* 4^8 */
#define NMOD_STATUS_NO_CODE 64             /* nmod_kmer_model only: code[i] < 0 (or, device memory, outside [-1, ncodes)): the position takes no part */
typedef struct nmod_kmer_out { int32_t struct_size; int32_t reserved;
  int64_t *n_positions, *n_samples, *n_clipped;   /* ncodes each; a NULL member is skipped */
  double  *mean, *sd;                              /* ncodes each */
  uint8_t *pos_status;                             /* npos, optional */ } nmod_kmer_out;
int nmod_kmer_model(const nmod_params* prm, int64_t npos, const void* sig, const int64_t* off /* or prm->stride0 */,
                    const int32_t* code, int32_t ncodes,
                    const double* keep_lo, const double* keep_hi /* ncodes each, both NULL = keep everything */,
                    const nmod_kmer_out* out);

/* The MODIFIED k-mer table learnt from a mixed sample (K17; the reference project has no such step — its simulations mix modified
 * and unmodified reads at a share, mySimulate.py --Percentages).  Per k-mer code the unmodified component is fixed at a control
 * table's entry (mean0[c], sd0[c]: what nmod_kmer_model gave for an unmodified control), the events of all positions of the code
 * are pooled as K10 pools them, and y ~ (1 - pi) N(mean0, sd0^2) + pi N(m, v) is fitted by K8's EM on the pooled HISTOGRAM: events
 * lie on the 0.001 grid, so the pooled data of a code is an integer histogram, built once, exactly and order-free.
 *   Usable codes, windows: code c is usable iff mean0[c] and sd0[c] are finite, sd0[c] > 0 and |mean0[c]| <= 1000.  Its window is
 *     the integers lo_c .. lo_c + NMOD_KMIX_BINS - 1 with lo_c = llrint(1000.0 * mean0[c]) - NMOD_KMIX_HALF: +-2.048 units, +-10 sd
 *     at the usual 0.2.  An unusable code gets NMOD_KMIX_NO_MODEL, NaN estimates, iters 0, zero counts and a zero histogram row.
 *   Samples: a sample has the integer k — int16: the value itself; float32 (up-cast) / float64: k = rint(1000.0 * x), ties to
 *     even.  For float rows the estimate is therefore that of the rows ROUNDED TO THE 3-DECIMAL GRID every event file is written on.
 *     A NaN or infinite sample is counted in n_outside and sets NMOD_STATUS_NONFINITE in pos_status; it does NOT drop its position
 *     (a deliberate difference from K10: the pass stays streaming).  So does a finite x whose 1000.0 * x is not: outside, no flag.
 *   Positions dropped whole, flagged in pos_status as K10 flags them: NMOD_STATUS_NO_CODE (code[i] < 0; device memory: outside
 *     [0, ncodes) — never an out-of-range write), NMOD_STATUS_EMPTY (n == 0), NMOD_STATUS_TOO_LARGE (n > NMOD_MAX_DEEP), set together
 *     where they apply together.  A position of an unusable code takes no part either (its pos_status carries no bit for that: the
 *     code's NMOD_KMIX_NO_MODEL says it).  Every other position has status 0, or NMOD_STATUS_NONFINITE as above.
 *   Histogram and counts per code, over its remaining positions: hist[c][b] = the samples with k == lo_c + b; n_used = sum_b hist;
 *     n_outside = the samples outside the window; n_positions = the positions with at least one sample inside.  Limit, as in K10:
 *     fewer than 2^32 samples per code.
 *   EM: K8's definition with weights h_b = hist[c][b] at x_b = (double)(lo_c + b) / 1000.0.  n = n_used, mu = mean0[c], s = sd0[c],
 *     s2 = s * s, ybar = ((double)S1 / (double)n) / 1000.0 with S1 = sum_b h_b (lo_c + b) exact in int64.  Start pi = 0.5,
 *     m = mu + 2 (ybar - mu), v = s2; iteration k = 1, 2, ...:
 *       t_b = ln((1 - pi) / pi) [+ 1/2 ln(v / s2), free model] + (x_b - m)^2 / (2 v) - (x_b - mu)^2 / (2 s2)     r_b = 1 / (1 + exp(t_b))
 *       W = sum h_b r_b,  pi' = W / n,  m' = sum h_b r_b x_b / W,  free model: v' = max(sum h_b r_b (x_b - m')^2 / W, s2 / 16)
 *       delta = max(|pi' - pi|, |m' - m| / s [, |sqrt(v') - sqrt(v)| / s]);  take the primed values
 *     and stop when delta <= tol (tol > 0) or k == max_iter; tol == 0 runs exactly max_iter iterations.  With the final parameters
 *     and one more evaluation of t_b: llr = 2 sum_b h_b [ln(1 - pi) + softplus(-t_b)].  Sums run over the bins in an order that is a
 *     fixed function of the bin index (bin b belongs to thread b mod 256, which chains its bins upwards; then a fixed-order
 *     reduction over the threads); an empty bin adds exactly 0.0.  No float atomics anywhere: a code's outputs are bit-identical
 *     under any order of the positions, CSR or stride, host or device memory, any other codes in the batch and any CU count; for
 *     float rows that round to the same k they are those of the int16 rows.
 *   llr is A SCORE, NOT A TEST, for K8's reason (pi = 0 lies on the boundary with m unidentified) and one more: the pooled events of
 *     a k-mer are not exactly normal, because the level varies between positions, so at 10^6 samples ANY second component is
 *     "significant".  Select k-mers by effect size (pi, |m - mu| / s), as nanomod_amd.kmermodel.learn_alt_model does.
 *   Status per code (NMOD_KMIX_* bits):
 *     NMOD_KMIX_NOT_CONVERGED  max_iter iterations ran without the stopping rule ending them (tol == 0: always); the estimates are written
 *     NMOD_KMIX_DEGENERATE     W underflowed to 0 (!(W > 0)): NaN estimates, iters 0
 *     NMOD_KMIX_NO_MODEL       the code is unusable (above)
 *     NMOD_KMIX_VAR_FLOORED    the variance floor was active in the last iteration
 *     NMOD_KMIX_TOO_FEW        n_used < max(opts->min_samples, 2): NaN estimates, iters 0; the counts and the histogram are written
 * Outputs, a NULL member skipped: n_positions, n_used, n_outside, pi, mu_mod (= m), sd_mod (= sqrt v), llr, iters, status (ncodes
 * each), hist (optional, ncodes * NMOD_KMIX_BINS counts) and pos_status (optional, npos).  Rows: CSR when `off` is given, else the
 * fixed stride prm->stride0.  Reads struct_size, device, stream, memspace, dtype, stride0 of prm and nothing else.  NMOD_MEM_DEVICE:
 * everything is enqueued on prm->stream and the call returns WITHOUT synchronising or reading the device; the scratch comes
 * stream-ordered from the library's pool: 16 KiB of histogram per code unless out->hist is given (k = 8: 1 GiB), 24 bytes per
 * position and 1 KiB per 2 048 positions for the grouping by code, 36 bytes per code.  NMOD_MEM_HOST: copy in, run, copy back,
 * synchronise (one staged copy, like K10).  npos == 0 is NMOD_OK with zero counts and NMOD_KMIX_TOO_FEW (NMOD_KMIX_NO_MODEL for an
 * unusable code).  NMOD_ERR_INVALID_ARG before any device work: npos < 0 or beyond 2^31 - 2, ncodes outside 1 ..
 * NMOD_MAX_KMER_CODES, a NULL mean0 / sd0 / opts / out, opts or out of another struct_size, a model outside {0, 1}, max_iter outside
 * 1 .. 10 000, tol negative, NaN or infinite, min_samples < 0, a NULL sig / code with npos > 0, neither offsets nor a stride, an
 * unknown dtype, host offsets that decrease, and (host memory only) a code outside [-1, ncodes).  int16 is the tuned form of the
 * histogram pass (every sample byte read once, in aligned 8-byte pieces); float32 / float64 go through the same kernel a sample at
 * a time and are not tuned. */
#define NMOD_KMIX_HALF 2048
#define NMOD_KMIX_BINS 4096
#define NMOD_KMIX_NOT_CONVERGED 1
#define NMOD_KMIX_DEGENERATE    2
#define NMOD_KMIX_NO_MODEL      4
#define NMOD_KMIX_VAR_FLOORED   8
#define NMOD_KMIX_TOO_FEW      16
typedef struct nmod_kmix_opts { int32_t struct_size, model /* 0 equal variance, 1 free */, max_iter, reserved;
  int64_t min_samples; double tol; } nmod_kmix_opts;
typedef struct nmod_kmix_out { int32_t struct_size, reserved;
  int64_t *n_positions, *n_used, *n_outside;          /* ncodes each; a NULL member is skipped */
  double  *pi, *mu_mod, *sd_mod, *llr;                /* ncodes each */
  int32_t *iters; uint8_t *status;                    /* ncodes each */
  uint32_t *hist;                                     /* ncodes * NMOD_KMIX_BINS, optional */
  uint8_t *pos_status;                                /* npos, optional */ } nmod_kmix_out;
int nmod_kmer_mix(const nmod_params* prm, int64_t npos, const void* sig, const int64_t* off /* or prm->stride0 */,
                  const int32_t* code, int32_t ncodes, const double* mean0, const double* sd0,
                  const nmod_kmix_opts* opts, const nmod_kmix_out* out);

/* Per-read shift and scale against a k-mer model (K11; the reference project has no such step): a robust weighted linear fit of a
 * read's event levels x against the model levels mu of their k-mers, x ~ a + b mu, and the rescaled events (x - a) / b, so that the reads
 * of a sample sit on the scale of a model built by nmod_kmer_model from another run.
 *   Inputs: a read set as flat arrays in nmod_pivot_reads' layout: off[nreads + 1] (int64 CSR event offsets; required, there is no stride
 *     form), val (prm->dtype) and base (one byte per event, the read's own base), events in read direction for both strands.
 *   Model: k in 1 .. 8, center in 0 .. k - 1, mean[4^k] and sd[4^k] (doubles, in the call's memspace).
 *   Code of an event: event j of a read of n events has the code c_j of the bytes base[j - center .. j + k - 1 - center]: A = 0, C = 1,
 *     G = 2, T = 3, upper case only, the first base most significant (kmermodel.kmer_codes' convention); c_j = -1 when the window leaves
 *     the read or holds any other byte.
 *   Eligible: c_j >= 0, mean[c_j] and sd[c_j] finite with sd[c_j] > 0, and x_j finite.  x_j is the value as a double (int16 k / 1000.0, a
 *     division; float32 up-cast; float64 as is), mu_j and s_j the model entries, w_j = 1.0 / (s_j * s_j) when `weighted`, else 1.
 *   Fit over a kept set K: W = sum w, mb = sum w mu / W, xb = sum w x / W, Smm = sum w (mu - mb)^2, Smx = sum w (mu - mb)(x - xb),
 *     b = Smx / Smm, a = xb - b mb.  The sums are taken in fp64 about the read's first eligible event (mu_0, x_0) — mu - mu_0 and
 *     x - x_0 in place of mu and x, which changes no centred sum in exact arithmetic and makes Smm exactly 0 for a read of one level —
 *     in a fixed order (a chain per lane, then a fixed lane / wave reduction; no float atomics).
 *     Round 0 uses K = the eligible events; each of clip_rounds further rounds keeps the eligible events with
 *     |x_j - a - b mu_j| <= clip_sigma |b| s_j, (a, b) from the round before, and fits again.
 *   A read fails, at the first round where it applies, with NMOD_RESCALE_TOO_FEW (|K| < min_events), NMOD_RESCALE_DEGENERATE (Smm not
 *     > 0, b not finite or b <= 0, a not finite), after the last round with NMOD_RESCALE_OUT_OF_RANGE (b outside [scale_lo, scale_hi]), and before any
 *     with NMOD_RESCALE_TOO_LARGE (n > NMOD_MAX_DEEP).
 *   Outputs per read (a NULL member is skipped): shift = a, scale = b, n_used = |K| of the last round that ran, status (NMOD_RESCALE_*
 *     bits).  A failed read gets shift = 0 and scale = 1, and its events are copied unchanged.
 *   Apply: val_out has the dtype and layout of val and may be val itself.  Every event of a fitted read, eligible or not:
 *     r = 1.0 / b, x' = (x - a) * r (a non-finite x stays as it is); float64: x', float32: (float)x', int16: rint(1000.0 * x'), ties to
 *     even, saturated to +-32 767, and a saturation sets NMOD_RESCALE_CLAMPED on the read.  Compiled with contraction off: bit-defined.
 *   Modes: NMOD_RESCALE_FIT_APPLY; NMOD_RESCALE_FIT_ONLY (val_out is not touched); NMOD_RESCALE_APPLY_ONLY: shift / scale are INPUTS
 *     (left as they are), the model and base are not read, n_used = 0; a read whose scale is not finite or <= 0, or whose shift is not
 *     finite, is DEGENERATE and copied unchanged.
 * Reads struct_size, device, stream, memspace, dtype of prm and nothing else.  NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no
 * host read and no synchronisation; scratch (8 bytes per read + 24 bytes per model entry) comes stream-ordered from the library's pool.
 * NMOD_MEM_HOST: copy in, run, copy back, synchronise (one staged copy).  nreads == 0 is NMOD_OK.  NMOD_ERR_INVALID_ARG before any
 * device work: an unknown mode, k or center out of range, clip_rounds outside 0 .. 8, clip_sigma not finite or <= 0 with clip_rounds > 0,
 * min_events < 2, scale_lo not > 0 or not finite or > scale_hi, nreads < 0 or beyond 2^32 - 2, NULL off / val with nreads > 0, NULL base
 * or model (or its arrays) when the mode fits, NULL val_out when it applies, NULL shift / scale in APPLY_ONLY, opts / out NULL or of
 * another struct_size, an unknown dtype, host offsets that decrease.
 * A read's outputs are the same bits whatever else is in the batch, in any order of the reads, from host or device memory, in place or
 * not.  A read is computed by one wave (up to NMOD_RESCALE_WAVE_MAX events) or one workgroup: a single very long read is not split. */
enum { NMOD_RESCALE_FIT_APPLY = 0, NMOD_RESCALE_FIT_ONLY = 1, NMOD_RESCALE_APPLY_ONLY = 2 };
enum { NMOD_RESCALE_TOO_FEW = 1, NMOD_RESCALE_DEGENERATE = 2, NMOD_RESCALE_OUT_OF_RANGE = 4, NMOD_RESCALE_CLAMPED = 8, NMOD_RESCALE_TOO_LARGE = 16 };
#define NMOD_RESCALE_WAVE_MAX 2048         /* events of a read: up to here a wave computes it, beyond a workgroup */
typedef struct nmod_rescale_model { int32_t k, center; const double *mean, *sd; /* 4^k each */ } nmod_rescale_model;
typedef struct nmod_rescale_opts { int32_t struct_size, mode, weighted, clip_rounds, min_events, reserved;
  double clip_sigma, scale_lo, scale_hi; } nmod_rescale_opts;
typedef struct nmod_rescale_out { int32_t struct_size; int32_t reserved;
  double *shift, *scale;          /* nreads each; inputs in NMOD_RESCALE_APPLY_ONLY */
  int32_t* n_used; uint8_t* status; /* nreads each */
  void* val_out;                  /* the events, prm->dtype, in val's layout */ } nmod_rescale_out;
int nmod_rescale_reads(const nmod_params* prm, int64_t nreads, const int64_t* off, const void* val, const uint8_t* base,
                       const nmod_rescale_model* model, const nmod_rescale_opts* opts, const nmod_rescale_out* out);

/* Per-read modification calls against a k-mer model (K12; the reference project has no such step): every event of every read is scored
 * against the model level of its k-mer, the scores of neighbouring events OF THE SAME READ are combined by Fisher's method, and an event
 * whose combined p-value is at most alpha is called.  The single-molecule counterpart of nmod_one_sample: which reads are modified where.
 *   Inputs: exactly those of nmod_rescale_reads: off[nreads + 1] (int64 CSR event offsets; required, there is no stride form), val
 *     (prm->dtype) and base (one byte per event, the read's own base), events in read direction for both strands; the model is K11's
 *     struct as it is: k in 1 .. 8, center in 0 .. k - 1, mean[4^k] and sd[4^k] (doubles, in the call's memspace).
 *   Code of an event: event j of a read of n events has the code c_j of the bytes base[j - center .. j + k - 1 - center]: A = 0, C = 1,
 *     G = 2, T = 3, upper case only, the first base most significant (kmermodel.kmer_codes' convention); c_j = -1 when the window leaves
 *     the read or holds any other byte.
 *   Eligible: c_j >= 0, mean[c_j] and sd[c_j] finite with sd[c_j] > 0, and x_j finite.  x_j is the value as a double (int16 k / 1000.0, a
 *     division; float32 up-cast; float64 as is), mu_j and s_j the model entries.
 *   An eligible event j, compiled with contraction off:
 *     z_j = (x_j - mu_j) / s_j,  u_j = |z_j| * 0.70710678118654752,
 *     p_j = max(erfc(u_j), DBL_MIN): the two-sided normal tail, clamped like every p-value of the library,
 *     l_j = log(erfcx(u_j)) - u_j * u_j: the logarithm of the UNCLAMPED tail.  It does not underflow, so a window keeps what its events
 *       say beyond |z| = 37.52, where p_j sits at DBL_MIN.
 *   Window of j: the ELIGIBLE events i of the same read with |i - j| <= nb and 0 <= i < n.  Ineligible events and events beyond the ends
 *     of the read take no part (a read is a wall: no window reaches into a neighbouring read).  W_j = the number of events in the window
 *     (at least 1: j itself), X_j = -2 * sum l_i with the terms added in ascending i, and
 *     P_j = max(chi2.sf(X_j, 2 W_j), DBL_MIN) — Fisher's method over the events that exist, chi2.sf with an even number of degrees of
 *     freedom as the closed sum exp(-X/2) sum_{m < W} (X/2)^m / m!.  nb == 0: P_j is p_j, the same bits.
 *   An ineligible event gets z = p = p_win = NaN, whatever its neighbours are.
 *   Per read: n_sites = the eligible events, n_called = #{j : P_j <= alpha}, status 0 or NMOD_CALLS_TOO_LARGE (n > NMOD_MAX_DEEP: NaN
 *     events and zero counts).  A read without an eligible event is not an error: zero counts, status 0.
 *   Outputs (a NULL member is skipped; out->struct_size = sizeof(nmod_calls_out)): per event, in val's layout, z, p and p_win = P as
 *     doubles (every p-value of the library is fp64); per read n_sites, n_called (int32) and status (uint8).
 * Reads struct_size, device, stream, memspace, dtype of prm and nothing else; the window width is opts->nb, not prm->nb.
 * NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no host read and no synchronisation; scratch (8 bytes per read + 16 bytes per
 * model entry) comes stream-ordered from the library's pool.  NMOD_MEM_HOST: copy in, run, copy back, synchronise (one staged copy).
 * nreads == 0 is NMOD_OK.  NMOD_ERR_INVALID_ARG before any device work: nb outside 0 .. NMOD_MAX_NB, alpha not in (0, 1], k or center out
 * of range, nreads < 0 or beyond 2^32 - 2, NULL off / val / base / model arrays with nreads > 0, model / opts / out NULL or (opts, out) of
 * another struct_size, an unknown dtype, host offsets that decrease.
 * A read's outputs are the same bits whatever else is in the batch, in any order of the reads, from host or device memory, and whichever
 * output members were requested.  A read is computed by one wave (up to NMOD_CALLS_WAVE_MAX events) or one workgroup: a single very long
 * read is not split.  No float atomics: the counts are integer reductions. */
#define NMOD_CALLS_TOO_LARGE 16            /* status of a read beyond NMOD_MAX_DEEP events */
#define NMOD_CALLS_WAVE_MAX 2048           /* events of a read: up to here a wave computes it, beyond a workgroup */
typedef struct nmod_calls_opts { int32_t struct_size, nb; double alpha; } nmod_calls_opts;
typedef struct nmod_calls_out { int32_t struct_size; int32_t reserved;
  double *z, *p, *p_win;            /* one per event, in val's layout */
  int32_t *n_sites, *n_called; uint8_t* status; /* nreads each */ } nmod_calls_out;
int nmod_read_calls(const nmod_params* prm, int64_t nreads, const int64_t* off, const void* val, const uint8_t* base,
                    const nmod_rescale_model* model, const nmod_calls_opts* opts, const nmod_calls_out* out);

/* Per-position call counts over pivoted scores (K12): the rows nmod_pivot_reads makes when the p_win track of nmod_read_calls is handed
 * to it as `val` with dtype F64 — one row of doubles per position, one score per read that covers it.
 *   Per position: n_valid = #{s : 0 <= s <= 1} (the validity rule of nmod_fdr_adjust; NaN means no call), n_called = #{valid s <= alpha},
 *     frac = (double)n_called / (double)n_valid, NaN when n_valid == 0.
 *   Outputs (a NULL member is skipped; out->struct_size = sizeof(nmod_site_out)): int32 n_valid, n_called and double frac, npos each.
 * Rows: CSR when `off` is given, else the fixed stride prm->stride0.  Reads struct_size, device, stream, memspace, stride0 of prm and
 * nothing else (the scores are doubles whatever prm->dtype says).  Both memspaces as above; npos == 0 is NMOD_OK.  NMOD_ERR_INVALID_ARG
 * before any device work: alpha not in (0, 1], neither offsets nor a stride, npos < 0 or beyond 2^31 - 2, a NULL score with npos > 0, out
 * NULL or of another struct_size, host offsets that decrease.  Integer counts: order-free, the same bits in CSR and stride form.  A wave
 * per row; not tuned. */
typedef struct nmod_site_out { int32_t struct_size; int32_t reserved; int32_t *n_valid, *n_called; double* frac; } nmod_site_out;
int nmod_site_calls(const nmod_params* prm, int64_t npos, const double* score, const int64_t* off /* or prm->stride0 */, double alpha,
                    const nmod_site_out* out);

/* Per-read log-likelihood ratios between two k-mer models (K13; the reference project has no such step): every event of every read is
 * scored against the level of its k-mer in the unmodified table `model` and in the modified table `alt`, the ratios of the events OF THE
 * SAME READ inside a window are summed, and an event is called modified, canonical or left ambiguous by that sum.  Where nmod_read_calls
 * asks "is this level an outlier of the null", this asks "which of the two levels is it".
 *   Inputs: exactly those of nmod_read_calls: flat reads in nmod_pivot_reads' layout, off[nreads + 1] (int64 CSR event offsets; required,
 *     there is no stride form), val (prm->dtype) and base (one byte per event), events in read direction; two nmod_rescale_model structs,
 *     `model` (mean0, sd0) and `alt` (mean1, sd1).  alt->k and alt->center must equal model's.  All four tables live in the call's
 *     memspace.
 *   Code of an event: K11 / K12's rule word for word: the bytes base[j - center .. j + k - 1 - center], A = 0, C = 1, G = 2, T = 3, upper
 *     case only, the first base most significant; a window that leaves the read, or a byte that is not A / C / G / T, gives code -1.
 *   Per code c, once per call: the code is usable iff mean0, sd0, mean1, sd1 are all finite and both spreads are > 0;
 *     g_c = log(sd0_c / sd1_c), one division and then log.
 *   Per event j, compiled with contraction off: the event is a candidate iff its code is usable and x_j is finite (x_j the value as a
 *     double: int16 k / 1000.0, a division; float32 up-cast; float64 as is);
 *       z0 = (x - mu0) / sd0,  z1 = (x - mu1) / sd1,  d = 0.5 * ((z0 - z1) * (z0 + z1)),  llr_j = g_c + d,
 *     which is ln N(x; mu1, sd1^2) - ln N(x; mu0, sd0^2): a positive value favours the modified model.  The event is ELIGIBLE iff it is a
 *     candidate and fabs(llr_j) <= NMOD_LLR_MAX (1e300): every window sum is then finite, and the inf - inf case of a near-zero spread is
 *     gone.  An ineligible event gets NaN in every per-event output and takes no part in any window.
 *   Window of j: the eligible events i of the same read with j - nb_lo <= i <= j + nb_hi and 0 <= i < n; nb_lo and nb_hi lie in
 *     0 .. NMOD_MAX_NB, independently.  A read is a wall, as in K12.  (The k-mer cover of base j — the events whose k-mer contains the
 *     base — is nb_lo = k - 1 - center, nb_hi = center: the default of the Python layers.)
 *   Per eligible event: L_j = the sum of llr_i over the window, the terms added in ascending i (nb_lo = nb_hi = 0: L_j is llr_j, the same
 *     bits);  t = L_j + prior_logit;  p_mod_j = t >= 0 ? 1 / (1 + exp(-t)) : exp(t) / (1 + exp(t)).  p_mod is a posterior, not a
 *     p-value: it is not clamped and may be 0 or 1.
 *   Calls, with thr > 0 finite: event j is MOD iff L_j >= thr, otherwise CAN iff L_j <= -thr, otherwise ambiguous.
 *   Per read: n_sites = the eligible events, n_mod, n_can (int32), status 0 or NMOD_CALLS_TOO_LARGE (n > NMOD_MAX_DEEP: NaN events and zero
 *     counts, as in K12).  A read without an eligible event is not an error.
 *   Outputs (a NULL member is skipped; out->struct_size = sizeof of the out struct): per event, in val's layout, llr, llr_win = L and
 *     p_mod as doubles; per read n_sites, n_mod, n_can (int32) and status (uint8).  Requesting fewer outputs never changes the bits of
 *     the others.
 * Reads struct_size, device, stream, memspace, dtype of prm and nothing else.  NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no
 * host read and no synchronisation; scratch (8 bytes per read + 40 bytes per code) comes stream-ordered from the library's pool.
 * NMOD_MEM_HOST: copy in, run, copy back, synchronise (one staged copy).  nreads == 0 is NMOD_OK.  NMOD_ERR_INVALID_ARG before any device
 * work: a window bound outside 0 .. NMOD_MAX_NB, thr not finite or <= 0, prior_logit not finite or |prior_logit| > 700, k or center out of
 * range or differing between the two models, and the size, NULL and offset rules of nmod_read_calls (nreads < 0 or beyond 2^32 - 2, NULL
 * off / val / base / table arrays with nreads > 0, model / alt / opts / out NULL or (opts, out) of another struct_size, an unknown dtype,
 * host offsets that decrease).
 * A read's bits depend on the read alone: not on the batch, the order of the reads, the memspace or the outputs asked for.  A read is
 * computed by one wave (up to NMOD_CALLS_WAVE_MAX events) or one workgroup.  No float atomics: the counts are integer reductions.
 * Stops here: two tables only; one window per call; no per-site prior (nmod_site_stoich, K14, estimates the share per site from the
 * window sums); the k-mers of both tables must match. */
#define NMOD_LLR_MAX 1e300                 /* an event whose |llr| lies beyond is ineligible */
typedef struct nmod_llr_opts { int32_t struct_size, nb_lo, nb_hi, reserved; double thr, prior_logit; } nmod_llr_opts;
typedef struct nmod_llr_out { int32_t struct_size; int32_t reserved;
  double *llr, *llr_win, *p_mod;    /* one per event, in val's layout */
  int32_t *n_sites, *n_mod, *n_can; uint8_t* status; /* nreads each */ } nmod_llr_out;
int nmod_read_llr(const nmod_params* prm, int64_t nreads, const int64_t* off, const void* val, const uint8_t* base,
                  const nmod_rescale_model* model, const nmod_rescale_model* alt, const nmod_llr_opts* opts, const nmod_llr_out* out);

/* Per-position counts over pivoted window sums (K13): the rows nmod_pivot_reads makes when the llr_win track of nmod_read_llr is handed
 * to it as `val` with dtype F64 — one row of doubles per position, one sum per read that covers it.
 *   Per row: n_valid = #{s : fabs(s) <= DBL_MAX}, n_mod = #{s >= thr}, n_can = #{s <= -thr},
 *     frac = (double)n_mod / (double)(n_mod + n_can), NaN when that denominator is 0: the modified share of the confident reads.
 *   Outputs (a NULL member is skipped): int32 n_valid, n_mod, n_can and double frac, npos each.
 * Argument rules, memspaces and the CSR / stride forms are those of nmod_site_calls, with thr (finite, > 0) in the place of alpha. */
typedef struct nmod_site_llr_out { int32_t struct_size; int32_t reserved; int32_t *n_valid, *n_mod, *n_can; double* frac; } nmod_site_llr_out;
int nmod_site_llr(const nmod_params* prm, int64_t npos, const double* score, const int64_t* off /* or prm->stride0 */, double thr,
                  const nmod_site_llr_out* out);

/* Per-read log-likelihood ratios of one unmodified k-mer table against SEVERAL modified tables in one walk, with a joint call and a
 * posterior over the states per event (K26; the reference project has no such step).  Where nmod_read_llr asks "modified or canonical"
 * against one alternative, this asks "which of n_alt modifications, or none": state 0 is canonical, state m (1 .. n_alt) is alt[m-1].
 *   Inputs: nmod_read_llr's, with n_alt (1 .. NMOD_MULTI_MAX) and alt, an array of n_alt pointers to nmod_rescale_model structs, in the
 *     place of `alt`; every alt[m]->k and ->center must equal model's; all tables live in the call's memspace (the structs and the array
 *     of pointers on the host).  total_events >= 0 is the length of one output plane: per-event outputs are PLANES of total_events
 *     elements, plane p at out[p * total_events + j] with j the event's index in val's layout; a host call requires
 *     off[nreads] <= total_events.  opts->prior_logit[m-1] is the log prior odds of state m against canonical, each finite with
 *     |.| <= 700 (entries beyond n_alt are not read).  One thr and one window (nb_lo, nb_hi) for all states.
 *   Tracks.  Track m is nmod_read_llr's llr and llr_win for the pair (model, alt[m-1]), word for word: the usable-code rule per pair,
 *     the candidate and eligibility rule with NMOD_LLR_MAX, the formula with contraction off, the ascending window sum that skips
 *     ineligible terms, reads as walls, NMOD_CALLS_TOO_LARGE.  Plane m-1 of llr and of llr_win therefore holds the BITS that
 *     nmod_read_llr(model, alt[m-1]) writes with the same window.  A plane is contiguous and goes into nmod_pivot_reads as `val`.
 *   Joint call per event, contraction off.  State m is OPEN at event j iff L_m (its llr_win) is not NaN; the event is eligible iff some
 *     state is open.  b = the open m with the largest L_m, ties to the smaller m; second = the largest of 0 and the other open L_m'.
 *       call = b                        iff L_b - second >= thr
 *            = 0 (canonical)            iff every open L_m <= -thr
 *            = NMOD_MULTI_AMBIGUOUS     otherwise
 *            = NMOD_MULTI_NONE          for an ineligible event.
 *     At n_alt = 1 this is nmod_read_llr's MOD / CAN rule exactly.
 *   Posterior (post, n_alt + 1 planes, plane 0 canonical): u_0 = 0 and u_m = L_m + prior_logit[m-1] over the open m; mx = the largest of
 *     0 and the u_m; e_0 = exp(-mx), e_m = exp(u_m - mx); Z = e_0 + e_m summed in ascending m; post_m = e_m / Z.  0 for a closed state,
 *     NaN in every plane for an ineligible event.  Not clamped: a plane may hold 0 or 1.
 *   Per read: n_sites = the eligible events, n_can = the events called 0, n_mod = n_alt planes of nreads (plane m-1 counts the events
 *     called m), all int32, and status (uint8) 0 or NMOD_CALLS_TOO_LARGE (NaN tracks, NMOD_MULTI_NONE calls, zero counts).
 *   Outputs: llr, llr_win (n_alt planes each), post (n_alt + 1 planes), call (uint8, total_events), n_sites, n_can (nreads), n_mod
 *     (n_alt * nreads), status (nreads).  A NULL member is skipped, and asking for fewer outputs never changes the bits of the others.
 *     Elements of a plane outside [off[0], off[nreads]) are left alone by a device call and are unspecified after a host call.
 * nmod_read_llr's contract carries over: prm's fields read, the memspaces, everything on prm->stream with no host read and no
 * synchronisation for NMOD_MEM_DEVICE (scratch: 8 bytes per read + 8 (2 + 3 n_alt) bytes per code, stream-ordered from the pool), a read's
 * bits depend on the read alone, no float atomics.  NMOD_ERR_INVALID_ARG before any device work: nmod_read_llr's refusals, and n_alt
 * outside 1 .. NMOD_MULTI_MAX, alt or an alt[m] NULL, a k or center that differs in any alt[m], a prior_logit[m] (m < n_alt) not finite
 * or beyond 700 in magnitude, total_events < 0 or (host) < off[nreads].
 * nmod_read_llr_multi_table_in_lds(n_alt, k): 1 if a call with these sizes keeps its table in LDS, 0 if it reads it through L2 (the two
 * forms give the same bits; tests use this to cover both), -1 for sizes out of range.
 * Stops here: one window and one threshold for all states; normal levels; reads independent; the states exclusive at a base (no
 * "both m6A and m5C in this k-mer"); n_alt <= NMOD_MULTI_MAX. */
#define NMOD_MULTI_MAX 4
#define NMOD_MULTI_AMBIGUOUS 255           /* call: eligible, but neither one state nor canonical by thr */
#define NMOD_MULTI_NONE 254                /* call: an ineligible event */
typedef struct nmod_llr_multi_opts { int32_t struct_size, nb_lo, nb_hi, reserved; double thr; double prior_logit[NMOD_MULTI_MAX]; } nmod_llr_multi_opts;
typedef struct nmod_llr_multi_out { int32_t struct_size; int32_t reserved;
  double *llr, *llr_win, *post;     /* n_alt, n_alt, n_alt + 1 planes of total_events */
  uint8_t* call;                    /* total_events */
  int32_t *n_sites, *n_can, *n_mod; uint8_t* status; /* nreads each; n_mod: n_alt planes of nreads */ } nmod_llr_multi_out;
int nmod_read_llr_multi(const nmod_params* prm, int64_t nreads, int64_t total_events, const int64_t* off, const void* val,
                        const uint8_t* base, const nmod_rescale_model* model, int32_t n_alt, const nmod_rescale_model* const* alt,
                        const nmod_llr_multi_opts* opts, const nmod_llr_multi_out* out);
int nmod_read_llr_multi_table_in_lds(int32_t n_alt, int32_t k);

/* Per-position modified fraction by maximum likelihood, with a likelihood interval, a test of "nothing is modified here" and a posterior
 * per read (K14; the reference project has no such step).  The rows are those of nmod_site_llr: per position the window sums L of the
 * reads that cover it.  If a share pi of the molecules is modified, the log-likelihood of the row relative to "all canonical" is
 *     l(pi) = sum_i log(1 - pi + pi e^{s_i}),
 * concave on [0, 1]; nmod_site_llr's hard-call share is replaced by its maximiser.
 *   Inputs, memspaces, the CSR / stride forms, the NULL and struct_size rules: exactly those of nmod_site_llr.
 *   A score is VALID iff fabs(s) <= DBL_MAX; n = the number of valid scores of the row.  Per valid score, once:
 *       t = -expm1(-fabs(s))   in [0, 1] (1 from |s| of about 37 on),   the side: s >= 0 ("plus", -0.0 included) or s < 0 ("minus").
 *     An invalid score takes no part (it counts as t = 0).
 *   One EVALUATION at pi, compiled with contraction off, per valid score with q = 1 - pi on the plus side and q = pi on the minus side:
 *       qt = q * t,   u = t / (1 - qt),   S += u (plus) or -u (minus),   D += u * u,   g += log1p(-qt).
 *     S(pi) is the score function dl/dpi (decreasing), -D its derivative, g the reduced log-likelihood: l(pi) = g(pi) + P with
 *     P = the sum of the valid s >= 0.  A zero denominator (t = 1 at q = 1: the ends only) gives u = +inf and g = -inf, which is wanted.
 *     No exp is evaluated inside an iteration and nothing overflows for any valid s.
 *   The estimate pi^: 0 iff S(0) <= 0 (NMOD_STOICH_AT_ZERO); otherwise 1 iff S(1) >= 0 (NMOD_STOICH_AT_ONE); otherwise the root of S in
 *     (0, 1) by the BRACKETED ITERATION below with F = S.
 *   The bracketed iteration on a bracket (a, b): x = a + 0.5 (b - a); then for k = 1 .. max_iter:
 *       evaluate at x;  the root lies right of x (a = x) or left of it (b = x) by the sign rule of the root in question;
 *       x' = the Newton point of the root in question;  if x' != x and not (a < x' < b) with the new a, b:  x' = a + 0.5 (b - a)
 *         (x' == x: the Newton step is below the spacing of doubles at x, or the function is exactly 0 there, and x stays);
 *       step = |x' - x|;  x = x';  stop iff tol > 0 and (b - a <= tol or step <= tol).
 *     The result is x: a point of a bracket that holds the root.  tol == 0 runs max_iter evaluations.  A root whose loop ends without
 *     the stop test holding sets NMOD_STOICH_NOT_CONVERGED; the values are written all the same.
 *       pi^:    right iff S(x) > 0;                       x' = x + S / D.
 *       pi_lo:  right iff h(x) > ci_drop;                 x' = x + (h - ci_drop) / (2 S)      with h(x) = 2 (g(pi^) - g(x)).
 *       pi_hi:  right iff h(x) <= ci_drop;                the same x'.
 *     iters = the evaluations the iteration for pi^ made (0 at either end); max_iter bounds each of the three roots on its own.
 *   l^ = 0 at pi^ = 0, else max(g(pi^) + P, 0);  stat = 2 l^ (>= 0; +inf when P overflows);
 *   p_null = 1 at pi^ = 0, else max(0.5 erfc(sqrt(l^)), DBL_MIN): the 1/2 chi2_0 + 1/2 chi2_1 boundary law of the likelihood-ratio test of
 *     pi = 0.  It is ASYMPTOTIC, assumes that both tables are right and the reads independent, and is conservative when the two levels
 *     are well separated (a simulation of canonical rows of 20 and 200 reads rejected 2.5 - 4.8 % at the 5 % level: tests/test_site_stoich.py).
 *   The interval {pi : h(pi) <= ci_drop} (the P terms cancel: no inf - inf): pi_lo = 0 iff h(0) <= ci_drop, else the root in (0, pi^);
 *     pi_hi = 1 iff h(1) <= ci_drop, else the root in (pi^, 1).  ci_drop = 3.841458820694124 (the 0.95 quantile of chi2_1) is the
 *     default of the Python layers.
 *   resp (optional, float64, in the score layout): the posterior of every read at pi^, with e = exp(-fabs(s)):
 *       0 at pi^ = 0;  1 at pi^ = 1;  else  s >= 0: pi^ / (pi^ + (1 - pi^) e),   s < 0: (pi^ e) / ((1 - pi^) + pi^ e);
 *     NaN for an invalid score and for every score of a row without an estimate.
 *   Outputs (npos each; a NULL member is skipped; requesting fewer never changes the bits of the others): doubles pi, pi_lo, pi_hi, stat,
 *     p_null; int32 n_valid, iters; uint8 status; and resp.  Status bits:
 *       NMOD_STOICH_TOO_FEW        n < min_valid: NaN outputs, iters 0 (n_valid is written)
 *       NMOD_STOICH_FLAT           every valid score is 0, S is 0 everywhere and pi is not identified: NaN outputs, iters 0
 *       NMOD_STOICH_NOT_CONVERGED  see above
 *       NMOD_STOICH_AT_ZERO, NMOD_STOICH_AT_ONE    pi^ = 0, pi^ = 1
 *       NMOD_STOICH_TOO_LARGE      a row beyond NMOD_MAX_DEEP scores: NaN outputs, n_valid 0, iters 0
 * Sums: a fixed-order chain per lane (the lane's scores in ascending index), then fixed-order lane, wave and LDS reductions; no float
 * atomics.  A row of up to NMOD_STOICH_SMALL scores is computed by 16 lanes, up to NMOD_STOICH_WAVE by a wave, a longer one by a workgroup:
 * a row's bits depend on the row alone, not on the batch, the order of the rows, CSR versus stride, the memspace or the outputs asked for.
 * Reads struct_size, device, stream, memspace, stride0 of prm.  NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no host read and
 * no synchronisation; scratch (12 bytes per row) comes stream-ordered from the library's pool.  npos == 0 is NMOD_OK.
 * NMOD_ERR_INVALID_ARG before any device work: opts NULL or of another struct_size, max_iter outside 1 .. 200, min_valid < 1, tol not
 * finite or < 0, ci_drop not finite or <= 0, and nmod_site_llr's rules for prm, npos, score, off / stride0 and out.
 * Stops here: two states only; the reads are treated as independent; the strands are not pooled; no prior on pi. */
#define NMOD_STOICH_SMALL 256              /* scores of a row up to which 16 lanes compute it */
#define NMOD_STOICH_WAVE 1024              /* ... up to which one wave does (a workgroup beyond) */
enum { NMOD_STOICH_TOO_FEW = 1, NMOD_STOICH_FLAT = 2, NMOD_STOICH_NOT_CONVERGED = 4, NMOD_STOICH_AT_ZERO = 8, NMOD_STOICH_AT_ONE = 16,
       NMOD_STOICH_TOO_LARGE = 32 };
typedef struct nmod_stoich_opts { int32_t struct_size, max_iter, min_valid, reserved; double tol, ci_drop; } nmod_stoich_opts;
typedef struct nmod_stoich_out { int32_t struct_size; int32_t reserved;
  double *pi, *pi_lo, *pi_hi, *stat, *p_null; int32_t *n_valid, *iters; uint8_t* status; /* npos each */
  double* resp;                                                                            /* one per score, in its layout */ } nmod_stoich_out;
int nmod_site_stoich(const nmod_params* prm, int64_t npos, const double* score, const int64_t* off /* or prm->stride0 */,
                     const nmod_stoich_opts* opts, const nmod_stoich_out* out);

/* The shares of all states at a site by maximum likelihood, with a test per state and the responsibilities per read (K26; the reference
 * project has no such step).  nmod_site_stoich's question with nmod_read_llr_multi's states: per position and state m = 1 .. n_alt one row
 * of window sums, s_im for read i, all n_alt rows in ONE layout (the pivoted llr_win planes: nmod_pivot_reads orders its rows by the
 * reads' layout alone, so pivoting each plane gives aligned rows).  With shares pi = (pi_0 canonical, pi_1 .. pi_n_alt) on the simplex, the
 * log-likelihood of the row relative to "all canonical" is
 *     l(pi) = sum_i log(pi_0 + sum_m pi_m e^{s_im}),
 * concave in pi; the estimate is its maximiser by EM.
 *   Inputs: n_alt (1 .. NMOD_MULTI_MAX), score: an array (on the host) of n_alt pointers to float64 scores in the call's memspace, all read
 *     by the one `off` (int64[npos + 1]) or prm->stride0; total_scores: the length of a score plane (>= off[npos], or npos * stride0),
 *     which is also the plane length of resp.  opts: min_valid >= 1, max_iter in 1 .. NMOD_COMPOSE_MAX_ITER, tol >= 0 finite.
 *   Per row.  A score is finite iff fabs(s) <= DBL_MAX.  State m is OPEN iff some s_im of the row is finite.  A read is VALID iff at least
 *     one state is open and its s_im is finite for every open m; n_valid counts them, n_partial counts the reads that are finite in some
 *     but not all open states: they take no part.  Weights, once per valid read: mx_i = the largest of 0 and the s_im of the open m,
 *     w_i0 = exp(-mx_i), w_im = exp(s_im - mx_i); 0 for a closed m.  No exp is evaluated inside an iteration.
 *   The fit (contraction off).  Start: pi_m = 1 / (1 + the number of open states) on canonical and the open states, 0 elsewhere.  One
 *     ITERATION, per valid read: t_0 = pi_0 w_i0, den_i = t_0, then in ascending m t_m = pi_m w_im, den_i += t_m; q = 1 / den_i;
 *     R_m += t_m q.  Then pi'_m = R_m / n_valid, step = max_m |pi'_m - pi_m|, pi = pi'.  Stop iff tol > 0 and step <= tol; max_iter
 *     bounds the iterations; iters = those made.  A fit whose loop ends without the stop test holding (always, at tol == 0) sets
 *     NMOD_COMPOSE_NOT_CONVERGED; the values are written all the same.  One last evaluation at the final pi:
 *     ll = sum_i (log(den_i) + mx_i);  stat = 2 max(ll, 0).  A closed state keeps pi_m = 0.
 *   Per-state test (only when stat_m or p_m is asked for; asking never changes the bits of the other outputs, status's bits from the refits
 *     excepted).  For every open m: the same fit with state m closed as well — the same weights and valid reads, the uniform start over
 *     the rest, the same max_iter and tol — gives ll_without_m;  stat_m = 2 max(ll - ll_without_m, 0);  p_m = 1 at stat_m = 0, else
 *     max(0.5 erfc(sqrt(stat_m / 2)), DBL_MIN): the 1/2 chi2_0 + 1/2 chi2_1 boundary law of the likelihood-ratio test of pi_m = 0.  It is
 *     ASYMPTOTIC, and right only when the remaining shares are interior; it assumes that all tables are right and the reads independent.
 *     A closed m gets NaN.  A refit that does not converge also sets NMOD_COMPOSE_NOT_CONVERGED.  At n_alt = 1, stat_1, p_1 and pi_1 are
 *     nmod_site_stoich's stat, p_null and pi up to the convergence of EM.
 *   resp (optional; n_alt + 1 planes of total_scores in the score layout, plane 0 canonical): t_m q of the last evaluation; NaN in every
 *     plane for a read that is not valid and for every read of a row without an estimate.
 *   Outputs (a NULL member is skipped): pi (n_alt + 1 planes of npos: pi[m * npos + row]), ll, stat (npos), stat_m, p_m (n_alt planes of
 *     npos, plane m - 1 for state m), int32 n_valid, n_partial, iters, uint8 open_mask (bit m - 1: state m is open) and status (npos), resp.
 *     Status bits:
 *       NMOD_COMPOSE_NO_STATE        no state is open: NaN outputs, iters 0
 *       NMOD_COMPOSE_TOO_FEW         a state is open and n_valid < min_valid: NaN outputs, iters 0 (the counts and open_mask are written)
 *       NMOD_COMPOSE_NOT_CONVERGED   see above
 *       NMOD_COMPOSE_DEGENERATE      a den_i of 0 after a share underflowed: NaN outputs, iters 0; in a refit: NaN stat_m and p_m of that state
 *       NMOD_COMPOSE_TOO_LARGE       a row beyond NMOD_MAX_DEEP reads (or, NMOD_MEM_DEVICE, beyond total_scores): NaN outputs, zero counts
 * Sums: a fixed-order chain per lane (the lane's reads in ascending index), then fixed-order lane, wave and LDS reductions; no float
 * atomics.  A row of up to NMOD_STOICH_SMALL reads is computed by 16 lanes, up to NMOD_STOICH_WAVE by a wave, a longer one by a workgroup:
 * a row's bits depend on the row alone, not on the batch, the order of the rows, CSR versus stride, the memspace or the outputs asked for.
 * Reads struct_size, device, stream, memspace, stride0 of prm.  NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no host read and no
 * synchronisation; scratch comes stream-ordered from the library's pool: 12 bytes per row, and 8 (n_alt + 1) total_scores bytes when a row
 * can be longer than nmod_site_compose_stage_reads(n_alt) (by the host offsets or the stride where known, else by total_scores).
 * npos == 0 is NMOD_OK.  NMOD_ERR_INVALID_ARG before any device work: opts / out NULL or of another struct_size, max_iter outside
 * 1 .. NMOD_COMPOSE_MAX_ITER, min_valid < 1, tol not finite or < 0, n_alt out of range, score or a score[m] NULL with npos > 0,
 * total_scores < 0 or below the scores the rows hold, and nmod_site_llr's rules for prm, npos and off / stride0.
 * Stops here: states exclusive at a base; reads independent; one window upstream; plain EM without acceleration (a share that goes to the
 * boundary converges slowly: raise max_iter or accept NOT_CONVERGED); no interval on the shares; p_m's law as said above. */
#define NMOD_COMPOSE_MAX_ITER 2000
enum { NMOD_COMPOSE_TOO_FEW = 1, NMOD_COMPOSE_NO_STATE = 2, NMOD_COMPOSE_NOT_CONVERGED = 4, NMOD_COMPOSE_DEGENERATE = 8,
       NMOD_COMPOSE_TOO_LARGE = 32 };
typedef struct nmod_compose_opts { int32_t struct_size, max_iter, min_valid, reserved; double tol; } nmod_compose_opts;
typedef struct nmod_compose_out { int32_t struct_size; int32_t reserved;
  double *pi, *ll, *stat, *stat_m, *p_m;                       /* n_alt + 1, 1, 1, n_alt, n_alt planes of npos */
  int32_t *n_valid, *n_partial, *iters; uint8_t *open_mask, *status; /* npos each */
  double* resp;                                                /* n_alt + 1 planes of total_scores */ } nmod_compose_out;
int nmod_site_compose(const nmod_params* prm, int64_t npos, int64_t total_scores, int32_t n_alt, const double* const* score,
                      const int64_t* off /* or prm->stride0 */, const nmod_compose_opts* opts, const nmod_compose_out* out);
int64_t nmod_site_compose_stage_reads(int32_t n_alt);         /* reads of a row up to which the workgroup form keeps its weights in LDS */

/* The modified shares of two samples compared per site: each sample's estimate, the pooled one, the likelihood-ratio test of
 * pi0 = pi1 and the profile-likelihood interval of delta = pi1 - pi0 (K15; the reference project has no such step).  Per site two
 * rows of float64 window sums, as nmod_site_stoich takes one: row 0 (sample 0, the control condition) from score0 by off0 or
 * prm->stride0, row 1 from score1 by off1 or prm->stride1; the two may differ in length.  Memspaces, the NULL and struct_size rules:
 * those of nmod_site_stoich.
 *   Per row X, K14's quantities unchanged: a score is VALID iff fabs(s) <= DBL_MAX, n_X = the valid scores; t = -expm1(-fabs(s)) with
 *     the side of s; S_X(pi), D_X(pi), g_X(pi) are K14's EVALUATION over row X, each row's sums on their own.
 *   No estimate (NaN outputs, iters 0, n_valid0 / n_valid1 still written):
 *       NMOD_DIFF_TOO_LARGE      either row beyond NMOD_MAX_DEEP scores (n_valid0 = n_valid1 = 0)
 *       NMOD_DIFF_TOO_FEW        n_0 < min_valid or n_1 < min_valid
 *       NMOD_DIFF_FLAT           otherwise, the sum of t is 0 in either row
 *   pi0, pi1: K14's estimate of each row alone, by the same rule: 0 iff S(0) <= 0, else 1 iff S(1) >= 0, else the root of S by K14's
 *     BRACKETED ITERATION on (0, 1) with its stop test.
 *   pi_pool: the same rule and iteration on S_0 + S_1 with D_0 + D_1 as the slope (x' = x + (S_0 + S_1) / (D_0 + D_1)).
 *     iters = the evaluations the iteration for pi_pool made (0 at either end).  NMOD_DIFF_POOL_AT_END: pi_pool is 0 or 1.
 *   stat = max(2 (g^ - g_pool), 0) with g^ = g_0(pi0) + g_1(pi1), g_pool = g_0(pi_pool) + g_1(pi_pool); the sums of s of K14's l
 *     cancel between the two: no inf - inf.  p_diff = max(erfc(sqrt(stat / 2)), DBL_MIN), the chi2_1 tail.  With pi_pool at an end
 *     the null sits on the boundary and the tail is conservative.
 *   delta = pi1 - pi0.
 *   The interval of delta.  For d in [-1, 1]: I(d) = [max(0, -d), min(1, 1 - d)], the pair at (x, d) is (pi0, pi1) =
 *     (x, min(max(x + d, 0), 1)), and h(d) = g_0(x*) + g_1(x* + d) at the INNER maximiser x*: the lower end of I(d) iff
 *     S_0 + S_1 <= 0 at the pair there; else the upper end iff S_0 + S_1 >= 0 there; else the root of S_0(x) + S_1(x + d) in I(d) by
 *     the bracketed iteration (slope D_0 + D_1).  h is concave, h(delta) = g^, h(0) = g_pool.  The interval is
 *     {d : 2 (g^ - h(d)) <= ci_drop}:  delta_lo = -1 iff 2 (g^ - (g_0(1) + g_1(0))) <= ci_drop, else the root in (-1, delta);
 *     delta_hi = 1 iff 2 (g^ - (g_0(0) + g_1(1))) <= ci_drop, else the root in (delta, 1).  The OUTER roots run K14's bracketed
 *     iteration for pi_lo / pi_hi with H(d) = 2 (g^ - h(d)) in the place of h and the envelope slope S_1(x* + d) in the place of S:
 *         delta_lo: right iff H(d) > ci_drop;   delta_hi: right iff H(d) <= ci_drop;   d' = d + (H - ci_drop) / (2 S_1(x* + d))
 *     where x* is interior; where x* is an end of I(d) the step is the bisection step d' = a + 0.5 (b - a).  Every outer evaluation
 *     runs its own inner iteration from the midpoint of I(d).  max_iter bounds every root, inner and outer, on its own; one still
 *     running then sets NMOD_DIFF_NOT_CONVERGED, the values are written all the same.  With delta_lo and delta_hi both NULL no
 *     interval root is run.
 *   stat is the profile deviance at d = 0: p_diff <= alpha and "0 outside the interval at level 1 - alpha" are one statement.
 *   Outputs (npos each; a NULL member is skipped; requesting fewer never changes the bits of the others): doubles pi0, pi1, pi_pool,
 *     delta, delta_lo, delta_hi, stat, p_diff; int32 n_valid0, n_valid1, iters; uint8 status.  No per-read posterior: K14 has it.
 * Sums as in K14.  The class of a site follows the longer of its rows: both up to NMOD_DIFF_SMALL scores: 16 lanes; up to
 * NMOD_DIFF_WAVE: a wave; beyond: a workgroup.  A site's bits depend on its two rows alone, not on the batch, the order of the sites,
 * CSR versus stride, the memspace or the outputs asked for.  Reads struct_size, device, stream, memspace, stride0, stride1 of prm.
 * NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no host read and no synchronisation.  npos == 0 is NMOD_OK.
 * NMOD_ERR_INVALID_ARG before any device work: nmod_site_stoich's refusals, for both rows' arguments.
 * Limits: two conditions only, no replicates or covariates; the reads are treated as independent; both k-mer tables are taken as
 * right; each strand is its own site; the chi2_1 law is asymptotic and slightly liberal at low coverage (of 40 000 simulated null pairs,
 * rejected at the 5 % level: 0.050 at 20 v 20 reads, levels 1 sd apart, pi 0.3; 0.053 at 200 v 200, 1 sd, 0.3; 0.052 at 200 v 200, 3 sd,
 * 0.5; 0.057 at 20 v 20, 3 sd, 0.5; 0.064 at 10 v 10, 3 sd, 0.5; 0.063 at 200 v 200, 3 sd, 0.02; below 0.001 at pi 0 and at pi 1:
 * tests/test_site_diff.py, profiles/site_diff.txt). */
#define NMOD_DIFF_SMALL 128                /* scores of the longer row up to which 16 lanes compute a site */
#define NMOD_DIFF_WAVE 512                 /* ... up to which one wave does (a workgroup beyond) */
enum { NMOD_DIFF_TOO_FEW = 1, NMOD_DIFF_FLAT = 2, NMOD_DIFF_NOT_CONVERGED = 4, NMOD_DIFF_POOL_AT_END = 8, NMOD_DIFF_TOO_LARGE = 32 };
typedef struct nmod_diff_opts { int32_t struct_size, max_iter, min_valid, reserved; double tol, ci_drop; } nmod_diff_opts;
typedef struct nmod_diff_out { int32_t struct_size; int32_t reserved;
  double *pi0, *pi1, *pi_pool, *delta, *delta_lo, *delta_hi, *stat, *p_diff; int32_t *n_valid0, *n_valid1, *iters; uint8_t* status;
} nmod_diff_out;
int nmod_site_diff(const nmod_params* prm, int64_t npos, const double* score0, const int64_t* off0 /* or prm->stride0 */,
                   const double* score1, const int64_t* off1 /* or prm->stride1 */,
                   const nmod_diff_opts* opts, const nmod_diff_out* out);

/* The modified shares of two REPLICATED conditions compared per site: every replicate's estimate, the two condition-level estimates
 * and their test as nmod_site_diff gives them for the pooled reads, the heterogeneity of the replicates inside their conditions, and
 * a test and an interval of delta that carry the dispersion between replicates (K24; the reference project has no such step).  An
 * analysis of deviance: the likelihood-ratio statistic of the conditions over the mean deviance between replicates, F on (1, G - 2).
 *   Input.  Per site G = nsamples rows of float64 window sums, CSR only: one `score` array and off[npos * G + 1], row i * G + g for
 *     site i and sample g.  The first `ncontrol` samples of every site are condition 0, the rest condition 1:
 *     3 <= G <= NMOD_REP_MAX_SAMPLES, 1 <= ncontrol <= G - 1 (G = 2 is refused: that is nmod_site_diff).  The two condition
 *     SUPER-ROWS of a site are therefore contiguous: off[i G] .. off[i G + ncontrol] and off[i G + ncontrol] .. off[(i + 1) G].
 *   Per score, K14's quantities unchanged: VALID, the signed t, the EVALUATION (S, D, g), the estimate rule (0 iff S(0) <= 0, else 1 iff
 *     S(1) >= 0, else the root), the BRACKETED ITERATION and its stop test; contraction is off for the unit.
 *   No estimate (NaN outputs, iters 0, n_valid still written):
 *       NMOD_REP_TOO_LARGE       a super-row beyond NMOD_MAX_DEEP scores (n_valid 0 in every sample)
 *       NMOD_REP_TOO_FEW         any sample with fewer than min_valid valid scores: every replicate carries an estimate, and the
 *                                degrees of freedom are G - 2 at every site
 *       NMOD_REP_FLAT            otherwise, the sum of t is 0 in any sample
 *   Three nested fits per site.
 *     Saturated:  pi_s[g] = K14's estimate of sample row g alone;  g_sat = sum_g g_g(pi_s[g]), summed in ascending g.
 *     Condition:  pi0, pi1, pi_pool, delta, stat_cond, p_cond, iters are exactly nmod_site_diff's pi0, pi1, pi_pool, delta, stat,
 *       p_diff, iters for the two super-rows;  g_cond = g_0(pi0) + g_1(pi1).
 *     Heterogeneity:  df = G - 2;  stat_het = max(2 (g_sat - g_cond), 0);  p_het = max(chi2_df tail of stat_het, DBL_MIN), with
 *       x = stat_het / 2:  even df: exp(-x) sum_{m < df/2} x^m / m!;  odd df: erfc(sqrt(x)) + exp(-x) sum_{j=1..(df-1)/2}
 *       x^(j - 1/2) / Gamma(j + 1/2);  phi = stat_het / df, the dispersion of the site.
 *   The replicate-aware test.  phi_used = max(phi, opts->phi_floor);  F = stat_cond / phi_used;  p_rep = max(the two-sided Student t
 *     tail of sqrt(F) on df degrees of freedom, DBL_MIN): the F(1, df) tail.  stat_cond == 0: p_rep = 1.  Otherwise phi_used == 0:
 *     p_rep = DBL_MIN with NMOD_REP_PHI_ZERO.  phi_floor = 0 is the default of the Python layers; phi_floor = 1 never lets the
 *     dispersion fall below the binomial one (methylKit's rule) and is very conservative.  phi_floor must be finite and >= 0.
 *   The interval of delta: nmod_site_diff's profile-likelihood interval of the two super-rows at the drop phi_used * ci_drop (one
 *     multiplication).  The caller passes ci_drop = the ci_level quantile of F(1, df).  phi_used == 0: the drop is 0, the interval
 *     is the point delta_lo = delta_hi = delta and no interval root is run.  With delta_lo and delta_hi both NULL none is run either.
 *   Status bits: NMOD_REP_TOO_FEW, FLAT, NOT_CONVERGED (any root of the three fits or of the interval still running at max_iter; the
 *     values are written all the same), POOL_AT_END, TOO_LARGE with nmod_site_diff's values, and NMOD_REP_PHI_ZERO.
 *   Outputs (a NULL member is skipped; requesting fewer never changes the bits of the others): doubles pi_s[npos * G] and, npos each,
 *     pi0, pi1, pi_pool, delta, delta_lo, delta_hi, stat_cond, p_cond, stat_het, p_het, phi, p_rep; int32 n_valid[npos * G], iters;
 *     uint8 status.
 * Sums.  The condition level has nmod_site_diff's bits: the class of a site follows the longer super-row with its steps
 * (NMOD_DIFF_SMALL: 16 lanes, NMOD_DIFF_WAVE: a wave, a workgroup beyond) and each class keeps its lane layout, reduction order and
 * LDS stage, so that pi0, pi1, pi_pool, stat_cond, p_cond, iters and, at the same drop, delta_lo / delta_hi are the bytes
 * nmod_site_diff gives for the concatenated rows.  A sample is an index range of its super-row: an element outside it enters the
 * sample's sums as t = 0, which adds exactly 0 to S, D and g, and the G roots run one after the other over the data already resident.
 * A sample's sums run in the sample's own order (the lane partials are rotated by its offset before they are reduced): pi_s[g] has the
 * same bits wherever in its super-row sample g lies, so permuting the samples inside a condition permutes pi_s bit for bit.
 * A site's bits depend on its rows, G and ncontrol alone, not on the batch, the order of the sites, the memspace or the outputs asked
 * for; no float atomics.  Reads struct_size, device, stream, memspace of prm.  NMOD_MEM_DEVICE: everything is enqueued on
 * prm->stream, no host read and no synchronisation.  npos == 0 is NMOD_OK.
 * NMOD_ERR_INVALID_ARG before any device work: nmod_site_diff's refusals (opts, out, max_iter, min_valid, tol, ci_drop, prm, npos, a
 * decreasing host off), off NULL, nsamples outside 3 .. NMOD_REP_MAX_SAMPLES, ncontrol outside 1 .. nsamples - 1, npos * nsamples
 * beyond INT32_MAX - 1, phi_floor not finite or < 0.
 * Limits: two conditions, no covariates or pairing; every sample must cover the site (a site with a thin replicate has no estimate);
 * one dispersion per site, neither shared between sites nor shrunk, so that F on as few as 1 degree of freedom (2 v 1) has little
 * power; both k-mer tables are taken as right; the F law is an approximation.  Measured with the numpy restatement on seeded null
 * sites (share 0.3 in both conditions, levels 2 sd apart, replicates of 50 reads whose shares are drawn Beta with intraclass
 * correlation rho; rejected at the 5 % level, of 400 sites per cell: tests/test_site_diff_rep.py, profiles/site_diff_rep.txt):
 *     3 v 3, rho 0:     p_cond 0.045   p_rep 0.040   p_rep at phi_floor 1 0.005   p_het 0.043
 *     3 v 3, rho 0.05:  p_cond 0.203   p_rep 0.053   p_rep at phi_floor 1 0.025   p_het 0.375
 *     3 v 3, rho 0.15:  p_cond 0.403   p_rep 0.058   p_rep at phi_floor 1 0.050   p_het 0.768
 *     2 v 2, rho 0.1:   p_cond 0.278   p_rep 0.028   p_rep at phi_floor 1 0.003   p_het 0.523 */
#define NMOD_REP_MAX_SAMPLES 16            /* the largest G */
enum { NMOD_REP_TOO_FEW = 1, NMOD_REP_FLAT = 2, NMOD_REP_NOT_CONVERGED = 4, NMOD_REP_POOL_AT_END = 8, NMOD_REP_PHI_ZERO = 16,
       NMOD_REP_TOO_LARGE = 32 };
typedef struct nmod_rep_opts { int32_t struct_size, max_iter, min_valid, reserved; double tol, ci_drop, phi_floor; } nmod_rep_opts;
typedef struct nmod_rep_out { int32_t struct_size; int32_t reserved;
  double *pi_s /* npos * G */, *pi0, *pi1, *pi_pool, *delta, *delta_lo, *delta_hi, *stat_cond, *p_cond, *stat_het, *p_het, *phi, *p_rep;
  int32_t *n_valid /* npos * G */, *iters; uint8_t* status;
} nmod_rep_out;
int nmod_site_diff_rep(const nmod_params* prm, int64_t npos, int32_t nsamples, int32_t ncontrol, const double* score, const int64_t* off,
                       const nmod_rep_opts* opts, const nmod_rep_out* out);

/* The dispersions of nmod_site_diff_rep shrunk across sites: an empirical-Bayes prior law of phi fitted over all sites of a call
 * (nmod_rep_prior), and nmod_site_diff_rep with every site's phi replaced by its posterior value under that law and its test taken on
 * the degrees of freedom the prior adds (nmod_site_diff_rep_mod) (K25; the reference project has no such step).  limma's, DSS's and
 * edgeR's step: with 2 or 4 degrees of freedom per site the denominator of F is mostly noise, and all sites together say how much.
 *
 * nmod_rep_prior.  Inputs: df = G - 2 in 1 .. NMOD_REP_MAX_SAMPLES - 2; phi[npos] (double) and status[npos] (uint8) as
 *   nmod_site_diff_rep wrote them; ci_level strictly inside (0, 1).  Output: the RECORD prior[NMOD_REP_PRIOR_WORDS], 8 doubles.  All
 *   arrays in the memspace of prm.
 *   A site ENTERS THE FIT iff its status has none of NMOD_REP_TOO_FEW, FLAT, TOO_LARGE and phi is finite and phi > 0; n of them.  A
 *   site with none of these bits and phi <= 0 is a ZERO (nmod_site_diff_rep clamps stat_het at 0: such sites exist); a NaN phi is
 *   neither.
 *   The fit is limma's fitFDist at equal degrees of freedom (phi ~ s0^2 F(df, d0); psi, psi' the di- and trigamma functions):
 *     e_i = ln phi_i - psi(df / 2) + ln(df / 2)          (in this order: two roundings after the logarithm)
 *     emean = sum e_i / n
 *     evar = sum (e_i - emean)^2 / (n - 1) - psi'(df / 2)        (the centred squares in a second pass over phi)
 *     evar > 0:   d0 = 2 psi'^-1(evar),   s0^2 = exp(emean + psi(d0 / 2) - ln(d0 / 2))
 *     evar <= 0:  d0 = +inf,              s0^2 = exp(emean)      (the sites differ no more than chi2_df alone makes them)
 *     n < 2:      d0 = 0 ("no prior"),    s0^2 = NaN, evar = NaN (emean: the one e, or NaN)
 *   psi'^-1 is a Newton iteration on 1 / psi' from 1/2 + 1/x; it stops after the first step of relative size below 1e-8 (what is
 *   left is of the order of its square) or after 50 steps; x > 1e7: 1 / sqrt(x), x < 1e-6: 1 / x.
 *   The record, in this order:  d0;  s0^2;  df_tot = df + d0;  ci_drop, the ci_level quantile of F(1, df_tot), found by bisecting the
 *   two-sided Student t tail for real df_tot down to neighbouring doubles (df_tot = +inf: norm_isf((1 - ci_level) / 2)^2, the chi2_1
 *   quantile; d0 = 0: the F(1, df) quantile);  n (n_used);  the number of zeros (n_zero);  emean;  evar.
 *   Sums.  A CHUNK is NMOD_REP_PRIOR_CHUNK consecutive sites.  A workgroup of 256 threads sums a chunk: thread t its sites t, t + 256,
 *   ... in ascending order, the threads joined by the wave and workgroup sums; one workgroup then adds the chunks' words in ascending
 *   chunk order (thread t a contiguous run of chunks, the runs joined in ascending t), and does the scalar solve — psi, psi', psi'^-1,
 *   s0^2 and the quantile — in one thread on the device.  No float atomics; nothing depends on the size of the grid: for given arrays
 *   the record has the same bits in every run and in both memspaces.  NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no host
 *   read and no synchronisation.
 *   NMOD_ERR_INVALID_ARG before any device work: prm as for nmod_site_diff_rep, a NULL prior, NULL phi or status with npos > 0, df out
 *   of range, ci_level outside (0, 1) or NaN, npos < 0 or beyond INT32_MAX - 1.  npos == 0 is NMOD_OK and gives the n < 2 record.
 *
 * nmod_site_diff_rep_mod: nmod_site_diff_rep's arguments, then prior (the record, in the memspace of prm; read by the kernels, never
 *   by the host) and phi_post (double[npos] or NULL, a trailing output: nmod_rep_out keeps its size).  What changes:
 *     d0 == 0:     phi_post = phi
 *     d0 == +inf:  phi_post = s0^2
 *     otherwise:   phi_post = (d0 s0^2 + df phi) / (d0 + df)      (two products, two sums, one division; contraction is off)
 *     phi_used = max(phi_post, opts->phi_floor);  F = stat_cond / phi_used;  p_rep = max(the two-sided Student t tail of sqrt(F) on
 *     df_tot = prior[2] degrees of freedom, DBL_MIN); df_tot = +inf: erfc(sqrt(F / 2)).  stat_cond == 0: p_rep = 1; otherwise
 *     phi_used == 0 (d0 == 0 or s0^2 == 0, and a floor of 0): p_rep = DBL_MIN with NMOD_REP_PHI_ZERO.
 *     The interval of delta is taken at the drop phi_used * prior[3]; opts->ci_drop is checked as before and then IGNORED.
 *   Everything else — pi_s, pi0, pi1, pi_pool, delta, stat_cond, p_cond, stat_het, p_het, phi, n_valid, iters — has the bytes
 *   nmod_site_diff_rep gives for the same rows, and with a d0 == 0 record so have p_rep and, at ci_drop = prior[3], the interval.
 *   The record's contents are not validated by the entry (they may exist on the device alone).  A NaN in d0 or df_tot, a NaN in s0^2
 *   while d0 > 0, or a negative value among the record's first four words gives EVERY site, with or without an estimate, NaN p_rep,
 *   phi_post, delta_lo and delta_hi and the status bit NMOD_REP_BAD_PRIOR; no interval root is run and NMOD_REP_PHI_ZERO is not set.
 *   Refusals: nmod_site_diff_rep's, and a NULL prior.
 * Limits: the prior has no trend in coverage or share; all sites carry the same df; zeros are left out of the fit
 * (and moderated all the same); no robust (winsorised) fit: a few wild sites lower d0 for all; the F(1, df_tot) law of a moderated
 * quasi-likelihood ratio is an approximation.  The three fits run twice (once for phi, once moderated).  Measured with the numpy
 * restatement (tests/diff_mod_ref.py) on nmod_site_diff_rep's seeded cells, the prior fitted per cell, rejected at the 5 % level of
 * 400 sites (tests/test_site_diff_mod.py, profiles/site_diff_mod.txt); `planted`: the same cell with a planted difference:
 *     3 v 3, rho 0, null:    p_cond 0.045  p_rep 0.040  moderated 0.045
 *     3 v 3, rho 0, planted: p_cond 0.368  p_rep 0.250  moderated 0.363
 *     3 v 3, rho 0.05, null:    p_cond 0.203  p_rep 0.053  moderated 0.048
 *     3 v 3, rho 0.05, planted: p_cond 0.695  p_rep 0.310  moderated 0.425
 *     3 v 3, rho 0.15, null:    p_cond 0.403  p_rep 0.058  moderated 0.053
 *     3 v 3, rho 0.15, planted: p_cond 0.903  p_rep 0.328  moderated 0.525
 *     2 v 2, rho 0.1, null:    p_cond 0.278  p_rep 0.028  moderated 0.033
 *     2 v 2, rho 0.1, planted: p_cond 0.985  p_rep 0.400  moderated 0.875
 * (planted differences of the share: +0.12, +0.22, +0.36, +0.50, chosen so that p_rep rejects a quarter to two fifths of the sites.
 * In six of the eight fits evar <= 0 and d0 = +inf: 400 sites of one cell do not tell their dispersions apart, and the test is then
 * the normal one at the common dispersion s0^2.) */
#define NMOD_REP_PRIOR_WORDS 8
#define NMOD_REP_PRIOR_CHUNK 1024          /* sites per chunk of nmod_rep_prior's sums */
enum { NMOD_REP_BAD_PRIOR = 64 };
int nmod_rep_prior(const nmod_params* prm, int64_t npos, int32_t df, const double* phi, const uint8_t* status, double ci_level,
                   double* prior);
int nmod_site_diff_rep_mod(const nmod_params* prm, int64_t npos, int32_t nsamples, int32_t ncontrol, const double* score,
                           const int64_t* off, const nmod_rep_opts* opts, const nmod_rep_out* out, const double* prior, double* phi_post);

/* Same-read co-occurrence of modification calls at pairs of sites: per pair the 2 x 2 table of the reads that have a call at both
 * sites, its log odds ratio, phi and the two-sided exact test (K16; the reference project has no such step).  K11 .. K15 reduce over
 * the reads of one position; this entry keeps the read: it walks the reads and counts, per pair of candidate sites, the reads by
 * their two calls.  Memspaces, the NULL and struct_size rules: those of nmod_read_llr and nmod_site_stoich.
 *   Inputs.  Reads in nmod_pivot_reads' layout: nreads, cs[r] (int32, 2 * chrom index + (strand == '-')), start[r] (int64, >= 0),
 *     roff[nreads + 1] (int64); score: float64, one per event in read direction (K13's llr_win).  Candidate sites: nsites keys
 *     (int64, cs << 40 | pos), strictly ascending.  Event i of a read of n events lies at position start + i on '+' and at
 *     start + n - 1 - i on '-' (nmod_pivot_reads' rule); a read COVERS the sites whose cs is its own and whose pos lies in
 *     [start, start + n - 1].
 *   The CALL of read r at a site it covers, with L the score of its event at that position:  MOD (1) iff L >= thr;  CAN (0) iff
 *     L <= -thr;  otherwise none (a NaN is none).  thr is finite and > 0, as in K13.
 *   PAIRS.  Site b is a partner of site a iff b > a, key_b >> 40 == key_a >> 40 and pos_b - pos_a <= max_dist, max_dist in
 *     1 .. NMOD_PAIRS_MAX_DIST.  The partners of a are contiguous in key order: pair (a, b) has the index poff[a] + (b - a - 1),
 *     poff[nsites + 1] (int64) being the exclusive scan of the partner counts, poff[nsites] = npairs.
 *   nmod_pair_index computes poff (on prm->stream) and synchronises the stream once to return *npairs_out (a host pointer), as
 *     nmod_select_tested does.  NMOD_ERR_INVALID_ARG: nsites outside 0 .. 2^31 - 2, max_dist out of range, a NULL pointer, host keys
 *     that do not strictly ascend (nothing is enqueued), npairs > 2^31 - 1 (poff is written by then).  Device keys are not checked.
 *     Reads struct_size, device, stream, memspace of prm.
 *   nmod_site_pairs.  A read takes part in pair j = (a, b) iff it has a call at both sites: counts[4 j + 2 call_a + call_b] += 1.
 *     The table of pair j is (n11, n10, n01, n00) = counts[4 j + 3], [4 j + 2], [4 j + 1], [4 j]: the first index is site a's call.
 *     counts are int32, zeroed by the entry on the stream.  With N = n11 + n10 + n01 + n00, r1 = n11 + n10, r0 = N - r1,
 *     c1 = n11 + n01, c0 = N - c1:
 *       log_or = log(((n11 + 0.5) (n00 + 0.5)) / ((n10 + 0.5) (n01 + 0.5)))       (both products exact below 2^26 reads)
 *       se     = sqrt(((1 / (n11 + 0.5) + 1 / (n10 + 0.5)) + 1 / (n01 + 0.5)) + 1 / (n00 + 0.5))
 *       phi    = double(n11 n00 - n10 n01) / sqrt(double(r1 r0) * double(c1 c0)), the integer products in 64 bits; NaN iff a margin is 0
 *       first[j] = a, second[j] = b (int32)
 *       p_fisher, the two-sided exact test conditional on the margins:  lo = max(0, r1 + c1 - N), hi = min(r1, c1), the support
 *         has L = hi - lo + 1 tables x = n11;  mode = ((r1 + 1) (c1 + 1)) / (N + 2) in 64-bit integer division, clamped into
 *         [lo, hi];  w(mode) = 1;  w(x + 1) = w(x) * (double((c1 - x) (r1 - x)) / double((x + 1) (N - c1 - r1 + x + 1))) upwards and
 *         w(x - 1) = w(x) * (double(x (N - c1 - r1 + x)) / double((c1 - x + 1) (r1 - x + 1))) downwards: one correctly rounded division
 *         and one multiplication per step.  The integer products are taken in 64 bits and are exact as doubles while N < 2^26 (they
 *         stay below 2^52); up to 2^31 - 1 reads they still fit 64 bits and are rounded once more.  With cut = w(n11) * (1 + 1e-7) (the
 *         tie slack of R's fisher.test):  p = min(T / S, 1), then max(p, DBL_MIN), where S is the sum of every w(x) and T the sum of
 *         those with w(x) <= cut.  L = 1 gives p = 1.  No weight overflows: every ratio on the far side of the mode is <= 1; a
 *         w(n11) that underflows to 0 gives DBL_MIN.
 *       Orders.  L <= NMOD_PAIRS_THREAD_MAX (one thread): U = the w(x) above the mode added in ascending x from 0.0, D = those below
 *         it in descending x from 0.0, S = (1.0 + U) + D; T likewise over the weights <= cut (the mode's 1.0 replaced by 0.0 when
 *         1.0 > cut).  Beyond (one wave): the elements of each side are dealt to the lanes in tiles of 64, element mode + 1 + 64 t +
 *         lane (mode - 1 - 64 t - lane below), an element outside the support having the ratio 0; the weights of a tile are the
 *         inclusive product scan of its ratios over the lanes (steps 1, 2, 4, 8, 16, 32: v[l] = v[l] * v[l - d] for l >= d, the old
 *         values) times the carry, the weight of lane 63 of the tile before (1.0 for the first).  A lane adds its weights in tile
 *         order, the side above first, then the side below; the 64 lane sums are added as the library's wave sum does (partners
 *         l ^ 1, l ^ 2, then the mirror of each 8 lanes, then of each 16; the four rows of 16 in order from 0.0); S = 1.0 + that
 *         sum, T likewise.  The class of a pair depends on its own L alone: a pair's bits depend on its table alone.
 *     Status: NMOD_PAIRS_TOO_FEW: N < opts->min_reads (min_reads >= 1): log_or, se, phi, p_fisher are NaN, the counts (and first,
 *       second) are still written.  NMOD_PAIRS_DEGENERATE: a margin is 0: phi is NaN and p_fisher = 1 (NaN under TOO_FEW).
 *     Outputs (a NULL member is skipped; requesting fewer never changes the bits of the others): counts int32[4 npairs]; first,
 *       second int32[npairs]; log_or, se, phi, p_fisher double[npairs]; status uint8[npairs].  p_fisher is per pair and unadjusted:
 *       nmod_fdr_adjust takes it (a NaN is left out of the family).
 *     opts->flags: NMOD_PAIRS_FORCE_DIRECT: the read kernel adds to the counters in device memory even where the call would keep
 *       its table in LDS (npairs <= NMOD_PAIRS_LDS_MAX: every workgroup sums into an LDS table and flushes its non-zero counters at
 *       the end).  Integer atomics in both: the counts do not depend on the form, the order of the reads, or the memspace.
 *     Reads struct_size, device, stream, memspace of prm.  NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no host read
 *     and no synchronisation; key, poff and the reads are not checked (an event index outside its read or a pair index outside
 *     [0, npairs) is skipped).  NMOD_MEM_HOST: one staged copy.  nreads == 0: zero counts; npairs == 0: NMOD_OK, nothing to do.
 *     NMOD_ERR_INVALID_ARG before any device work: nreads outside 0 .. 2^31 - 1, nsites outside 0 .. 2^31 - 2, npairs outside
 *     0 .. 2^31 - 1, thr not finite or <= 0, min_reads < 1, unknown flags, a NULL input that is needed, host offsets that decrease,
 *     host keys that do not strictly ascend, host poff that does not start at 0, ascend and end at npairs.
 * Limits: hard calls only, no posterior-weighted table; pairs only; both sites on one (chrom, strand); a molecule sequenced twice
 * counts twice. */
#define NMOD_PAIRS_MAX_DIST 65536          /* largest max_dist */
#define NMOD_PAIRS_LDS_MAX 2048            /* pairs up to which the read kernel keeps the call's table in LDS (32 KiB) */
#define NMOD_PAIRS_THREAD_MAX 64           /* tables of a pair's support up to which one thread computes p_fisher (a wave beyond) */
#define NMOD_PAIRS_FORCE_DIRECT 1          /* opts->flags */
enum { NMOD_PAIRS_TOO_FEW = 1, NMOD_PAIRS_DEGENERATE = 2 };
typedef struct nmod_pairs_opts { int32_t struct_size, min_reads, flags, reserved; double thr; } nmod_pairs_opts;
typedef struct nmod_pairs_out { int32_t struct_size; int32_t reserved;
  int32_t *counts, *first, *second; double *log_or, *se, *phi, *p_fisher; uint8_t* status;
} nmod_pairs_out;
int nmod_pair_index(const nmod_params* prm, int64_t nsites, const int64_t* key, int64_t max_dist, int64_t* poff_out,
                    int64_t* npairs_out /* host */);
int nmod_site_pairs(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                    const double* score, int64_t nsites, const int64_t* key, const int64_t* poff, int64_t npairs,
                    const nmod_pairs_opts* opts, const nmod_pairs_out* out);

/* Soft same-read linkage of pairs of sites from window sums: per pair the two marginal modified shares, the linkage D of the two
 * hidden states with a likelihood interval, the correlation r and the likelihood-ratio test of independence (K18; the reference
 * project has no such step).  K16 counts a read at a site only where its window sum lies beyond +-thr; here every read with a VALID
 * score at both sites takes part with its likelihood, as in K14.  Memspaces, the NULL and struct_size rules: those of nmod_site_pairs
 * and nmod_site_stoich.
 *   ROWS.  Reads, scores, keys, poff and npairs are nmod_site_pairs' arguments, under its rules and refusals.  A read takes part in
 *     pair j = (a, b) iff it covers both sites and its scores there, s_a and s_b, are VALID (fabs(s) <= DBL_MAX, as in K14).  The row of
 *     pair j holds those reads IN ASCENDING READ INDEX: rows prow_off[j] .. prow_off[j + 1] - 1 of sa, sb (float64) and read (int32).
 *     nmod_pair_rows_count computes prow_off[npairs + 1] (int64; integer atomics and a scan, on prm->stream) and synchronises the
 *       stream once to return *nrows_out (a host pointer), as nmod_pair_index does.  NMOD_ERR_INVALID_ARG: nmod_site_pairs' refusals
 *       for the shared arguments, a NULL prow_off_out or nrows_out, nrows > 2^31 - 1 (prow_off is written by then).
 *     nmod_pair_rows_fill writes sa, sb, read (nrows each; a NULL one is skipped).  Every read takes the next free row of its pair by
 *       an integer atomic, then the 64-bit keys pair << 32 | read are sorted (radix_sort.hpp) and the scores gathered: no float
 *       atomics, and two runs give the same bytes in either memspace.  NMOD_ERR_INVALID_ARG: the same refusals, nrows outside
 *       0 .. 2^31 - 1, a NULL prow_off, host prow_off that does not start at 0, ascend and end at nrows.  Device prow_off is not
 *       checked: a row outside its pair's range is skipped.  nrows == 0: NMOD_OK, nothing to do.
 *   nmod_pair_linkage(prm, npairs, sa, sb, prow_off, opts, out): per pair its row of (s_a, s_b); a read with either score invalid takes
 *     no part (it counts as t = 0 in both rows), n = the reads that do.  The joint law of the two hidden states (1: modified):
 *         pi11 = pa pb + D,   pi10 = pa qb - D,   pi01 = qa pb - D,   pi00 = qa qb + D,     q = 1 - p.
 *     A TWO-STAGE estimate: the margins from the marginal likelihoods, then D with the margins fixed.
 *     Stage 1.  pa = K14's estimate over the row of s_a, pb over the row of s_b: the same rule (0 iff S(0) <= 0, else 1 iff S(1) >= 0,
 *       else the root), the same EVALUATION, BRACKETED ITERATION and stop test, in the same order of operations and of the sums: pa and
 *       pb have the bits nmod_site_stoich gives for that row.  Each margin's likelihood is correctly specified whatever D is.
 *     Stage 2.  Per read u_a = K14's u at pa with the sign of the side: + t / (1 - qa t) on the plus side, - t / (1 - pa t) on the minus
 *       side; u_b likewise at pb; v = u_a * u_b.  The read's likelihood relative to independence is exactly 1 + D v.
 *       The range of D: d_min = -min(pa pb, qa qb), d_max = min(pa qb, qa pb).  One evaluation at D, contraction off, per read:
 *           dv = max(D * v, -1),   w = v / (1 + dv),   S += w,   Q += w * w,   g += log1p(dv).
 *       A zero denominator (the ends only) gives w = +-inf and g = -inf, which is wanted, as in K14.
 *       D^: d_min iff S(d_min) <= 0 (NMOD_LINK_AT_MIN); else d_max iff S(d_max) >= 0 (NMOD_LINK_AT_MAX); else the root of S in
 *       (d_min, d_max) by K14's bracketed iteration, right iff S(x) > 0, x' = x + S / Q.  iters = its evaluations (0 at either end).
 *     stat = max(2 g(D^), 0);  p_indep = max(erfc(sqrt(stat / 2)), DBL_MIN), the chi2_1 tail;  r = D^ / sqrt((pa qa) (pb qb)).
 *     The interval {d : 2 (g(D^) - g(d)) <= ci_drop}: d_lo = d_min iff that holds at d_min, else the root in (d_min, D^) by K14's pi_lo
 *       iteration (h = 2 (g(D^) - g(x)), x' = x + (h - ci_drop) / (2 S)); d_hi = d_max iff it holds at d_max, else the root in
 *       (D^, d_max) by K14's pi_hi iteration.  With d_lo and d_hi both NULL no interval root is run.  max_iter bounds each of the five
 *       roots on its own; one still running then sets NMOD_LINK_NOT_CONVERGED, the values are written all the same.
 *     Status bits:
 *       NMOD_LINK_TOO_FEW      n < min_reads: NaN outputs, iters 0 (n_valid is written)
 *       NMOD_LINK_FLAT         K14's FLAT on either margin (the sum of t of a row is 0): NaN outputs, iters 0
 *       NMOD_LINK_DEGENERATE   a margin is 0 or 1, the range of D is a point: d = d_lo = d_hi = 0, stat = 0, p_indep = 1, r = NaN, iters 0
 *       NMOD_LINK_AT_MIN, NMOD_LINK_AT_MAX, NMOD_LINK_NOT_CONVERGED   see above
 *       NMOD_LINK_TOO_LARGE    a row beyond NMOD_MAX_DEEP reads: NaN outputs, n_valid 0, iters 0
 *     Outputs (npairs each; a NULL member is skipped; requesting fewer never changes the bits of the others): doubles pa, pb, d, d_lo,
 *       d_hi, r, stat, p_indep; int32 n_valid, iters; uint8 status.  p_indep is per pair and unadjusted: nmod_fdr_adjust takes it.
 *     Sums as in K14: the lane's reads in ascending index, then the library's lane, wave and LDS reductions; no float atomics.  A row of
 *     up to NMOD_LINK_SMALL reads is computed by 16 lanes, up to NMOD_LINK_WAVE by a wave, a longer one by a workgroup (K14's steps, which
 *     the bits of pa and pb rest on; not tuned for this kernel): a pair's bits depend on its row alone, not on the batch, the order of
 *     the pairs, the memspace or the outputs asked for.  Reads struct_size, device, stream, memspace of prm.  NMOD_MEM_DEVICE:
 *     everything is enqueued on prm->stream, no host read and no synchronisation.  npairs == 0 is NMOD_OK.
 *     NMOD_ERR_INVALID_ARG before any device work: opts NULL or of another struct_size, max_iter outside 1 .. 200, min_reads < 1, tol
 *     not finite or < 0, ci_drop not finite or <= 0, npairs outside 0 .. 2^31 - 2, a NULL prow_off, NULL sa or sb where a row has a
 *     read, host prow_off that decreases.
 *   What this is and is not.  D is information-orthogonal to the margins at D = 0 (the expected cross term factorises into a
 *     zero-mean score), so stat has the chi2_1 law of the full likelihood-ratio test under independence; it never exceeds the full
 *     likelihood-ratio statistic, the margins being held at values the full fit is free to move (in a simulation of 4 000 pairs per
 *     cell against the full model by EM to 1e-11 the largest excess was 0 to rounding and the median ratio 0.96 - 0.999).  The full EM
 *     needed a median of 560 iterations at 1 sd separation and did not converge in 2 000 for 7 - 9 % of the pairs, which is why it is
 *     not what is built.  Null rejection at the 5 % level (tests/test_site_linkage.py): 0.053 at 200 reads, 3 sd, shares 0.3 / 0.5;
 *     0.057 at 20 reads, 3 sd, 0.5 / 0.5 (4 000 seeded null pairs each).  It is liberal below about 20 reads (0.068 at 10 reads, 3 sd,
 *     0.5 / 0.5) and conservative near an end of the range or at low separation (0.032 at 200 reads, 1 sd, 0.3 / 0.3; 0.024 at 200
 *     reads, 3 sd, 0.05 / 0.05).  The default min_reads of the Python layers is 20.
 * Stops at: pairs only; the reads are treated as independent; both k-mer tables are taken as right; no interval for the pi cells;
 * p_indep is unadjusted. */
#define NMOD_LINK_SMALL 256                /* reads of a row up to which 16 lanes compute it (K14's step) */
#define NMOD_LINK_WAVE 1024                /* ... up to which one wave does (a workgroup beyond) */
enum { NMOD_LINK_TOO_FEW = 1, NMOD_LINK_FLAT = 2, NMOD_LINK_NOT_CONVERGED = 4, NMOD_LINK_AT_MIN = 8, NMOD_LINK_AT_MAX = 16,
       NMOD_LINK_TOO_LARGE = 32, NMOD_LINK_DEGENERATE = 64 };
typedef struct nmod_link_opts { int32_t struct_size, max_iter, min_reads, reserved; double tol, ci_drop; } nmod_link_opts;
typedef struct nmod_link_out { int32_t struct_size; int32_t reserved;
  double *pa, *pb, *d, *d_lo, *d_hi, *r, *stat, *p_indep; int32_t *n_valid, *iters; uint8_t* status;
} nmod_link_out;
int nmod_pair_rows_count(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                         const double* score, int64_t nsites, const int64_t* key, const int64_t* poff, int64_t npairs,
                         int64_t* prow_off_out, int64_t* nrows_out /* host */);
int nmod_pair_rows_fill(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                        const double* score, int64_t nsites, const int64_t* key, const int64_t* poff, int64_t npairs,
                        const int64_t* prow_off, int64_t nrows, double* sa, double* sb, int32_t* read);
int nmod_pair_linkage(const nmod_params* prm, int64_t npairs, const double* sa, const double* sb, const int64_t* prow_off,
                      const nmod_link_opts* opts, const nmod_link_out* out);

/* Per-read two-state hidden Markov smoothing of the window sums at the candidate sites a read covers: along each molecule the posterior
 * of "modified" at every site given all the read's scores, hard states at a posterior threshold, the runs of modified sites, and the
 * read's log-likelihood under the chain and under independence (K19; the reference project has no such step).  K16 and K18 keep the
 * read but look at two sites at a time; here the whole read is one chain.  Memspaces, the NULL and struct_size rules: those of
 * nmod_site_pairs.
 *   Inputs.  Reads, score (K13's llr_win, float64, one per event in read direction) and the candidate-site keys (int64, cs << 40 | pos,
 *     strictly ascending) are nmod_site_pairs' arguments, under its rules, refusals, COVERS rule and strand-aware event index.  There
 *     are no pairs, no max_dist and no poff.
 *   ENTRIES of a read: the candidate sites it covers whose score there is VALID (fabs(s) <= DBL_MAX, as in K14), in ascending key:
 *     j = 0 .. m - 1 at positions x_j with scores s_j.  An invalid score is skipped: the chain runs over the valid neighbours with the
 *     larger gap.  m = 0 is not an error.  The entries of read r are the rows hoff[r] .. hoff[r + 1] - 1 of the per-entry outputs.
 *   Model.  opts->pi, the stationary modified share (1e-9 <= pi <= 1 - 1e-9), and opts->length, the correlation length in bases
 *     (1e-3 <= length <= 1e9).  With q = 1 - pi (formed once on the host) and d = x_j - x_(j-1) >= 1, an exact integer as a double:
 *         rho = exp(-(d / length)),   eps = -expm1(-(d / length)),
 *         T_j = [[q + pi rho, pi eps], [q eps, pi + q rho]]     rows the state at j - 1, columns the state at j;
 *     every entry is a sum of non-negative terms, nothing is formed by 1 - x.  Emissions, scaled so that the larger is 1:
 *     e_j = (exp(-max(s_j, 0)), exp(min(s_j, 0))).  Initial law (q, pi).  Contraction is off for the whole translation unit.
 *   Per entry.  post_j = P(state_j = 1 | all scores of the read's entries) by scaled forward-backward:
 *     post_j = a_j1 b_j1 / (a_j0 b_j0 + a_j1 b_j1) with a the forward and b the backward vector; a posterior, not clamped: it may be 0
 *     or 1.  site_j = the index of the site in key (int32).  state_j (uint8): 1 iff post_j >= call_post; 0 iff post_j <= 1 - call_post,
 *     that difference formed once on the host; 2 otherwise (a NaN too).  call_post lies in (0.5, 1).  state is decided from the post
 *     that is written: the two outputs agree bit for bit.
 *   Per read.  n_sites = m (int32); n_mod, n_can = the entries in state 1 and 0; n_runs = the maximal runs of consecutive entries in
 *     state 1;  ll = sum_j (log c_j + max(s_j, 0)) with c_j the forward normalisers: the chain's log-likelihood relative to "every site
 *     canonical";  ll_indep = sum_j (log(q e_j0 + pi e_j1) + max(s_j, 0)), the same under independence: 2 (ll - ll_indep) says whether
 *     the molecule carries domains, and the sum of ll over the reads is what length is chosen by.  status (uint8): NMOD_HMM_NO_SITE
 *     when m = 0 (ll = ll_indep = 0, the counts 0).
 *   Per site (int32[nsites] each, integer atomics, zeroed by the entry on the stream): site_n = the reads with an entry there,
 *     site_mod = the entries in state 1, site_can = those in state 0.
 *   ORDER of the operations.  A step is the matrix A_k = T_k diag(e_k) (T_0 = I) forwards, k = j; backwards the transpose of
 *     T_j diag(e_j) for j = m - k, and I at k = 0: step k of the backward scan belongs to entry m - 1 - k.  Both passes are one scan
 *     over steps k = 0 .. m - 1 with a row vector x: x_k = x_(k-1) A_k, from (q, pi) forwards and (1, 1) backwards; a_j = x_j forwards,
 *     b_j = x_(m-1-j) backwards.  A product of two matrices is c_rc = l_r0 r_0c + l_r1 r_1c and a vector step y_c = x_0 m_0c + x_1 m_1c:
 *     two multiplications and one addition each, no fused operation.  Every product is then scaled by 2^-ex, ex the exponent frexp
 *     gives for its largest entry, and ex is added to an integer exponent: scaling adds no rounding (unless an entry turns subnormal).
 *     A read of up to NMOD_HMM_WAVE_MAX entries is computed by T = 64 threads, a longer one by T = 256, in tiles of T * NMOD_HMM_CHUNK
 *     steps: thread t of the tile at k0 owns steps k0 + t * NMOD_HMM_CHUNK + c, c = 0 .. NMOD_HMM_CHUNK - 1 (a step beyond m - 1 is I).
 *     It multiplies its steps left to right into P_t.  The 64 lanes of a wave scan those products: for d = 1, 2, 4, 8, 16, 32 lane l >= d
 *     takes P_l = P_(l-d) P_l from the old values.  The vector in front of a thread's chunk is the tile's carry, times the scanned
 *     product of lane 63 of every wave in front of its own in ascending order, times that of the lane before it; from there it replays
 *     its steps one vector step each.  The carry of the next tile is the vector of thread T - 1 after its chunk.
 *     ll = (log(x_0 + x_1) + E ln 2) + S, x and E the last forward carry and its exponent, ln 2 = 0.6931471805599453, S the sum of
 *     max(s_j, 0); S and ll_indep add a thread's entries in ascending order, then the library's wave sum, then the waves in order.
 *     The order is fixed by (m, t) alone: an entry's and a read's bits depend on the read and the sites alone, not on the batch, the
 *     order of the reads, the memspace or the outputs asked for.  No float atomics.
 *   nmod_read_sites_count(prm, nreads, cs, start, roff, score, nsites, key, hoff_out, nrows_out) computes hoff[nreads + 1] (int64), the
 *     exclusive scan of m, on prm->stream and synchronises the stream once to return *nrows_out (a host pointer), as
 *     nmod_pair_rows_count does.  NMOD_ERR_INVALID_ARG: the shared refusals, a NULL hoff_out or nrows_out, nrows > 2^31 - 1 (hoff is
 *     written by then).
 *   nmod_read_hmm(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows, opts, out).  Outputs (a NULL member is skipped;
 *     requesting fewer never changes the bits of the others): post double[nrows], site int32[nrows], state uint8[nrows]; n_sites, n_mod,
 *     n_can, n_runs int32[nreads]; ll, ll_indep double[nreads]; status uint8[nreads]; site_n, site_mod, site_can int32[nsites].  When
 *     none of post, state, n_mod, n_can, n_runs and the site counts is asked for, the backward pass is not run.
 *     Reads struct_size, device, stream, memspace of prm.  NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no host read and
 *     no synchronisation; hoff is not checked: a row outside its read's hoff range or outside [0, nrows) is skipped.  NMOD_MEM_HOST:
 *     one staged copy.  nreads == 0 or nrows == 0: NMOD_OK with zeroed site counts (with reads, each gets NMOD_HMM_NO_SITE).
 *     NMOD_ERR_INVALID_ARG before any device work: the shared refusals of nmod_site_pairs (nreads, nsites, NULL inputs, host offsets
 *     that decrease, host keys that do not strictly ascend); pi, length or call_post outside its range or not finite; opts or out NULL
 *     or of another struct_size; nrows outside 0 .. 2^31 - 1 or positive without reads or sites; a NULL hoff; host hoff that does not
 *     start at 0, ascend and end at nrows.
 *   Scratch: 32 B per row (position, score, forward vector), 36 B where site is not asked for.
 * Stops at: two states; one (pi, length) for all sites and reads (a per-site prior on request: K23, nmod_read_hmm_prior, below);
 * posterior decoding (the most probable path is
 * nmod_read_viterbi's, below); no Baum-Welch: pi and length are given (nmod_read_hmm_grad, below, is what a maximum-likelihood fit of
 * both is built on; a grid of lengths is the caller's other choice); the reads are independent and
 * both k-mer tables are taken as right; one (chrom, strand) per read. */
#define NMOD_HMM_CHUNK 4                   /* steps of a tile a thread owns */
#define NMOD_HMM_WAVE_MAX 1024             /* entries of a read up to which one wave computes it (a workgroup of four beyond) */
enum { NMOD_HMM_NO_SITE = 1 };
typedef struct nmod_hmm_opts { int32_t struct_size, reserved; double pi, length, call_post; } nmod_hmm_opts;
typedef struct nmod_hmm_out { int32_t struct_size; int32_t reserved;
  double* post; int32_t* site; uint8_t* state; int32_t *n_sites, *n_mod, *n_can, *n_runs; double *ll, *ll_indep; uint8_t* status;
  int32_t *site_n, *site_mod, *site_can;
} nmod_hmm_out;
int nmod_read_sites_count(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                          const double* score, int64_t nsites, const int64_t* key, int64_t* hoff_out, int64_t* nrows_out /* host */);
int nmod_read_hmm(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                  const double* score, int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows,
                  const nmod_hmm_opts* opts, const nmod_hmm_out* out);

/* Per-read Viterbi decoding of nmod_read_hmm's chain: the jointly most probable sequence of states of a read's entries, how firmly
 * every entry belongs to it, and the path's log-probability (K20; the reference project has no such step).  nmod_read_hmm's state is
 * a marginal call per entry, and a sequence of such calls need not be a likely path; a domain is a statement about a path.
 *   Inputs, word for word nmod_read_hmm's: the reads, score, key, hoff and nrows (from nmod_read_sites_count), the ENTRIES of a read,
 *     opts->pi and opts->length with their ranges, q = 1 - pi formed once on the host, T_j, the memspaces, the stream contract, the
 *     NULL-skips-an-output rule, and the refusals (there is no call_post); a row outside its read's hoff range is skipped.
 *   Model, in logarithms.  log q and log pi are formed once on the host.  The emissions le_j = (-max(s_j, 0), min(s_j, 0)), formed as
 *     (s_j > 0 ? -s_j : 0, s_j < 0 ? s_j : 0): exact, no exp and no log.  With rho and eps as in nmod_read_hmm, the step is
 *         L_j[r][c] = log(T_j[r][c]) + le_j[c],   T_0 = I: L_0 = [[le_00, -inf], [-inf, le_01]];
 *     three logarithms a step: log T_j = [[log(q + pi rho), log pi + log eps], [log q + log eps, log(pi + q rho)]], each sum formed
 *     before le is added.  The identity of the (max, +) algebra is [[0, -inf], [-inf, 0]].  Every term is <= 0
 *     up to rounding: no +inf and no NaN arises, and nothing is rescaled.  Contraction is off for the whole translation unit.
 *   MAX of two sums (u, v) is v where v > u and u otherwise: the first of equals, everywhere below.
 *   Products.  Of two matrices c_rc = MAX(l_r0 + r_0c, l_r1 + r_1c); a vector step y_c = MAX(x_0 + m_0c, x_1 + m_1c), forwards from
 *     (log q, log pi): a_j = x_j, the best score of a path over entries 0 .. j that ends in each state.
 *   Back-pointers.  psi_j(c) = 1 iff x_1 + m_1c > x_0 + m_0c, strictly (a tie goes to state 0), from the two sums that give y_c in the
 *     thread's replay of step j (ORDER below): path and vit agree with each other bit for bit.
 *   Traceback.  z_(m-1) = 1 iff a_(m-1),1 > a_(m-1),0;  z_(j-1) = psi_j(z_j).  (Computed as a scan of compositions of maps
 *     {0, 1} -> {0, 1} over tiles from the last entry to the first; integers, so any order gives the recursion's result.)
 *   Per entry.  path_j = z_j (uint8, 0 or 1).  site_j as in nmod_read_hmm.  delta_j = M_j(1) - M_j(0) with M_j(s) = a_j(s) + b_j(s),
 *     the score of the best path that is in state s at entry j: b is the backward vector, from nmod_read_hmm's backward scan in this
 *     algebra (the transposes of L_j reversed, from (0, 0)); delta_j = (a_j1 + b_j1) - (a_j0 + b_j0) in that order.  delta_j > 0 says
 *     how much score the best path loses if entry j is forced canonical, delta_j < 0 the same for modified; in exact arithmetic
 *     path_j = 1 implies delta_j >= 0.
 *   Per read.  n_sites = m (int32); n_mod = the entries of the path in state 1; n_runs = its maximal runs of 1;
 *     vit = MAX(a_(m-1),0, a_(m-1),1) + S, S the sum of max(s_j, 0) in nmod_read_hmm's order: the best path's log-probability on ll's
 *     scale, so vit <= ll up to rounding and vit - ll is the log of P(best path | the read's scores).  status (uint8):
 *     NMOD_HMM_NO_SITE when m = 0 (vit = 0, the counts 0).
 *   Per site (int32[nsites] each, integer atomics, zeroed by the entry on the stream): site_n = the reads with an entry there,
 *     site_mod = the entries of the paths in state 1.
 *   ORDER of the operations: nmod_read_hmm's, with the same NMOD_HMM_CHUNK and NMOD_HMM_WAVE_MAX: T = 64 or 256 threads by m, tiles
 *     of T * NMOD_HMM_CHUNK steps, a thread's product of its steps left to right, the six-step scan of the lanes (d = 1 .. 32, lane
 *     l >= d takes P_(l-d) P_l), the vector in front of a thread's chunk = the tile's carry, times the totals of the waves in front
 *     in ascending order, times the scanned product of the lane before; then one vector step per entry, and the carry of the next
 *     tile is thread T - 1's vector.  The backward scan: step k is the transpose of L_(m-k), the identity at k = 0, and belongs to
 *     entry m - 1 - k.  The bits of every output depend on the read and the sites alone, not on the batch, the order of the reads,
 *     the memspace or the outputs asked for.  No float atomics.
 *   Passes.  When none of path, n_mod, n_runs and site_mod is asked for, the traceback is not run and no back-pointer is stored; when
 *     delta is not asked for, the backward scan is not run and no forward vector is stored.  Asking for fewer outputs never changes
 *     the bits of the others.
 *   Overflow.  Scores whose sums leave the double range make vit and delta unspecified (infinite or NaN); path stays 0 or 1.
 *   NMOD_ERR_INVALID_ARG before any device work: nmod_read_hmm's list without call_post.  nreads == 0 or nrows == 0: NMOD_OK with
 *     zeroed site counts (with reads, each gets NMOD_HMM_NO_SITE).
 *   Scratch: at most 33 B per row (position, score, forward vector, one byte of back-pointers), 37 B where site is not asked for; 16 B
 *     less without delta, 1 B less without the traceback.
 * Stops at: the single best path, no k-best list and no minimum-length constraint on a domain; the model is nmod_read_hmm's with all
 * its limits (two states, one (pi, length) — a per-site prior on request: K23, nmod_read_viterbi_prior, below —, no Baum-Welch: both are
 * given, or fitted through nmod_read_hmm_grad, below). */
typedef struct nmod_vit_opts { int32_t struct_size, reserved; double pi, length; } nmod_vit_opts;
typedef struct nmod_vit_out { int32_t struct_size; int32_t reserved;
  uint8_t* path; int32_t* site; double* delta;                          /* [nrows] */
  int32_t *n_sites, *n_mod, *n_runs; double* vit; uint8_t* status;      /* [nreads] */
  int32_t *site_n, *site_mod;                                           /* [nsites] */
} nmod_vit_out;
int nmod_read_viterbi(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                      const double* score, int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows,
                      const nmod_vit_opts* opts, const nmod_vit_out* out);

/* The gradient of nmod_read_hmm's log-likelihood in the chain's two parameters, per read and summed over the batch: what a maximum-
 * likelihood fit of (pi, length) needs from the device, one call per evaluation (K21; the reference project has no such step).  The
 * fit itself, a few Newton-like steps on eight numbers, is the caller's (nanomod_amd/readllr.py: fit_hmm).
 *   Inputs, word for word nmod_read_hmm's: the reads, score, key, hoff and nrows, the ENTRIES of a read, opts->pi and opts->length with
 *     their ranges, q = 1 - pi formed once on the host, e_j, T_j, rho, eps, r = d / length, the memspaces, the stream contract, the
 *     NULL-skips-an-output rule and the refusals (there is no call_post); a row outside its read's hoff range is skipped.
 *   Parameters.  eta = logit(pi) and lam = ln(length): the scales on which both are unbounded and their likelihood is closest to a
 *     quadratic.  pi q is formed once on the host.
 *   Definition (Fisher's identity: the gradient of ll is the posterior mean of the gradient of the complete-data log-likelihood, a sum
 *     over the initial law and the transitions).  a_j = the forward vector of entry j as nmod_read_hmm's forward pass stores it, b_j =
 *     the backward vector at entry j as its backward pass replays it (ORDER there).  For j = 1 .. m - 1, with y0 = e_j0 b_j0,
 *     y1 = e_j1 b_j1, A = a_(j-1) and T = T_j:
 *         Z   = A0 (t00 y0 + t01 y1) + A1 (t10 y0 + t11 y1)
 *         P_j = eps (A0 + A1) (y1 - y0) / Z                        (d/d pi of the transition's logarithm, averaged)
 *         L_j = rho r (pi A0 - q A1) (y0 - y1) / Z                 (the same in lam: d rho / d lam = rho r)
 *     each evaluated left to right as written, no fused operation; post_0 = a_01 b_01 / (a_00 b_00 + a_01 b_01) as nmod_read_hmm forms it;
 *         g_eta = (post_0 - pi) + (pi q) SUM_j P_j,     abs_eta = |post_0 - pi| + (pi q) SUM_j |P_j|,
 *         g_lam = SUM_j L_j,                            abs_lam = SUM_j |L_j|.
 *     Both terms are ratios that are homogeneous of degree 0 in a and in b: the exponents the scan drops do not enter.  No division by
 *     an entry of T occurs.  abs_eta and abs_lam are what an error bound of g_eta and g_lam is relative to (tests/hmm_fit_ref.py).
 *     A Z that underflows (emissions of opposite sign beyond +-700 at every state) makes the terms unspecified, as it does post.
 *   Per read (double[nreads] each): ll, bit for bit nmod_read_hmm's for the same inputs; g_eta, g_lam, abs_eta, abs_lam; status (uint8):
 *     NMOD_HMM_NO_SITE when m = 0 (every value 0).  A read of one entry has g_lam = 0.
 *   ORDER.  The forward pass is nmod_read_hmm's.  The backward pass is its scan; the term of transition j is formed by the thread that
 *     replays step k = m - 1 - j, which adds its terms in the order of its steps (descending j) over all tiles into one word per sum;
 *     then the library's wave sum, then the waves in order, as S.  The bits depend on the read and the sites alone, not on the batch,
 *     the order of the reads, the memspace or the outputs asked for.  No float atomics.
 *   sums (double[8]): SUM ll, SUM g_eta, SUM g_lam, SUM g_eta^2, SUM g_eta g_lam, SUM g_lam^2 over the reads, the number of reads with
 *     m >= 1 and the number of entries (as doubles, exact below 2^53).  One workgroup of 256 threads in a second kernel on the same
 *     stream: thread t adds reads t, t + 256, ... in ascending order (a product is rounded, then added), then the wave sum of every
 *     word and the four waves in order.  The bits depend on the per-read values and their order alone.  The three matrix words are the
 *     outer-product (BHHH) estimate of the information in (eta, lam).
 *   nmod_read_hmm_grad(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows, opts, out).  NMOD_MEM_DEVICE: everything is
 *     enqueued on prm->stream, no host read and no synchronisation.  NMOD_MEM_HOST: one staged copy.  nreads == 0: NMOD_OK, sums all 0.
 *     NMOD_ERR_INVALID_ARG before any device work: nmod_read_hmm's list without call_post.
 *   Scratch: 36 B per row (position, score, forward vector, site), and 8 B per read for each of ll, g_eta, g_lam not asked for.
 * Stops at: one (pi, length) for all reads and sites (a per-site prior on request: K23, nmod_read_hmm_grad_prior, below); the emissions and both k-mer tables are taken as right (no gradient in them);
 * the outer-product information, not the observed Hessian: standard errors from it are right at the model and in large samples only;
 * the caller's intervals are Wald intervals on the logit and log scales; the first derivative only. */
typedef struct nmod_hmm_grad_opts { int32_t struct_size, reserved; double pi, length; } nmod_hmm_grad_opts;
typedef struct nmod_hmm_grad_out { int32_t struct_size; int32_t reserved;
  double *ll, *g_eta, *g_lam, *abs_eta, *abs_lam; uint8_t* status;     /* [nreads] */
  double* sums;                                                         /* [8] */
} nmod_hmm_grad_out;
int nmod_read_hmm_grad(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                       const double* score, int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows,
                       const nmod_hmm_grad_opts* opts, const nmod_hmm_grad_out* out);

/* The read chain with a prior share per candidate site: nmod_read_hmm, nmod_read_viterbi and nmod_read_hmm_grad, argument for argument,
 * with one more, site_pi (double[nsites], in the memspace of the call), after key (K23; the reference project has no such step).  One
 * stationary share for every site is the chain's largest misspecification on real samples: the shares of neighbouring sites differ by
 * an order of magnitude, and a chain that redraws every site from the mean share over-calls the rarely modified sites and under-calls
 * the others (nmod_read_hmm_grad then reports the misfit as a shorter fitted length).  The opts and out structs are the counterparts';
 * what is not restated here is the counterpart's, word for word.
 *   Share of entry j.  pi_j = site_pi[site_j] clamped to 1e-9 .. 1 - 1e-9 (an infinity is clamped like any other value); where that word
 *     is a NaN, pi_j = opts->pi (nmod_site_stoich gives a NaN to a site without an estimate).  opts->pi keeps its range check.
 *     q_j = 1 - pi_j, formed on the device from the clamped pi_j (one subtraction, the same double wherever entry j is met).  The share
 *     of a row is resolved once per call, by a gather over the rows behind the fill of the entries, not inside the scan.
 *   Transition.  With rho, eps and r exactly as in nmod_read_hmm:
 *         T_j = [[q_j + pi_j rho, pi_j eps], [q_j eps, pi_j + q_j rho]]     rows the state at j - 1, columns the state at j;
 *     the share is that of the entry arrived at: "copy the neighbour's state with probability rho, else redraw from the site's own
 *     law".  Initial law (q_0, pi_0).  Emissions, scaling, tiles, scan order, carries, the backward scan, states, runs, site counts,
 *     ll, the S sum and the passes-not-run rules are nmod_read_hmm's;  ll_indep = SUM_j (log(q_j e_j0 + pi_j e_j1) + max(s_j, 0)).
 *   Viterbi.  log pi_j and log q_j are formed on the device from the clamped pi_j and the q_j above (nmod_read_viterbi forms its two
 *     logarithms on the host: with a constant site_pi the two entries may differ in the last bits of vit and delta, and in path where
 *     delta is a tie to rounding).  The forward scan starts from (log q_0, log pi_0); L_j, MAX, the back-pointers, the traceback,
 *     delta, vit and the tie rule are nmod_read_viterbi's with pi_j, q_j and their logarithms in place of pi, q and theirs.
 *   Gradient.  g_lam and abs_lam are nmod_read_hmm_grad's L_j with pi_j, q_j in place of pi, q.  g_eta is the derivative of ll in a
 *     common logit offset kappa of all shares (logit pi_j -> logit pi_j + kappa), evaluated at the shares given:
 *         g_eta = (post_0 - pi_0) + SUM_j ((pi_j q_j) P_j),     abs_eta = |post_0 - pi_0| + SUM_j |(pi_j q_j) P_j|,
 *     P_j nmod_read_hmm_grad's expression with T_j as above (d T_j / d pi_j = eps [[-1, 1], [-1, 1]] and d pi_j / d kappa = pi_j q_j);
 *     the product (pi_j q_j) P_j is rounded, then added, in the order of nmod_read_hmm_grad's sums.  With a constant site_pi, ll,
 *     g_lam, abs_lam and status have nmod_read_hmm_grad's bits, g_eta its value to rounding.  sums[8] keeps its layout and its kernel.
 *   With site_pi constant at opts->pi, or all NaN, every output of nmod_read_hmm_prior has nmod_read_hmm's bits.
 *   CAVEAT.  Under this law the marginal share of entry j is rho P(z_(j-1) = 1) + eps pi_j, not pi_j, while an estimate such as
 *     nmod_site_stoich's is a marginal.  The mismatch grows where neighbouring sites less than a `length` apart have very different
 *     shares.  A transition that preserves given marginals exactly is another model and is not built.
 *   NMOD_ERR_INVALID_ARG before any device work: site_pi NULL with nsites > 0; everything else: the counterpart's list.  The values of
 *     site_pi are never refused, in either memspace.  Stream contract, memspaces, NULL-skips-an-output: the counterparts'.  An entry's
 *     and a read's bits depend on the read, the sites and site_pi alone.
 *   Scratch, beside the counterpart's: 8 B per row for nmod_read_hmm_prior and nmod_read_hmm_grad_prior (the clamped share of the
 *     row), 24 B per row for nmod_read_viterbi_prior (the share and its two logarithms); a host call stages site_pi as well. */
int nmod_read_hmm_prior(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                        const double* score, int64_t nsites, const int64_t* key, const double* site_pi, const int64_t* hoff, int64_t nrows,
                        const nmod_hmm_opts* opts, const nmod_hmm_out* out);
int nmod_read_viterbi_prior(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                            const double* score, int64_t nsites, const int64_t* key, const double* site_pi, const int64_t* hoff, int64_t nrows,
                            const nmod_vit_opts* opts, const nmod_vit_out* out);
int nmod_read_hmm_grad_prior(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                             const double* score, int64_t nsites, const int64_t* key, const double* site_pi, const int64_t* hoff, int64_t nrows,
                             const nmod_hmm_grad_opts* opts, const nmod_hmm_grad_out* out);

/* Latent-class clustering of the reads by their modification pattern: a finite mixture of C classes over the reads, every class with
 * a weight and a modified share of its own at every candidate site, fitted by EM (K22; the reference project has no such step).  K14
 * to K21 take every read from one population; here a site whose share is 0.45 may be 35 % of the molecules at 0.8 and the rest at 0.1,
 * and gamma says which read is which.  One EM step per call; the loop is the caller's (nanomod_amd/readllr.py: fit_classes).
 * Memspaces, the stream contract, the NULL and struct_size rules: those of nmod_read_hmm.
 *   ENTRIES of a read: nmod_read_hmm's, with its VALID and COVERS rules.  Entry j is at site site_j with the window sum s_j.
 *   Model.  Class c has the weight w_c and the share theta[site][c]; the sites are independent within a class.  With
 *     t_j = -expm1(-|s_j|), K14's form:
 *         g(s, th)    = log1p(-((s >= 0 ? 1 - th : th) * t))              = log((1 - th) e_0 + th e_1), K19's scaled emissions
 *         post(s, th) = s >= 0 ? th / (1 - (1 - th) * t) : th * (1 - t) / (1 - th * t),
 *     each evaluated left to right as written, no fused operation: contraction is off for the whole translation unit.
 *   Per read.  l_rc = SUM_j g(s_j, theta[site_j][c]);  a_rc = log(w_c) + l_rc, log(w_c) the device's log of w_in[c] (in
 *     NMOD_MEM_DEVICE nothing is read back, so both memspaces form it on the device and agree bit for bit);  M = MAX_c a_rc, the first
 *     of equals;  x_c = exp(a_rc - M), Z = SUM_c x_c added in ascending c from 0;  gamma_rc = x_c / Z;
 *     ll_r = (M + log(Z)) + S_r with S_r = SUM_j max(s_j, 0): the read's log-likelihood relative to "every site canonical"; with C = 1
 *     it is nmod_read_hmm's ll_indep with a pi per site.  cls_r (int32) = the arg max of gamma, the first of equals.  status (uint8):
 *     NMOD_HMM_NO_SITE when m = 0, with gamma = 0, ll = 0 and cls = -1; such a read takes no part in any sum.
 *     ORDER.  A read of up to NMOD_HMM_WAVE_MAX entries is computed by T = 64 threads, a longer one by T = 256.  Thread t adds the terms
 *     of entries t, t + T, t + 2 T, ... in ascending order from 0.0 into one word per class and one for S; then the library's wave sum
 *     of every word (lanes l ^ 1, l ^ 2, the mirror within 8, the mirror within 16, then 0.0 + the four rows of 16 in order), then for
 *     T = 256 the four waves from 0.0 in order.  The classes of a site are theta[site * C .. site * C + C - 1].
 *   Per site and class, over the rows of the site in ascending row index (that is ascending read index):
 *     N_jc = SUM gamma_rc;  Mo_jc = SUM (gamma_rc * post(s, theta_in[j][c])), the product rounded and then added;
 *     theta_out[j][c] = Mo_jc / N_jc clamped to 1e-9 .. 1 - 1e-9, and theta_in[j][c] where N_jc == 0 (n_site is N).
 *     ORDER.  A site of up to NMOD_CLASSES_SMALL rows is computed by G = 16 lanes, up to NMOD_CLASSES_WAVE by G = 64, a larger one by
 *     G = 256 threads.  Thread g adds rows g, g + G, ... of the site's list in ascending order from 0.0; then for G = 16 the first four
 *     steps of the wave sum (l ^ 1, l ^ 2, the two mirrors; lane 0's word), for G = 64 the wave sum, for G = 256 the wave sums and the
 *     four waves from 0.0 in order.  The bits of a site depend on its rows and their order alone.
 *   Weights and sums: one workgroup of 256 threads.  Thread t adds reads t, t + 256, ... with an entry in ascending order, then the wave
 *     sum of every word and the four waves in order.  sums (double[4 + C]): SUM ll, R1 = the reads with an entry, the entries (as
 *     doubles, exact below 2^53), MAX |theta_out - theta_in| over the (site, class) cells with N > 0, and SUM_r gamma_rc per class.
 *     w_out[c] = sums[4 + c] / R1, and w_in[c] where R1 == 0.
 *   No float atomics.  A read's gamma, ll and cls depend on the read, theta_in and w_in alone: not on the batch, the order of the
 *     reads, the memspace or the outputs asked for.
 *   nmod_read_class_rows(prm, nreads, cs, start, roff, score, nsites, key, hoff, nrows, out), once per data set: nmod_read_hmm's read
 *     arguments with hoff and nrows from nmod_read_sites_count.  Per row site (int32) and s (double), nmod_read_hmm's site and score
 *     byte for byte, and rread (int32), the row's read; the site-major view soff (int64[nsites + 1]) and srow (int32[nrows]): the rows
 *     of site j are srow[soff[j] .. soff[j + 1] - 1] in ascending row index (a stable sort of the rows by their site).  A NULL output
 *     is skipped.  Refusals: nmod_read_hmm's without the options.  Scratch: 36 B per row beside the sort's, 44 B without site and srow.
 *     A row that no read owns (NMOD_MEM_DEVICE with nrows above hoff[nreads], which is not read back) keeps site -1, s 0.0 and rread -1,
 *     sorts behind every site in ascending row index (the last nrows - hoff[nreads] words of srow) and leaves soff[nsites] = hoff[nreads].
 *   nmod_read_classes_step(prm, nreads, nsites, nrows, hoff, site, s, rread, soff, srow, opts, theta_in, w_in, out), once per EM step:
 *     the reads are not walked again.  theta_in double[nsites * C], the C classes of a site contiguous; w_in double[C].  Outputs (a NULL
 *     member is skipped; asking for fewer never changes the bits of the others): gamma double[nreads * C], ll double[nreads], cls
 *     int32[nreads], status uint8[nreads], theta_out and n_site double[nsites * C], w_out double[C], sums double[4 + C].
 *     NMOD_MEM_DEVICE: everything is enqueued on prm->stream, no host read and no synchronisation; nothing is checked: a row index
 *     outside [0, nrows), a site outside [0, nsites), an rread outside [0, nreads) and offsets outside the rows are skipped and never
 *     dereferenced.  NMOD_MEM_HOST: one staged copy.
 *     NMOD_ERR_INVALID_ARG before any device work: the shared refusals (counts out of range, a NULL input, opts or out NULL or of
 *     another struct_size, nrows positive without reads or sites); n_classes outside 1 .. NMOD_CLASSES_MAX; host theta_in or w_in
 *     outside 1e-9 .. 1 - 1e-9 or not finite (with one class the weight 1 is the only one there is, and is accepted); host w_in not
 *     summing to 1 within 1e-9; host hoff or soff that does not start at 0, ascend and end at nrows.
 *     Scratch: 8 C B per read for gamma and 8 B for ll where a later kernel needs them and they are not asked for; the same per site
 *     for theta_out and n_site when only sums asks for them.
 * Stops at: sites independent within a class, no chain inside a class; both k-mer tables taken as right; EM finds a local maximum and
 * the caller's restarts are the only defence; no standard errors of theta; the choice of C is the caller's (BIC in readllr.py);
 * C <= NMOD_CLASSES_MAX; a molecule sequenced twice counts twice. */
#define NMOD_CLASSES_MAX 8                 /* classes of a fit */
#define NMOD_CLASSES_SMALL 64              /* rows of a site up to which 16 lanes compute it */
#define NMOD_CLASSES_WAVE 512              /* ... up to which one wave does (a workgroup of 256 beyond) */
typedef struct nmod_class_rows_out { int32_t struct_size; int32_t reserved;
  int32_t* site; double* s; int32_t* rread;                             /* [nrows] */
  int64_t* soff;                                                        /* [nsites + 1] */
  int32_t* srow;                                                        /* [nrows] */
} nmod_class_rows_out;
typedef struct nmod_classes_opts { int32_t struct_size, n_classes; } nmod_classes_opts;
typedef struct nmod_classes_out { int32_t struct_size; int32_t reserved;
  double *gamma, *ll; int32_t* cls; uint8_t* status;                    /* [nreads * C], [nreads] ... */
  double *theta_out, *n_site;                                           /* [nsites * C] */
  double *w_out, *sums;                                                 /* [C], [4 + C] */
} nmod_classes_out;
int nmod_read_class_rows(const nmod_params* prm, int64_t nreads, const int32_t* cs, const int64_t* start, const int64_t* roff,
                         const double* score, int64_t nsites, const int64_t* key, const int64_t* hoff, int64_t nrows,
                         const nmod_class_rows_out* out);
int nmod_read_classes_step(const nmod_params* prm, int64_t nreads, int64_t nsites, int64_t nrows, const int64_t* hoff,
                           const int32_t* site, const double* s, const int32_t* rread, const int64_t* soff, const int32_t* srow,
                           const nmod_classes_opts* opts, const double* theta_in, const double* w_in, const nmod_classes_out* out);

/* ---- position shards across the GPUs of a node without any host framework (BASELINE.json north_star: "an RCCL
 * all-gather over xGMI to reassemble the per-base p-value track").  The reference has no counterpart (one CPU process).  One
 * process (or thread) per GPU computes a contiguous block of positions (+- nb recomputed neighbours) with
 * nmod_detect_batch and calls nmod_allgather_tracks: rank r's block of `block_len` doubles of every track lands at
 * full[t] + r * block_len on every rank (blocks of equal length: pad the last one).  The library does not link RCCL: it binds
 * librccl.so at the first call — the copy the process has already loaded if there is one (a PyTorch process: torch's), else
 * librccl.so.1 from the loader path — and returns NMOD_ERR_NO_RCCL when there is none.
 *   rank 0:      nmod_comm_unique_id(id)  -> hand the NMOD_COMM_ID_BYTES bytes to the other ranks (file, socket, MPI, ...)
 *   every rank:  nmod_comm_init_rank(id, nranks, rank, device, &comm)           (collective: all ranks must call it)
 *                nmod_allgather_tracks(comm, stream, block_len, ntracks, local, full)   enqueued on `stream`, no synchronisation
 *                nmod_comm_destroy(comm) */
#define NMOD_COMM_ID_BYTES 128
#define NMOD_ERR_NO_RCCL (-6)      /* librccl.so could not be bound */
#define NMOD_ERR_RCCL (-7)         /* an RCCL call failed; see nmod_strerror */
typedef struct nmod_comm nmod_comm;
int nmod_comm_unique_id(void* id_out);
int nmod_comm_init_rank(const void* unique_id, int32_t nranks, int32_t rank, int32_t device, nmod_comm** comm_out);
int nmod_allgather_tracks(nmod_comm* comm, void* stream, int64_t block_len, int32_t ntracks,
                          const double* const* local, double* const* full);
int nmod_comm_destroy(nmod_comm* comm);

/* ---- read-level input: per-read event tables -> the tested CSR rows, on the device (nanomod_amd/csrc/read_pivot.hip).
 * The reference appends every event of every aligned read to its position's list (mReadSignalBase, myDetect.py:104-124),
 * filters thin positions (mfilter_coverage, myDetect.py:301-314) and tests the positions both groups share, in sorted order
 * (myDetect.py:421,427-431).  These three calls do the same for flat read sets: prm->memspace must be NMOD_MEM_DEVICE (every
 * array pointer is device memory; sizes and counts marked "host" are host pointers), prm->dtype is the value type of the
 * samples, prm->device / prm->stream as everywhere.  Each call synchronises its stream once or a few times to learn its
 * data-dependent sizes; outputs are identical bytes on every run.  Scratch comes from the library's per-device pool
 * (nmod_trim_scratch returns it).
 *
 * nmod_pivot_reads — myDetect.py:104-124 for a whole read set.  Read r has (chrom, strand) id cs[r] = 2 * chrom index +
 * (strand == '-') (ids ascend in mtest2's order, '+' before '-'; 0 <= cs < ncs), 0-based start[r] (mapped_start) and events
 * roff[r] .. roff[r+1] (roff[0] == 0, non-decreasing; at most 2^32 - 1 events in all) of val (prm->dtype) and base (one byte
 * each).  Event i of a read of n events lies at position start + i on '+', start + n - 1 - i on '-'; events outside the
 * inclusive clip [pos_lo, pos_hi] (either bound -1 = none; the event-level window of myDetect.py:112-114) are dropped.
 * Output: *npos_out rows, key_out[i] = cs << 40 | pos strictly ascending, off_out[0 .. npos] CSR offsets into sig_out /
 * the samples of a row in read order (the order GroupBuilder.finish gives), base_out[i] = the base of the row's LAST read
 * (myDetect.py:122).  Capacities: key_out / base_out cap_pos rows, off_out cap_pos + 1, sig_out roff[nreads] samples.
 * NMOD_ERR_INVALID_ARG (nothing written) for bad offsets, cs outside [0, ncs), a negative start, a position at or past 2^40,
 * or cap_pos below the row count; also when the rows beyond 1 024 samples hold 2^31 - 1 or more samples in all (they are
 * ordered by one radix sort, whose index range that is; key_out / off_out are written by then, sig_out / base_out are not).
 * Scratch: 28 B per position of the dense range of every cs (its last covered position minus its first, plus one, summed
 * over cs) + 4 B per event, and 24 B per sample of rows beyond 1 024 samples (so at most 24 B x (2^31 - 1)). */
int nmod_pivot_reads(const nmod_params* prm, int64_t nreads, int32_t ncs, const int32_t* cs, const int64_t* start,
                     const int64_t* roff, const void* val, const uint8_t* base, int64_t pos_lo, int64_t pos_hi,
                     int64_t cap_pos, int64_t* key_out, int64_t* off_out, void* sig_out, uint8_t* base_out,
                     int64_t* npos_out /* host */, int64_t* nsamples_out /* host */);

/* nmod_select_tested — myDetect.py:301-314 per group + :421,427-431: the rows of both pivoted groups (keys strictly ascending,
 * offsets off*[0 .. npos*] over nsig* samples of prm->dtype) whose key both groups hold with at least min_coverage samples,
 * in key order: rows0 / rows1 (cap entries each), the CSR offsets of the tested rows off0_out / off1_out (cap + 1 each),
 * *ntested_out, the samples per group and *dtype_out, the one dtype detect.encode_pair picks for the tested samples of both
 * groups (a device reduction): float32 input stays float32; otherwise float32 if every value is float32-exact, else int16
 * milli-units if every value is k/1000.0 with |k| <= 32767, else float64; float64 input beyond 4 000 000 tested samples
 * passes through, int16 input is never widened to float64 (its values are k/1000.0).  NMOD_ERR_INVALID_ARG for bad offsets
 * or cap below the tested row count.  Scratch: 24 B per row of group 1. */
int nmod_select_tested(const nmod_params* prm, int64_t min_coverage,
                       int64_t npos0, const int64_t* key0, const int64_t* off0, const void* sig0, int64_t nsig0,
                       int64_t npos1, const int64_t* key1, const int64_t* off1, const void* sig1, int64_t nsig1,
                       int64_t cap, int64_t* rows0, int64_t* rows1, int64_t* off0_out, int64_t* off1_out,
                       int64_t* ntested_out /* host */, int64_t* nsamples0_out /* host */, int64_t* nsamples1_out /* host */,
                       int32_t* dtype_out /* host */);

/* nmod_gather_tested — the tested rows (from nmod_select_tested) as the inputs of nmod_detect_batch: sig0_out / sig1_out in
 * out_dtype at off0_out / off1_out, run_out[t] (detect.run_ids / pos_check, myDetect.py:366-371: a new run at every change of
 * cs or gap in pos, from the keys), key_out[t] = key1[rows1[t]], base0_out / base1_out the bases of both groups (the table
 * uses group 2's; myDetect.py:432-434 reports mismatches).  int16 input means k/1000.0 in every conversion.  Enqueued only:
 * no synchronisation.  Scratch: 8 B per tested row. */
int nmod_gather_tested(const nmod_params* prm, int64_t ntested, const int64_t* rows0, const int64_t* rows1,
                       const int64_t* off0, const void* sig0, const uint8_t* base0,
                       const int64_t* off1, const void* sig1, const uint8_t* base1, const int64_t* key1,
                       int32_t out_dtype, const int64_t* off0_out, const int64_t* off1_out, void* sig0_out, void* sig1_out,
                       int32_t* run_out, int64_t* key_out, uint8_t* base0_out, uint8_t* base1_out);

/* Lane-permutation self test of the wave primitives the sort is built from
 * (runs tiny kernels; returns NMOD_OK or the number of the first failing primitive). */
int nmod_selftest(int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* NANOMOD_HIP_H */
