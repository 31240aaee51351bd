"""ctypes binding of libnanomod_hip.so (include/nanomod_hip.h).

The product path has no CPU fallback: if the HIP library is missing, loading
fails loudly with instructions to build it.
"""
from __future__ import annotations

import ctypes as C
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (NMOD_HIP_LIB: another build of the same library, for A/B measurements of kernel variants on one box)
LIB_PATH = os.environ.get('NMOD_HIP_LIB') or os.path.join(_HERE, 'libnanomod_hip.so')

NMOD_ABI_VERSION = 4
DTYPE_F32, DTYPE_I16_MILLI, DTYPE_F64 = 0, 1, 2
MEM_HOST, MEM_DEVICE = 0, 1
METHOD_KS, METHOD_STOUFFER, METHOD_FISHER = 0, 1, 2
TEST_KS, TEST_MWU, TEST_WELCH, TEST_ALL = 1, 2, 4, 7
FLAG_KS_RATIONAL_D, FLAG_CHECK_FINITE, FLAG_NO_COUNTING, FLAG_NO_COUNT_WIDE, FLAG_NO_HOST_NARROW = 1, 2, 4, 8, 16
FLAG_DEEP = 32            # groups beyond MAX_RANKED (up to MAX_DEEP) take the deep form instead of STATUS_TOO_LARGE
FLAG_K1_STATIC_ITEMS = 128   # the KS-only K1 kernel walks equal strided shares instead of claiming chunks of items (A/B, parity tests)
STATUS_MWU_ALL_IDENTICAL, STATUS_T_NAN, STATUS_EMPTY, STATUS_TOO_LARGE, STATUS_NONFINITE = 1, 2, 4, 8, 16
STATUS_BAD_REFERENCE = 32   # nmod_one_sample only: an unusable reference (mean / sd not finite, sd <= 0, ref_n < 2)
STATUS_NO_CODE = 64         # nmod_kmer_model only: the position has no k-mer code and takes no part
KERNEL_RANK_STATS, KERNEL_FINALIZE, KERNEL_COMBINE, KERNEL_SYNTH = 0, 1, 2, 3
MAX_GROUP = 2048          # largest group of the wave-resident kernels; larger ones (<= MAX_RANKED) take big_rank_kernel
MAX_RANKED = 65535
MAX_DEEP = 2 ** 24 - 1    # largest group with FLAG_DEEP
MAX_NB = 64
MAX_ONE, MAX_ONE_F64 = 16384, 8192   # nmod_one_sample: samples per position (float32 / int16, float64)
MAX_KMER_CODES = 65536    # nmod_kmer_model: 4^8
COMM_ID_BYTES = 128
ERR_NO_RCCL, ERR_RCCL = -6, -7

METHOD_BY_NAME = {'ks': METHOD_KS, 'stouffer': METHOD_STOUFFER, 'fisher': METHOD_FISHER}

OUT_FIELDS = ('mwu_u', 'mwu_p', 't_t', 't_p', 'ks_d', 'ks_p', 'comb_st', 'comb_p',
              'mean0', 'std0', 'mean1', 'std1')


class NmodParams(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('device', C.c_int32), ('stream', C.c_void_p),
                ('memspace', C.c_int32), ('dtype', C.c_int32), ('tests', C.c_int32),
                ('method', C.c_int32), ('nb', C.c_int32), ('want_mstd', C.c_int32),
                ('weights_dif', C.c_double), ('stride0', C.c_int64), ('stride1', C.c_int64),
                ('max_n0', C.c_int32), ('max_n1', C.c_int32), ('timer', C.c_void_p), ('flags', C.c_int32), ('reserved', C.c_int32)]


class NmodOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in OUT_FIELDS] + [('status', C.c_void_p)]


class NmodHostStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ('chunks', 'slots', 'copy_threads', 'pinned_input', 'chunk_positions',
                                         'device_bytes', 'pinned_bytes', 'h2d_bytes', 'd2h_bytes', 'narrowed_chunks')]


class NmodDispatchStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ('positions', 'ks_rank', 'rank_hist', 'rank_hist_wide', 'rank_pair', 'rank_count', 'rank_count_wide',
                                         'big', 'skipped', 'count_tried', 'count_rejected', 'f64_redo', 'deep')] + [('reserved', C.c_int64 * 3)]


def last_dispatch_stats():
    """nmod_last_dispatch_stats as a dict: which K1 form computed the positions of this thread's last nmod_detect_batch"""
    st = NmodDispatchStats()
    check(load().nmod_last_dispatch_stats(C.byref(st)), 'nmod_last_dispatch_stats')
    return {n: int(getattr(st, n)) for n, _ in NmodDispatchStats._fields_ if n != 'reserved'}


FDR_BH, FDR_BY = 0, 1
FDR_BY_NAME = {'bh': FDR_BH, 'by': FDR_BY}


class NmodFdrSummary(C.Structure):
    _fields_ = [('tested', C.c_int64), ('excluded', C.c_int64), ('rejected', C.c_int64), ('p_crit', C.c_double)]


MIX_EQUAL_VAR, MIX_FREE_VAR = 0, 1
MIX_BY_NAME = {'equal': MIX_EQUAL_VAR, 'free': MIX_FREE_VAR}
MIX_NOT_CONVERGED, MIX_DEGENERATE, MIX_SKIPPED, MIX_VAR_FLOORED, MIX_TOO_LARGE = 1, 2, 4, 8, 16
MIX_FIELDS = ('pi', 'mu_mod', 'sd_mod', 'llr')


class NmodMixOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in MIX_FIELDS] + [('iters', C.c_void_p), ('status', C.c_void_p), ('resp', C.c_void_p)]


def make_out(cls, /, **members):
    """an out struct of class `cls`: struct_size filled in where the struct has one, the named members set, the rest left NULL
    (`cls` by position alone: nmod_classes_out has a member of that name)"""
    o = cls()
    if hasattr(cls, 'struct_size'):
        o.struct_size = C.sizeof(cls)
    for k, v in members.items():
        setattr(o, k, v)
    return o


ONE_FIELDS = ('ks_d', 'ks_p', 't_t', 't_p', 'shift', 'mean', 'std', 'comb_st', 'comb_p')


class NmodOneOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(name, C.c_void_p) for name in ONE_FIELDS] + [('status', C.c_void_p)]


make_one_out = functools.partial(make_out, NmodOneOut)


KMER_COUNT_FIELDS = ('n_positions', 'n_samples', 'n_clipped')
KMER_FIELDS = KMER_COUNT_FIELDS + ('mean', 'sd')


class NmodKmerOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(name, C.c_void_p) for name in KMER_FIELDS] + [('pos_status', C.c_void_p)]


make_kmer_out = functools.partial(make_out, NmodKmerOut)


KMIX_HALF, KMIX_BINS = 2048, 4096         # nmod_kmer_mix: a code's window is llrint(1000 mean0) - KMIX_HALF .. + KMIX_BINS - 1
KMIX_NOT_CONVERGED, KMIX_DEGENERATE, KMIX_NO_MODEL, KMIX_VAR_FLOORED, KMIX_TOO_FEW = 1, 2, 4, 8, 16
KMIX_NO_ESTIMATE = KMIX_DEGENERATE | KMIX_NO_MODEL | KMIX_TOO_FEW
KMIX_COUNT_FIELDS = ('n_positions', 'n_used', 'n_outside')
KMIX_FIELDS = ('pi', 'mu_mod', 'sd_mod', 'llr')


class NmodKmixOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'model', 'max_iter', 'reserved')] + [('min_samples', C.c_int64), ('tol', C.c_double)]


class NmodKmixOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + \
               [(n, C.c_void_p) for n in KMIX_COUNT_FIELDS + KMIX_FIELDS + ('iters', 'status', 'hist', 'pos_status')]


def make_kmix_opts(model=MIX_FREE_VAR, max_iter=200, tol=1e-6, min_samples=2):
    o = NmodKmixOpts()
    o.struct_size = C.sizeof(NmodKmixOpts)
    o.model, o.max_iter, o.min_samples, o.tol = int(model), int(max_iter), int(min_samples), float(tol)
    return o


make_kmix_out = functools.partial(make_out, NmodKmixOut)


RESCALE_FIT_APPLY, RESCALE_FIT_ONLY, RESCALE_APPLY_ONLY = 0, 1, 2
RESCALE_MODE_BY_NAME = {'fit_apply': RESCALE_FIT_APPLY, 'fit_only': RESCALE_FIT_ONLY, 'apply_only': RESCALE_APPLY_ONLY}
RESCALE_TOO_FEW, RESCALE_DEGENERATE, RESCALE_OUT_OF_RANGE, RESCALE_CLAMPED, RESCALE_TOO_LARGE = 1, 2, 4, 8, 16
RESCALE_FAILED = RESCALE_TOO_FEW | RESCALE_DEGENERATE | RESCALE_OUT_OF_RANGE | RESCALE_TOO_LARGE
RESCALE_WAVE_MAX = 2048   # nmod_rescale_reads: events of a read up to which one wave computes it (a workgroup beyond)


class NmodRescaleModel(C.Structure):
    _fields_ = [('k', C.c_int32), ('center', C.c_int32), ('mean', C.c_void_p), ('sd', C.c_void_p)]


class NmodRescaleOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'mode', 'weighted', 'clip_rounds', 'min_events', 'reserved')] + \
               [(n, C.c_double) for n in ('clip_sigma', 'scale_lo', 'scale_hi')]


class NmodRescaleOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in ('shift', 'scale', 'n_used', 'status', 'val_out')]


def make_rescale_opts(mode=RESCALE_FIT_APPLY, weighted=True, clip_sigma=3.0, clip_rounds=2, min_events=50, scale_lo=0.5, scale_hi=2.0):
    o = NmodRescaleOpts()
    o.struct_size = C.sizeof(NmodRescaleOpts)
    o.mode, o.weighted, o.clip_rounds, o.min_events = int(mode), int(bool(weighted)), int(clip_rounds), int(min_events)
    o.clip_sigma, o.scale_lo, o.scale_hi = float(clip_sigma), float(scale_lo), float(scale_hi)
    return o


make_rescale_out = functools.partial(make_out, NmodRescaleOut)


CALLS_TOO_LARGE = 16       # nmod_read_calls: status of a read beyond MAX_DEEP events
CALLS_WAVE_MAX = 2048      # nmod_read_calls: events of a read up to which one wave computes it (a workgroup beyond)
CALLS_EVENT_FIELDS = ('z', 'p', 'p_win')
SITE_FIELDS = ('n_valid', 'n_called', 'frac')


class NmodCallsOpts(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('nb', C.c_int32), ('alpha', C.c_double)]


class NmodCallsOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + \
               [(n, C.c_void_p) for n in CALLS_EVENT_FIELDS + ('n_sites', 'n_called', 'status')]


class NmodSiteOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in SITE_FIELDS]


def make_calls_opts(nb=2, alpha=0.01):
    o = NmodCallsOpts()
    o.struct_size = C.sizeof(NmodCallsOpts)
    o.nb, o.alpha = int(nb), float(alpha)
    return o


make_calls_out = functools.partial(make_out, NmodCallsOut)
make_site_out = functools.partial(make_out, NmodSiteOut)


LLR_MAX = 1e300            # nmod_read_llr: an event whose |llr| lies beyond is ineligible
LLR_PRIOR_LOGIT_MAX = 700.0
LLR_EVENT_FIELDS = ('llr', 'llr_win', 'p_mod')
LLR_READ_FIELDS = ('n_sites', 'n_mod', 'n_can', 'status')
SITE_LLR_FIELDS = ('n_valid', 'n_mod', 'n_can', 'frac')


class NmodLlrOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'nb_lo', 'nb_hi', 'reserved')] + [('thr', C.c_double), ('prior_logit', C.c_double)]


class NmodLlrOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in LLR_EVENT_FIELDS + LLR_READ_FIELDS]


class NmodSiteLlrOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in SITE_LLR_FIELDS]


def make_llr_opts(nb_lo=0, nb_hi=0, thr=2.5, prior_logit=0.0):
    o = NmodLlrOpts()
    o.struct_size = C.sizeof(NmodLlrOpts)
    o.nb_lo, o.nb_hi, o.thr, o.prior_logit = int(nb_lo), int(nb_hi), float(thr), float(prior_logit)
    return o


make_llr_out = functools.partial(make_out, NmodLlrOut)
make_site_llr_out = functools.partial(make_out, NmodSiteLlrOut)


STOICH_TOO_FEW, STOICH_FLAT, STOICH_NOT_CONVERGED, STOICH_AT_ZERO, STOICH_AT_ONE, STOICH_TOO_LARGE = 1, 2, 4, 8, 16, 32
STOICH_NO_ESTIMATE = STOICH_TOO_FEW | STOICH_FLAT | STOICH_TOO_LARGE
STOICH_SMALL, STOICH_WAVE = 256, 1024     # nmod_site_stoich: scores of a row up to which 16 lanes / one wave compute it (a workgroup beyond)
STOICH_MAX_ITER = 200
STOICH_CI_DROP_95 = 3.841458820694124     # the 0.95 quantile of chi2_1
STOICH_FIELDS = ('pi', 'pi_lo', 'pi_hi', 'stat', 'p_null')
STOICH_INT_FIELDS = ('n_valid', 'iters')


class NmodStoichOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'max_iter', 'min_valid', 'reserved')] + [('tol', C.c_double), ('ci_drop', C.c_double)]


class NmodStoichOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + \
               [(n, C.c_void_p) for n in STOICH_FIELDS + STOICH_INT_FIELDS + ('status', 'resp')]


def make_stoich_opts(max_iter=60, min_valid=3, tol=1e-12, ci_drop=STOICH_CI_DROP_95):
    o = NmodStoichOpts()
    o.struct_size = C.sizeof(NmodStoichOpts)
    o.max_iter, o.min_valid, o.tol, o.ci_drop = int(max_iter), int(min_valid), float(tol), float(ci_drop)
    return o


make_stoich_out = functools.partial(make_out, NmodStoichOut)


MULTI_MAX = 4              # nmod_read_llr_multi / nmod_site_compose: alternative tables (states beside canonical) of one call
MULTI_AMBIGUOUS, MULTI_NONE = 255, 254     # nmod_read_llr_multi: the call of an eligible event that is neither, of an ineligible event
LLR_MULTI_EVENT_FIELDS = ('llr', 'llr_win', 'post', 'call')
LLR_MULTI_READ_FIELDS = ('n_sites', 'n_can', 'n_mod', 'status')


class NmodLlrMultiOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'nb_lo', 'nb_hi', 'reserved')] + [('thr', C.c_double), ('prior_logit', C.c_double * MULTI_MAX)]


class NmodLlrMultiOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in LLR_MULTI_EVENT_FIELDS + LLR_MULTI_READ_FIELDS]


def make_llr_multi_opts(nb_lo=0, nb_hi=0, thr=2.5, prior_logit=()):
    o = NmodLlrMultiOpts()
    o.struct_size = C.sizeof(NmodLlrMultiOpts)
    o.nb_lo, o.nb_hi, o.thr = int(nb_lo), int(nb_hi), float(thr)
    for m, v in enumerate(prior_logit):
        o.prior_logit[m] = float(v)
    return o


make_llr_multi_out = functools.partial(make_out, NmodLlrMultiOut)


def model_ptr_array(models):
    """an array of pointers to the given nmod_rescale_model structs (keep both alive for the call)"""
    return (C.POINTER(NmodRescaleModel) * len(models))(*[C.pointer(m) for m in models])


COMPOSE_TOO_FEW, COMPOSE_NO_STATE, COMPOSE_NOT_CONVERGED, COMPOSE_DEGENERATE, COMPOSE_TOO_LARGE = 1, 2, 4, 8, 32
COMPOSE_NO_ESTIMATE = COMPOSE_TOO_FEW | COMPOSE_NO_STATE | COMPOSE_DEGENERATE | COMPOSE_TOO_LARGE
COMPOSE_MAX_ITER = 2000
COMPOSE_FIELDS = ('pi', 'll', 'stat', 'stat_m', 'p_m')
COMPOSE_INT_FIELDS = ('n_valid', 'n_partial', 'iters')


class NmodComposeOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'max_iter', 'min_valid', 'reserved')] + [('tol', C.c_double)]


class NmodComposeOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + \
               [(n, C.c_void_p) for n in COMPOSE_FIELDS + COMPOSE_INT_FIELDS + ('open_mask', 'status', 'resp')]


def make_compose_opts(max_iter=500, min_valid=3, tol=1e-9):
    o = NmodComposeOpts()
    o.struct_size = C.sizeof(NmodComposeOpts)
    o.max_iter, o.min_valid, o.tol = int(max_iter), int(min_valid), float(tol)
    return o


make_compose_out = functools.partial(make_out, NmodComposeOut)


DIFF_TOO_FEW, DIFF_FLAT, DIFF_NOT_CONVERGED, DIFF_POOL_AT_END, DIFF_TOO_LARGE = 1, 2, 4, 8, 32
DIFF_NO_ESTIMATE = DIFF_TOO_FEW | DIFF_FLAT | DIFF_TOO_LARGE
DIFF_SMALL, DIFF_WAVE = 128, 512          # nmod_site_diff: scores of the longer row up to which 16 lanes / one wave compute a site
DIFF_FIELDS = ('pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat', 'p_diff')
DIFF_INT_FIELDS = ('n_valid0', 'n_valid1', 'iters')


class NmodDiffOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'max_iter', 'min_valid', 'reserved')] + [('tol', C.c_double), ('ci_drop', C.c_double)]


class NmodDiffOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in DIFF_FIELDS + DIFF_INT_FIELDS + ('status',)]


def make_diff_opts(max_iter=60, min_valid=3, tol=1e-12, ci_drop=STOICH_CI_DROP_95):
    o = NmodDiffOpts()
    o.struct_size = C.sizeof(NmodDiffOpts)
    o.max_iter, o.min_valid, o.tol, o.ci_drop = int(max_iter), int(min_valid), float(tol), float(ci_drop)
    return o


make_diff_out = functools.partial(make_out, NmodDiffOut)


REP_TOO_FEW, REP_FLAT, REP_NOT_CONVERGED, REP_POOL_AT_END, REP_PHI_ZERO, REP_TOO_LARGE = 1, 2, 4, 8, 16, 32
REP_NO_ESTIMATE = REP_TOO_FEW | REP_FLAT | REP_TOO_LARGE
REP_BAD_PRIOR = 64          # nmod_site_diff_rep_mod: the record of the prior cannot be used
REP_PRIOR_WORDS = 8         # nmod_rep_prior: the doubles of its record, REP_PRIOR_FIELDS in order
REP_PRIOR_CHUNK = 1024      # nmod_rep_prior: consecutive sites per chunk of its sums
REP_PRIOR_FIELDS = ('d0', 's0sq', 'df_tot', 'ci_drop', 'n_used', 'n_zero', 'emean', 'evar')
REP_MAX_SAMPLES = 16        # nmod_site_diff_rep: the largest number of samples of a site (the smallest is 3)
REP_SAMPLE_FIELDS = ('pi_s',)                               # npos * G doubles
REP_FIELDS = ('pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat_cond', 'p_cond', 'stat_het', 'p_het', 'phi', 'p_rep')
REP_SAMPLE_INT_FIELDS = ('n_valid',)                        # npos * G int32
REP_INT_FIELDS = ('iters',)


class NmodRepOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'max_iter', 'min_valid', 'reserved')] + \
               [('tol', C.c_double), ('ci_drop', C.c_double), ('phi_floor', C.c_double)]


class NmodRepOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + \
               [(n, C.c_void_p) for n in REP_SAMPLE_FIELDS + REP_FIELDS + REP_SAMPLE_INT_FIELDS + REP_INT_FIELDS + ('status',)]


def make_rep_opts(max_iter=60, min_valid=3, tol=1e-12, ci_drop=STOICH_CI_DROP_95, phi_floor=0.0):
    o = NmodRepOpts()
    o.struct_size = C.sizeof(NmodRepOpts)
    o.max_iter, o.min_valid, o.tol, o.ci_drop, o.phi_floor = int(max_iter), int(min_valid), float(tol), float(ci_drop), float(phi_floor)
    return o


make_rep_out = functools.partial(make_out, NmodRepOut)


PAIRS_MAX_DIST = 65536      # nmod_pair_index: largest max_dist
PAIRS_LDS_MAX = 2048        # nmod_site_pairs: pairs up to which the read kernel keeps the call's table in LDS
PAIRS_THREAD_MAX = 64       # nmod_site_pairs: tables of a pair's support up to which one thread computes p_fisher (a wave beyond)
PAIRS_FORCE_DIRECT = 1      # nmod_pairs_opts.flags
PAIRS_TOO_FEW, PAIRS_DEGENERATE = 1, 2
PAIRS_INT_FIELDS = ('counts', 'first', 'second')
PAIRS_FIELDS = ('log_or', 'se', 'phi', 'p_fisher')


class NmodPairsOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'min_reads', 'flags', 'reserved')] + [('thr', C.c_double)]


class NmodPairsOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in PAIRS_INT_FIELDS + PAIRS_FIELDS + ('status',)]


def make_pairs_opts(thr=2.5, min_reads=10, flags=0):
    o = NmodPairsOpts()
    o.struct_size = C.sizeof(NmodPairsOpts)
    o.min_reads, o.flags, o.thr = int(min_reads), int(flags), float(thr)
    return o


make_pairs_out = functools.partial(make_out, NmodPairsOut)


LINK_TOO_FEW, LINK_FLAT, LINK_NOT_CONVERGED, LINK_AT_MIN, LINK_AT_MAX, LINK_TOO_LARGE, LINK_DEGENERATE = 1, 2, 4, 8, 16, 32, 64
LINK_NO_ESTIMATE = LINK_TOO_FEW | LINK_FLAT | LINK_TOO_LARGE
LINK_SMALL, LINK_WAVE = 256, 1024         # nmod_pair_linkage: reads of a row up to which 16 lanes / one wave compute it (K14's steps)
LINK_FIELDS = ('pa', 'pb', 'd', 'd_lo', 'd_hi', 'r', 'stat', 'p_indep')
LINK_INT_FIELDS = ('n_valid', 'iters')


class NmodLinkOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ('struct_size', 'max_iter', 'min_reads', 'reserved')] + [('tol', C.c_double), ('ci_drop', C.c_double)]


class NmodLinkOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in LINK_FIELDS + LINK_INT_FIELDS + ('status',)]


def make_link_opts(max_iter=60, min_reads=20, tol=1e-12, ci_drop=STOICH_CI_DROP_95):
    o = NmodLinkOpts()
    o.struct_size = C.sizeof(NmodLinkOpts)
    o.max_iter, o.min_reads, o.tol, o.ci_drop = int(max_iter), int(min_reads), float(tol), float(ci_drop)
    return o


make_link_out = functools.partial(make_out, NmodLinkOut)


HMM_CHUNK, HMM_WAVE_MAX = 4, 1024         # nmod_read_hmm: steps of a tile a thread owns; entries of a read up to which one wave computes it
HMM_NO_SITE = 1
HMM_ENTRY_FIELDS = ('post', 'site', 'state')
HMM_READ_FIELDS = ('n_sites', 'n_mod', 'n_can', 'n_runs', 'll', 'll_indep', 'status')
HMM_SITE_FIELDS = ('site_n', 'site_mod', 'site_can')


class NmodHmmOpts(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('pi', C.c_double), ('length', C.c_double), ('call_post', C.c_double)]


class NmodHmmOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in HMM_ENTRY_FIELDS + HMM_READ_FIELDS + HMM_SITE_FIELDS]


def make_hmm_opts(pi=0.5, length=200.0, call_post=0.9):
    o = NmodHmmOpts()
    o.struct_size = C.sizeof(NmodHmmOpts)
    o.pi, o.length, o.call_post = float(pi), float(length), float(call_post)
    return o


make_hmm_out = functools.partial(make_out, NmodHmmOut)


VIT_ENTRY_FIELDS = ('path', 'site', 'delta')   # nmod_read_viterbi; the constants and NMOD_HMM_NO_SITE are nmod_read_hmm's
VIT_READ_FIELDS = ('n_sites', 'n_mod', 'n_runs', 'vit', 'status')
VIT_SITE_FIELDS = ('site_n', 'site_mod')


class NmodVitOpts(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('pi', C.c_double), ('length', C.c_double)]


class NmodVitOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in VIT_ENTRY_FIELDS + VIT_READ_FIELDS + VIT_SITE_FIELDS]


def make_vit_opts(pi=0.5, length=200.0):
    o = NmodVitOpts()
    o.struct_size = C.sizeof(NmodVitOpts)
    o.pi, o.length = float(pi), float(length)
    return o


make_vit_out = functools.partial(make_out, NmodVitOut)


HMM_GRAD_READ_FIELDS = ('ll', 'g_eta', 'g_lam', 'abs_eta', 'abs_lam', 'status')   # nmod_read_hmm_grad; status: NMOD_HMM_NO_SITE
HMM_GRAD_SUMS = ('ll', 'g_eta', 'g_lam', 'g_eta2', 'g_eta_lam', 'g_lam2', 'n_reads', 'n_entries')   # the words of its `sums`


class NmodHmmGradOpts(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32), ('pi', C.c_double), ('length', C.c_double)]


class NmodHmmGradOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in HMM_GRAD_READ_FIELDS + ('sums',)]


def make_hmm_grad_opts(pi=0.5, length=200.0):
    o = NmodHmmGradOpts()
    o.struct_size = C.sizeof(NmodHmmGradOpts)
    o.pi, o.length = float(pi), float(length)
    return o


make_hmm_grad_out = functools.partial(make_out, NmodHmmGradOut)


CLASSES_MAX = 8                            # nmod_read_classes_step: classes of a fit
CLASSES_SMALL, CLASSES_WAVE = 64, 512      # rows of a site up to which 16 lanes compute it, up to which one wave does
CLASS_ROWS_FIELDS = ('site', 's', 'rread', 'soff', 'srow')             # nmod_read_class_rows
CLASSES_READ_FIELDS = ('gamma', 'll', 'cls', 'status')                 # nmod_read_classes_step; status: NMOD_HMM_NO_SITE
CLASSES_SITE_FIELDS = ('theta_out', 'n_site')
CLASSES_SUMS = ('ll', 'n_reads', 'n_entries', 'max_move')              # the first words of its `sums`; then sum gamma per class


class NmodClassRowsOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in CLASS_ROWS_FIELDS]


class NmodClassesOpts(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('n_classes', C.c_int32)]


class NmodClassesOut(C.Structure):
    _fields_ = [('struct_size', C.c_int32), ('reserved', C.c_int32)] + [(n, C.c_void_p) for n in CLASSES_READ_FIELDS + CLASSES_SITE_FIELDS
                                                                         + ('w_out', 'sums')]


def make_classes_opts(n_classes=2):
    o = NmodClassesOpts()
    o.struct_size = C.sizeof(NmodClassesOpts)
    o.n_classes = int(n_classes)
    return o


make_class_rows_out = functools.partial(make_out, NmodClassRowsOut)
make_classes_out = functools.partial(make_out, NmodClassesOut)


class NanomodLibraryError(RuntimeError):
    pass


_lib = None

# every symbol include/nanomod_hip.h declares: (restype, argtypes)
_SIGNATURES = {
    'nmod_abi_version': (C.c_int, []),
    'nmod_device_count': (C.c_int, []),
    'nmod_strerror': (C.c_char_p, [C.c_int]),
    'nmod_workspace_bytes': (C.c_int64, [C.POINTER(NmodParams), C.c_int64]),
    'nmod_item_claim_plan': (C.c_int, [C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]),
    'nmod_detect_batch': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(NmodOut)]),
    'nmod_combine_track': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    'nmod_synth_fill': (C.c_int, [C.POINTER(NmodParams), C.c_uint64, C.c_int64, C.c_int64, C.c_int32,
                                  C.c_int32, C.c_int64, C.c_float, C.c_void_p]),
    'nmod_synth_fill_csr': (C.c_int, [C.POINTER(NmodParams), C.c_uint64, C.c_int64, C.c_int64, C.c_int32,
                                      C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    'nmod_synth_fill_events': (C.c_int, [C.POINTER(NmodParams), C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    'nmod_evtimer_create': (C.c_int, [C.c_int32, C.POINTER(C.c_void_p)]),
    'nmod_evtimer_reset': (C.c_int, [C.c_void_p]),
    'nmod_evtimer_read': (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    'nmod_evtimer_destroy': (C.c_int, [C.c_void_p]),
    'nmod_selftest': (C.c_int, [C.c_int32]),
    'nmod_comm_unique_id': (C.c_int, [C.c_void_p]),
    'nmod_comm_init_rank': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    'nmod_allgather_tracks': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    'nmod_comm_destroy': (C.c_int, [C.c_void_p]),
    'nmod_narrow_probe': (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    'nmod_format_probe': (C.c_int, [C.POINTER(C.c_double), C.c_int64, C.c_int32, C.c_char_p, C.c_int64]),
    'nmod_trim_scratch': (C.c_int, [C.c_int32]),
    'nmod_host_pipeline_config': (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    'nmod_last_host_stats': (C.c_int, [C.POINTER(NmodHostStats)]),
    'nmod_last_dispatch_stats': (C.c_int, [C.POINTER(NmodDispatchStats)]),
    'nmod_build_info': (C.c_char_p, []),
    'nmod_downsample_ks': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int32, C.c_double, C.c_uint64, C.c_void_p, C.c_void_p]),
    'nmod_argsort_keys': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p]),
    'nmod_describe_dispatch': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int64, C.c_char_p, C.c_int32]),
    'nmod_write_sign_test': (C.c_int, [C.c_char_p, C.c_int64, C.c_void_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_void_p,
                                       C.c_char_p] + [C.c_void_p] * 10 + [C.c_int32]),
    'nmod_rank_order': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'nmod_region_rank': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p,
                                   C.c_int32, C.c_int32, C.c_char, C.c_double, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]),
    'nmod_fdr_adjust': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_double,
                                  C.POINTER(C.c_void_p), C.c_void_p]),
    'nmod_mix_fraction': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_double, C.c_void_p, C.c_double, C.POINTER(NmodMixOut)]),
    'nmod_one_sample': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 6 + [C.POINTER(NmodOneOut)]),
    'nmod_kmer_model': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.POINTER(NmodKmerOut)]),
    'nmod_kmer_mix': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                C.POINTER(NmodKmixOpts), C.POINTER(NmodKmixOut)]),
    'nmod_rescale_reads': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NmodRescaleModel),
                                     C.POINTER(NmodRescaleOpts), C.POINTER(NmodRescaleOut)]),
    'nmod_read_calls': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NmodRescaleModel),
                                  C.POINTER(NmodCallsOpts), C.POINTER(NmodCallsOut)]),
    'nmod_site_calls': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(NmodSiteOut)]),
    'nmod_read_llr': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NmodRescaleModel),
                                C.POINTER(NmodRescaleModel), C.POINTER(NmodLlrOpts), C.POINTER(NmodLlrOut)]),
    'nmod_site_llr': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(NmodSiteLlrOut)]),
    'nmod_site_stoich': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(NmodStoichOpts), C.POINTER(NmodStoichOut)]),
    'nmod_read_llr_multi': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NmodRescaleModel),
                                      C.c_int32, C.c_void_p, C.POINTER(NmodLlrMultiOpts), C.POINTER(NmodLlrMultiOut)]),
    'nmod_read_llr_multi_table_in_lds': (C.c_int, [C.c_int32, C.c_int32]),
    'nmod_site_compose': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(NmodComposeOpts),
                                    C.POINTER(NmodComposeOut)]),
    'nmod_site_compose_stage_reads': (C.c_int64, [C.c_int32]),
    'nmod_site_diff': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NmodDiffOpts),
                                 C.POINTER(NmodDiffOut)]),
    'nmod_site_diff_rep': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(NmodRepOpts),
                                     C.POINTER(NmodRepOut)]),
    'nmod_rep_prior': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    'nmod_site_diff_rep_mod': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(NmodRepOpts),
                                         C.POINTER(NmodRepOut), C.c_void_p, C.c_void_p]),
    'nmod_pair_index': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    'nmod_site_pairs': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.POINTER(NmodPairsOpts), C.POINTER(NmodPairsOut)]),
    'nmod_pair_rows_count': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.POINTER(C.c_int64)]),
    'nmod_pair_rows_fill': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'nmod_pair_linkage': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NmodLinkOpts),
                                    C.POINTER(NmodLinkOut)]),
    'nmod_read_sites_count': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p,
                                        C.POINTER(C.c_int64)]),
    'nmod_read_hmm': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                C.POINTER(NmodHmmOpts), C.POINTER(NmodHmmOut)]),
    'nmod_read_viterbi': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.POINTER(NmodVitOpts), C.POINTER(NmodVitOut)]),
    'nmod_read_hmm_grad': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.POINTER(NmodHmmGradOpts), C.POINTER(NmodHmmGradOut)]),
    # K23: the three entries above with site_pi (float64[nsites]) after key
    'nmod_read_hmm_prior': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.POINTER(NmodHmmOpts), C.POINTER(NmodHmmOut)]),
    'nmod_read_viterbi_prior': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int64, C.POINTER(NmodVitOpts), C.POINTER(NmodVitOut)]),
    'nmod_read_hmm_grad_prior': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_int64, C.POINTER(NmodHmmGradOpts), C.POINTER(NmodHmmGradOut)]),
    'nmod_read_class_rows': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 4 + [C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.POINTER(NmodClassRowsOut)]),
    'nmod_read_classes_step': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 6
                               + [C.POINTER(NmodClassesOpts), C.c_void_p, C.c_void_p, C.POINTER(NmodClassesOut)]),
    'nmod_pivot_reads': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int32] + [C.c_void_p] * 5 + [C.c_int64, C.c_int64, C.c_int64]
                         + [C.c_void_p] * 4 + [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'nmod_select_tested': (C.c_int, [C.POINTER(NmodParams), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4
                           + [C.POINTER(C.c_int64)] * 3 + [C.POINTER(C.c_int32)]),
    'nmod_gather_tested': (C.c_int, [C.POINTER(NmodParams), C.c_int64] + [C.c_void_p] * 9 + [C.c_int32] + [C.c_void_p] * 8),
}


def load():
    """Load the HIP library (once).  Raises NanomodLibraryError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NanomodLibraryError(
            'libnanomod_hip.so not found at %s. Build it with `python -c "import __graft_entry__ as g; '
            'g.build()"` or `make -C nanomod_amd/csrc`. There is no CPU fallback.' % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 and the package
    # uses torch for device memory and streams, so let torch load its copy first; the loader then
    # binds our DT_NEEDED libamdhip64.so.7 to that already-loaded object (same SONAME).  Loading in
    # the other order leaves two runtimes in the process and torch then sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    if lib.nmod_abi_version() != NMOD_ABI_VERSION:
        raise NanomodLibraryError('ABI version mismatch: library %d, binding %d'
                                  % (lib.nmod_abi_version(), NMOD_ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what='nanomod_hip'):
    if rc != 0:
        msg = load().nmod_strerror(rc).decode()
        raise NanomodLibraryError('%s failed: %s (code %d)' % (what, msg, rc))


def make_params(device=0, stream=0, memspace=MEM_HOST, dtype=DTYPE_F32, tests=TEST_ALL,
                method=METHOD_STOUFFER, nb=2, weights_dif=2.0, want_mstd=0,
                stride0=0, stride1=0, max_n0=0, max_n1=0, timer=None, flags=0):
    p = NmodParams()
    p.struct_size = C.sizeof(NmodParams)
    p.device = device
    p.stream = stream or None
    p.memspace = memspace
    p.dtype = dtype
    p.tests = tests
    p.method = method
    p.nb = nb
    p.want_mstd = want_mstd
    p.weights_dif = weights_dif
    p.stride0 = stride0
    p.stride1 = stride1
    p.max_n0 = max_n0
    p.max_n1 = max_n1
    p.timer = timer
    p.flags = flags
    p.reserved = 0
    return p
