"""Batch entry points over the C ABI.

`detect_host`   — numpy arrays in host memory (the drop-in `mtest2` path uses it).
`detect_device` — torch tensors already resident in HBM (bench / sharded path);
                  torch is used only for device memory and the current stream.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _check_csr(off, npos, name):
    if off is None:
        return
    if off.dtype != np.int64 or off.ndim != 1 or off.shape[0] != npos + 1:
        raise ValueError('%s must be int64[npos+1]' % name)


_warm = {}


def warm_up(device=0):
    """Start the HIP runtime, the device context and the code object of the library on a background thread (about a
    second in a fresh process) while the caller prepares its inputs on the host; detect_host joins it.  Idempotent."""
    import threading
    if device in _warm:
        return _warm[device]

    def run():
        try:
            L.load().nmod_selftest(int(device))          # a 64-thread kernel: forces context creation and module load
        except Exception:                                # (errors surface in the real call, with their message)
            pass
    t = threading.Thread(target=run, name='nanomod-warm-up', daemon=True)
    if not _warm:
        # a caller that fails before detect_host joins the thread (build_csr raising, say) must not let the interpreter
        # shut down while the HIP runtime is still initialising on it
        import atexit
        atexit.register(lambda: [_join_warm_up(d) for d in list(_warm)])
    _warm[device] = t
    t.start()
    return t


def _join_warm_up(device):
    t = _warm.get(device)
    if t is not None and t.is_alive():
        t.join()


def detect_host(sig0, off0, sig1, off1, run_id, *, nb=2, weights_dif=2.0, method='stouffer',
                tests=L.TEST_ALL, want_mstd=False, device=0, stride0=0, stride1=0, flags=0, deep=False, out=None):
    """Run the hot path on host-resident CSR inputs; returns a dict of numpy arrays.

    sig0/sig1: float32 (canonical), int16 (milli-units) or float64 1-D arrays; off0/off1:
    int64[npos+1] (or None with a fixed stride); run_id: int32[npos]; flags: L.FLAG_* (include/nanomod_hip.h).
    out: the dict a previous call of the same shape returned — its arrays are written again instead of allocating
    (and first-touching) new ones: at 4.6 M positions the page faults of fresh result arrays cost as much as 15 % of
    the PCIe-bound call."""
    lib = L.load()
    _join_warm_up(device)
    sig0 = np.ascontiguousarray(sig0)
    sig1 = np.ascontiguousarray(sig1)
    if sig0.dtype != sig1.dtype or sig0.dtype not in (np.float32, np.int16, np.float64):
        raise ValueError('sig0/sig1 must both be float32, both int16 (milli-units) or both float64')
    # float64 (what the reference holds): the library re-encodes it on the device, NMOD_DTYPE_F64
    dtype = {np.dtype(np.float32): L.DTYPE_F32, np.dtype(np.int16): L.DTYPE_I16_MILLI, np.dtype(np.float64): L.DTYPE_F64}[sig0.dtype]
    if off0 is not None:
        npos = len(off0) - 1
    elif off1 is not None:
        npos = len(off1) - 1
    else:
        npos = sig0.shape[0] // stride0
    off0 = None if off0 is None else np.ascontiguousarray(off0, dtype=np.int64)
    off1 = None if off1 is None else np.ascontiguousarray(off1, dtype=np.int64)
    _check_csr(off0, npos, 'off0')
    _check_csr(off1, npos, 'off1')
    method_id = L.METHOD_BY_NAME[method] if isinstance(method, str) else method
    run = None
    if run_id is not None:
        run = np.ascontiguousarray(run_id, dtype=np.int32)
        if run.shape[0] != npos:
            raise ValueError('run_id must be int32[npos]')
    if deep:
        flags = int(flags) | L.FLAG_DEEP
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype, tests=tests, method=method_id,
                        nb=nb, weights_dif=weights_dif, want_mstd=int(bool(want_mstd)),
                        stride0=stride0 if off0 is None else 0, stride1=stride1 if off1 is None else 0, flags=flags)
    res = {}
    wanted = []
    if tests & L.TEST_MWU:
        wanted += ['mwu_u', 'mwu_p']
    if tests & L.TEST_WELCH:
        wanted += ['t_t', 't_p']
    if (tests & L.TEST_KS) or method_id != L.METHOD_KS:
        wanted += ['ks_d', 'ks_p']
    if method_id != L.METHOD_KS:
        wanted += ['comb_st', 'comb_p']
    if want_mstd:
        wanted += ['mean0', 'std0', 'mean1', 'std1']
    reuse = out
    out = L.NmodOut()
    for name in wanted:
        if reuse is not None:
            a = reuse[name]
            if a.dtype != np.float64 or a.shape != (npos,) or not a.flags.c_contiguous:
                raise ValueError('out[%r] must be a contiguous float64[npos] array' % name)
            res[name] = a
        else:
            res[name] = np.empty(npos, dtype=np.float64)      # (every element is written: finalize_kernel stores all positions)
        setattr(out, name, _np_ptr(res[name]))
    if reuse is not None:
        res['status'] = reuse['status']
        if res['status'].dtype != np.uint8 or res['status'].shape != (npos,):
            raise ValueError("out['status'] must be a uint8[npos] array")
    else:
        res['status'] = np.empty(npos, dtype=np.uint8)
    out.status = _np_ptr(res['status'])
    rc = lib.nmod_detect_batch(C.byref(prm), npos, _np_ptr(sig0), _np_ptr(off0), _np_ptr(sig1), _np_ptr(off1),
                               _np_ptr(run), None, 0, C.byref(out))
    L.check(rc, 'nmod_detect_batch')
    return res


def combine_host(ks_d, ks_p, run_id, *, nb=2, weights_dif=2.0, method='stouffer', device=0):
    lib = L.load()
    ks_p = np.ascontiguousarray(ks_p, dtype=np.float64)
    ks_d = np.ascontiguousarray(ks_d, dtype=np.float64)
    run = np.ascontiguousarray(run_id, dtype=np.int32)
    npos = ks_p.shape[0]
    method_id = L.METHOD_BY_NAME[method] if isinstance(method, str) else method
    prm = L.make_params(device=device, memspace=L.MEM_HOST, method=method_id, nb=nb, weights_dif=weights_dif)
    st = np.empty(npos, dtype=np.float64)
    pv = np.empty(npos, dtype=np.float64)
    rc = lib.nmod_combine_track(C.byref(prm), npos, _np_ptr(ks_d), _np_ptr(ks_p), _np_ptr(run), _np_ptr(st), _np_ptr(pv))
    L.check(rc, 'nmod_combine_track')
    return st, pv


def rank_order_host(key_primary, key_second, key_third, descending=False, device=0):
    """myDetect.py:447-462 on the device: the order of Python's stable sorted() by the tuple
    (key_primary, key_second, key_third), reversed as a whole when `descending` (rankUse == 'st')."""
    lib = L.load()
    ks = [np.ascontiguousarray(k, dtype=np.float64) for k in (key_primary, key_second, key_third)]
    n = ks[0].shape[0]
    order = np.empty(n, dtype=np.int32)
    prm = L.make_params(device=device, memspace=L.MEM_HOST)
    rc = lib.nmod_rank_order(C.byref(prm), n, _np_ptr(ks[0]), _np_ptr(ks[1]), _np_ptr(ks[2]), 1 if descending else 0, _np_ptr(order))
    L.check(rc, 'nmod_rank_order')
    return order


def argsort_device(key):
    """stable ascending order of an int64 CUDA tensor (nmod_argsort_keys: the library's radix sort), as an int64 CUDA tensor"""
    import torch
    assert key.is_cuda and key.dtype == torch.int64 and key.is_contiguous()
    n = key.numel()
    order = torch.empty(n, dtype=torch.int32, device=key.device)
    prm = L.make_params(device=key.device.index or 0, memspace=L.MEM_DEVICE, stream=torch.cuda.current_stream(key.device).cuda_stream)
    L.check(L.load().nmod_argsort_keys(C.byref(prm), n, key.data_ptr(), order.data_ptr()), 'nmod_argsort_keys')
    return order.to(torch.int64)


FDR_SUMMARY_FIELDS = ('tested', 'excluded', 'rejected', 'p_crit')


def _fdr_method(method):
    if isinstance(method, str):
        if method not in L.FDR_BY_NAME:
            raise ValueError("fdr method must be 'bh' or 'by', not %r" % (method,))
        return L.FDR_BY_NAME[method]
    return int(method)


def fdr_adjust_host(tracks, method='bh', alpha=0.05, device=0):
    """Benjamini-Hochberg ('bh') or Benjamini-Yekutieli ('by') q-values of whole p-value tracks (nmod_fdr_adjust), one family per
    track: a float64 array or a list of up to eight of equal length.  An element outside [0, 1] (NaN included) gets q = NaN and
    is left out of the family.  Returns (list of q arrays, list of summary dicts: tested, excluded, rejected, p_crit)."""
    lib = L.load()
    if isinstance(tracks, np.ndarray) and tracks.ndim == 1:
        tracks = [tracks]
    ps = [np.ascontiguousarray(t, dtype=np.float64) for t in tracks]
    n = ps[0].shape[0] if ps else 0
    if any(t.ndim != 1 or t.shape[0] != n for t in ps):
        raise ValueError('fdr_adjust_host: the tracks must be one-dimensional and of one length')
    qs = [np.empty(n, dtype=np.float64) for _ in ps]
    nt = len(ps)
    parr = (C.c_void_p * max(nt, 1))(*[t.ctypes.data for t in ps])
    qarr = (C.c_void_p * max(nt, 1))(*[t.ctypes.data for t in qs])
    summ = (L.NmodFdrSummary * max(nt, 1))()
    prm = L.make_params(device=device, memspace=L.MEM_HOST)
    rc = lib.nmod_fdr_adjust(C.byref(prm), n, nt, parr, _fdr_method(method), float(alpha), qarr, C.cast(summ, C.c_void_p))
    L.check(rc, 'nmod_fdr_adjust')
    return qs, [{f: getattr(summ[t], f) for f in FDR_SUMMARY_FIELDS} for t in range(nt)]


def fdr_summary_dicts(summary):
    """the device tensor of DeviceDetector.fdr (ntracks x 4 float64 words) as summary dicts; synchronises"""
    raw = summary.cpu().numpy()
    counts = raw.view(np.int64)
    return [dict(tested=int(counts[t, 0]), excluded=int(counts[t, 1]), rejected=int(counts[t, 2]), p_crit=float(raw[t, 3]))
            for t in range(raw.shape[0])]


def _mix_args(mix_group, model, max_iter, tol):
    """the checked (mix_group, model id, max_iter, tol) of a mix call: ValueError for what the library would refuse"""
    if isinstance(model, str):
        if model not in L.MIX_BY_NAME:
            raise ValueError("mix model must be 'equal' or 'free', not %r" % (model,))
        model = L.MIX_BY_NAME[model]
    if model not in (L.MIX_EQUAL_VAR, L.MIX_FREE_VAR):
        raise ValueError('mix model must be 0 (equal variance) or 1 (free variance), not %r' % (model,))
    if mix_group not in (0, 1):
        raise ValueError('mix_group must be 0 (sig0 is the mixed group) or 1 (sig1 is), not %r' % (mix_group,))
    if int(max_iter) != max_iter or not 1 <= int(max_iter) <= 10000:
        raise ValueError('max_iter must be an integer in 1 .. 10000, not %r' % (max_iter,))
    tol = float(tol)
    if not (tol >= 0.0) or tol == float('inf'):
        raise ValueError('tol must be finite and >= 0, not %r' % (tol,))
    return int(mix_group), int(model), int(max_iter), tol


def mix_fraction_host(sig0, off0, sig1, off1, *, mix_group=1, model='equal', max_iter=200, tol=1e-6, gate=None, gate_max=0.05,
                      want_resp=False, device=0, stride0=0, stride1=0):
    """Per-position modified fraction by a two-component EM (nmod_mix_fraction, include/nanomod_hip.h) on host-resident rows:
    one group is the reference ("unmodified") group, the other (mix_group: 0 = sig0, 1 = sig1) a mixture of unmodified reads and
    reads at another level.  model 'equal' / 'free': the modified component shares the reference variance or has its own.
    gate: a float64 track, position i is computed iff gate[i] <= gate_max (NaN: not), e.g. the q-values of fdr_adjust_host.
    Returns a dict of numpy arrays: pi, mu_mod, sd_mod, llr (float64; llr is a score without a p-value), iters (int32), status
    (uint8, L.MIX_* bits) and with want_resp `resp` (float32, the posterior of every read of the mixed group, in its layout)."""
    lib = L.load()
    mix_group, model, max_iter, tol = _mix_args(mix_group, model, max_iter, tol)
    _join_warm_up(device)
    sig0 = np.ascontiguousarray(sig0)
    sig1 = np.ascontiguousarray(sig1)
    if sig0.dtype != sig1.dtype or sig0.dtype not in (np.float32, np.int16, np.float64):
        raise ValueError('sig0/sig1 must both be float32, both int16 (milli-units) or both float64')
    dtype = _dtype_code(sig0.dtype)
    if off0 is not None:
        npos = len(off0) - 1
    elif off1 is not None:
        npos = len(off1) - 1
    else:
        npos = sig0.shape[0] // stride0
    off0 = None if off0 is None else np.ascontiguousarray(off0, dtype=np.int64)
    off1 = None if off1 is None else np.ascontiguousarray(off1, dtype=np.int64)
    _check_csr(off0, npos, 'off0')
    _check_csr(off1, npos, 'off1')
    for sig, off, stride, name in ((sig0, off0, stride0, 'sig0'), (sig1, off1, stride1, 'sig1')):
        if npos and sig.shape[0] < (int(off[-1]) if off is not None else npos * stride):
            raise ValueError('%s is shorter than its offsets / stride say' % name)
    if gate is not None:
        gate = np.ascontiguousarray(gate, dtype=np.float64)
        if gate.shape != (npos,):
            raise ValueError('gate must be float64[npos]')
    res = {k: np.empty(npos, dtype=np.float64) for k in L.MIX_FIELDS}
    res['iters'] = np.empty(npos, dtype=np.int32)
    res['status'] = np.empty(npos, dtype=np.uint8)
    if want_resp:
        ysig, yoff, ystride = (sig1, off1, stride1) if mix_group == 1 else (sig0, off0, stride0)
        res['resp'] = np.empty((int(yoff[-1]) if yoff is not None else npos * ystride) if npos else 0, dtype=np.float32)
    out = L.NmodMixOut()
    for k, a in res.items():
        setattr(out, k, _np_ptr(a))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype, stride0=stride0 if off0 is None else 0,
                        stride1=stride1 if off1 is None else 0)
    rc = lib.nmod_mix_fraction(C.byref(prm), npos, _np_ptr(sig0), _np_ptr(off0), _np_ptr(sig1), _np_ptr(off1), mix_group, model,
                               max_iter, tol, _np_ptr(gate), float(gate_max), C.byref(out))
    L.check(rc, 'nmod_mix_fraction')
    return res


def one_sample_host(sig, off, ref_mean, ref_sd, ref_n=None, run_id=None, *, stride=0, nb=2, weights_dif=2.0, method='stouffer', device=0):
    """One read group against a stored per-position reference (nmod_one_sample, include/nanomod_hip.h) on host-resident rows:
    sig float32, int16 (milli-units) or float64, rows by `off` (int64[npos + 1]) or a fixed `stride`; ref_mean / ref_sd float64[npos]
    (sd with ddof = 0), ref_n int32[npos] for a stored control (Welch t from the statistics) or None for a model (one-sample t).
    Returns a dict of numpy arrays: ks_d, ks_p, t_t, t_p, shift, mean, std (float64), status (uint8, L.STATUS_* bits) and, when
    method is not 'ks' (run_id is then required), comb_st / comb_p: the window combine of the KS track."""
    lib = L.load()
    _join_warm_up(device)
    sig = np.ascontiguousarray(sig)
    if sig.dtype not in (np.float32, np.int16, np.float64):
        raise ValueError('sig must be float32, int16 (milli-units) or float64')
    ref_mean = np.ascontiguousarray(ref_mean, dtype=np.float64)
    ref_sd = np.ascontiguousarray(ref_sd, dtype=np.float64)
    npos = ref_mean.shape[0]
    off = None if off is None else np.ascontiguousarray(off, dtype=np.int64)
    _check_csr(off, npos, 'off')
    if ref_sd.shape != (npos,):
        raise ValueError('ref_sd must be float64[npos]')
    if npos and sig.shape[0] < (int(off[-1]) if off is not None else npos * stride):
        raise ValueError('sig is shorter than its offsets / stride say')
    if ref_n is not None:
        ref_n = np.ascontiguousarray(ref_n, dtype=np.int32)
        if ref_n.shape != (npos,):
            raise ValueError('ref_n must be int32[npos]')
    method_id = L.METHOD_BY_NAME[method] if isinstance(method, str) else method
    run = None
    if run_id is not None:
        run = np.ascontiguousarray(run_id, dtype=np.int32)
        if run.shape != (npos,):
            raise ValueError('run_id must be int32[npos]')
    names = [k for k in L.ONE_FIELDS if method_id != L.METHOD_KS or not k.startswith('comb_')]
    res = {k: np.empty(npos, dtype=np.float64) for k in names}
    res['status'] = np.empty(npos, dtype=np.uint8)
    out = L.make_one_out(**{k: _np_ptr(a) for k, a in res.items()})
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=_dtype_code(sig.dtype), method=method_id, nb=nb,
                        weights_dif=weights_dif, stride0=stride if off is None else 0)
    rc = lib.nmod_one_sample(C.byref(prm), npos, _np_ptr(sig), _np_ptr(off), _np_ptr(ref_mean), _np_ptr(ref_sd), _np_ptr(ref_n),
                             _np_ptr(run), C.byref(out))
    L.check(rc, 'nmod_one_sample')
    return res


def kmer_model_host(sig, off, code, ncodes, keep_lo=None, keep_hi=None, *, stride=0, device=0):
    """Per-code level models of host-resident rows (nmod_kmer_model, include/nanomod_hip.h): sig float32, int16 (milli-units) or
    float64, rows by `off` (int64[npos + 1]) or a fixed `stride`; code int32[npos] in [-1, ncodes) (-1: the position takes no part);
    keep_lo / keep_hi float64[ncodes] (inclusive bounds of the kept samples per code) or both None.  Returns a dict of numpy arrays:
    n_positions, n_samples, n_clipped (int64[ncodes]), mean, sd (float64[ncodes], NaN for a code without kept samples) and
    pos_status (uint8[npos], L.STATUS_* bits of the positions dropped whole)."""
    lib = L.load()
    _join_warm_up(device)
    sig = np.ascontiguousarray(sig)
    if sig.dtype not in (np.float32, np.int16, np.float64):
        raise ValueError('sig must be float32, int16 (milli-units) or float64')
    code = np.ascontiguousarray(code, dtype=np.int32)
    npos = code.shape[0]
    off = None if off is None else np.ascontiguousarray(off, dtype=np.int64)
    _check_csr(off, npos, 'off')
    if code.ndim != 1:
        raise ValueError('code must be int32[npos]')
    if npos and sig.shape[0] < (int(off[-1]) if off is not None else npos * stride):
        raise ValueError('sig is shorter than its offsets / stride say')
    ncodes = int(ncodes)
    if (keep_lo is None) != (keep_hi is None):
        raise ValueError('keep_lo and keep_hi come together')
    if keep_lo is not None:
        keep_lo = np.ascontiguousarray(keep_lo, dtype=np.float64)
        keep_hi = np.ascontiguousarray(keep_hi, dtype=np.float64)
        if keep_lo.shape != (ncodes,) or keep_hi.shape != (ncodes,):
            raise ValueError('keep_lo / keep_hi must be float64[ncodes]')
    m = max(ncodes, 0)
    res = {k: np.empty(m, dtype=np.int64) for k in L.KMER_COUNT_FIELDS}
    res['mean'] = np.empty(m, dtype=np.float64)
    res['sd'] = np.empty(m, dtype=np.float64)
    res['pos_status'] = np.empty(npos, dtype=np.uint8)
    out = L.make_kmer_out(**{k: _np_ptr(a) for k, a in res.items()})
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=_dtype_code(sig.dtype), stride0=stride if off is None else 0)
    rc = lib.nmod_kmer_model(C.byref(prm), npos, _np_ptr(sig), _np_ptr(off), _np_ptr(code), ncodes, _np_ptr(keep_lo), _np_ptr(keep_hi),
                             C.byref(out))
    L.check(rc, 'nmod_kmer_model')
    return res


def _rescale_opts(mode, weighted, clip_sigma, clip_rounds, min_events, scale_range, k=None, center=None):
    """nmod_rescale_opts from the Python arguments; ValueError for what the C entry refuses"""
    import math
    if isinstance(mode, str):
        if mode not in L.RESCALE_MODE_BY_NAME:
            raise ValueError("mode must be one of 'fit_apply', 'fit_only', 'apply_only'")
        mode = L.RESCALE_MODE_BY_NAME[mode]
    if mode not in (L.RESCALE_FIT_APPLY, L.RESCALE_FIT_ONLY, L.RESCALE_APPLY_ONLY):
        raise ValueError('unknown rescale mode %r' % (mode,))
    clip_sigma, clip_rounds, min_events = float(clip_sigma), int(clip_rounds), int(min_events)
    lo, hi = (float(v) for v in scale_range)
    if not 0 <= clip_rounds <= 8:
        raise ValueError('clip_rounds must be in 0 .. 8')
    if clip_rounds > 0 and not (math.isfinite(clip_sigma) and clip_sigma > 0.0):
        raise ValueError('clip_sigma must be finite and positive')
    if min_events < 2:
        raise ValueError('min_events must be at least 2')
    if not (math.isfinite(lo) and lo > 0.0 and lo <= hi):
        raise ValueError('scale_range must be (lo, hi) with 0 < lo <= hi, lo finite')
    if mode != L.RESCALE_APPLY_ONLY:
        if k is None or not 1 <= int(k) <= 8:
            raise ValueError('k must be in 1 .. 8')
        if not 0 <= int(center) < int(k):
            raise ValueError('center must be in 0 .. k - 1')
    return L.make_rescale_opts(mode, weighted, clip_sigma, clip_rounds, min_events, lo, hi)


def rescale_reads_host(val, off, base, model=None, *, mode='fit_apply', weighted=True, clip_sigma=3.0, clip_rounds=2, min_events=50,
                       scale_range=(0.5, 2.0), shift=None, scale=None, device=0):
    """Per-read shift and scale against a k-mer model and the rescaled events (nmod_rescale_reads, include/nanomod_hip.h) on
    host-resident reads: val float32, int16 (milli-units) or float64 and base (S1 / uint8), one entry per event, reads by `off`
    (int64[nreads + 1]); model: a mapping with k, center, mean, sd (a kmermodel model) — not needed for mode 'apply_only', which
    takes shift / scale (float64[nreads]) instead.  Returns a dict of numpy arrays: shift, scale (float64), n_used (int32), status
    (uint8, L.RESCALE_* bits) and, unless mode is 'fit_only', val: the rescaled events in val's dtype."""
    lib = L.load()
    val = np.ascontiguousarray(val)
    if val.dtype not in (np.float32, np.int16, np.float64):
        raise ValueError('val must be float32, int16 (milli-units) or float64')
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off.ndim != 1 or off.shape[0] < 1:
        raise ValueError('off must be int64[nreads + 1]')
    nreads = off.shape[0] - 1
    if nreads and (off[0] < 0 or bool(np.any(np.diff(off) < 0))):
        raise ValueError('off must start at or above 0 and never decrease')
    nev = int(off[-1]) if nreads else 0
    if val.ndim != 1 or val.shape[0] < nev:
        raise ValueError('val is shorter than its offsets say')
    k = center = None
    mean = sd = None
    if model is not None:
        k, center = int(model['k']), int(model['center'])
    opts = _rescale_opts(mode, weighted, clip_sigma, clip_rounds, min_events, scale_range, k, center)
    fit, apply = opts.mode != L.RESCALE_APPLY_ONLY, opts.mode != L.RESCALE_FIT_ONLY
    m = L.NmodRescaleModel()
    if fit:
        mean = np.ascontiguousarray(model['mean'], dtype=np.float64)
        sd = np.ascontiguousarray(model['sd'], dtype=np.float64)
        if mean.shape != (4 ** k,) or sd.shape != (4 ** k,):
            raise ValueError('model mean / sd must be float64[4^k]')
        base = np.asarray(base)
        base = np.ascontiguousarray(base if base.dtype == np.uint8 else base.astype('S1').view(np.uint8))
        if base.ndim != 1 or base.shape[0] < nev:
            raise ValueError('base is shorter than its offsets say')
        m.k, m.center, m.mean, m.sd = k, center, mean.ctypes.data, sd.ctypes.data
        shift_a, scale_a = np.empty(nreads, np.float64), np.empty(nreads, np.float64)
    else:
        if shift is None or scale is None:
            raise ValueError("mode 'apply_only' needs shift and scale")
        shift_a = np.array(shift, dtype=np.float64, order='C')
        scale_a = np.array(scale, dtype=np.float64, order='C')
        if shift_a.shape != (nreads,) or scale_a.shape != (nreads,):
            raise ValueError('shift / scale must be float64[nreads]')
        base = None
    res = dict(shift=shift_a, scale=scale_a, n_used=np.zeros(nreads, np.int32), status=np.zeros(nreads, np.uint8))
    if apply:
        res['val'] = np.empty_like(val)
        res['val'][nev:] = val[nev:]
    if nreads and off[0] > 0 and apply:
        res['val'][:off[0]] = val[:off[0]]
    _join_warm_up(device)
    out = L.make_rescale_out(shift=_np_ptr(shift_a), scale=_np_ptr(scale_a), n_used=_np_ptr(res['n_used']), status=_np_ptr(res['status']),
                             val_out=_np_ptr(res['val']) if apply else None)
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=_dtype_code(val.dtype))
    rc = lib.nmod_rescale_reads(C.byref(prm), nreads, _np_ptr(off), _np_ptr(val), _np_ptr(base), C.byref(m), C.byref(opts), C.byref(out))
    L.check(rc, 'nmod_rescale_reads')
    return res


def _calls_opts(nb, alpha, k, center, want):
    """nmod_calls_opts from the Python arguments; ValueError for what the C entry refuses"""
    nb, alpha = int(nb), float(alpha)
    if not 0 <= nb <= L.MAX_NB:
        raise ValueError('nb must be in 0 .. %d' % L.MAX_NB)
    if not 0.0 < alpha <= 1.0:
        raise ValueError('alpha must be in (0, 1]')
    if k is None or not 1 <= int(k) <= 8:
        raise ValueError('k must be in 1 .. 8')
    if center is None or not 0 <= int(center) < int(k):
        raise ValueError('center must be in 0 .. k - 1')
    want = tuple(want)
    if any(w not in L.CALLS_EVENT_FIELDS for w in want):
        raise ValueError("want must name tracks of 'z', 'p', 'p_win'")
    return L.make_calls_opts(nb, alpha), want


def read_calls_host(val, off, base, model, *, nb=2, alpha=0.01, want=('z', 'p', 'p_win'), device=0):
    """Per-read modification calls against a k-mer model (nmod_read_calls, include/nanomod_hip.h) on host-resident reads: val
    float32, int16 (milli-units) or float64 and base (S1 / uint8), one entry per event, reads by `off` (int64[nreads + 1]); model: a
    mapping with k, center, mean, sd (a kmermodel model).  Returns a dict of numpy arrays: the per-event tracks named in `want`
    (float64, in val's layout: z, the two-sided normal p, and p_win, Fisher's combination over the events of the same read within nb)
    and per read n_sites, n_called (int32) and status (uint8, L.CALLS_TOO_LARGE)."""
    lib = L.load()
    val = np.ascontiguousarray(val)
    if val.dtype not in (np.float32, np.int16, np.float64):
        raise ValueError('val must be float32, int16 (milli-units) or float64')
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off.ndim != 1 or off.shape[0] < 1:
        raise ValueError('off must be int64[nreads + 1]')
    nreads = off.shape[0] - 1
    if nreads and (off[0] < 0 or bool(np.any(np.diff(off) < 0))):
        raise ValueError('off must start at or above 0 and never decrease')
    nev = int(off[-1]) if nreads else 0
    if val.ndim != 1 or val.shape[0] < nev:
        raise ValueError('val is shorter than its offsets say')
    if model is None:
        raise ValueError('read_calls needs a k-mer model')
    k, center = int(model['k']), int(model['center'])
    opts, want = _calls_opts(nb, alpha, k, center, want)
    mean = np.ascontiguousarray(model['mean'], dtype=np.float64)
    sd = np.ascontiguousarray(model['sd'], dtype=np.float64)
    if mean.shape != (4 ** k,) or sd.shape != (4 ** k,):
        raise ValueError('model mean / sd must be float64[4^k]')
    base = np.asarray(base)
    base = np.ascontiguousarray(base if base.dtype == np.uint8 else base.astype('S1').view(np.uint8))
    if base.ndim != 1 or base.shape[0] < nev:
        raise ValueError('base is shorter than its offsets say')
    m = L.NmodRescaleModel()
    m.k, m.center, m.mean, m.sd = k, center, mean.ctypes.data, sd.ctypes.data
    res = {w: np.full(val.shape[0], np.nan) for w in want}
    res.update(n_sites=np.zeros(nreads, np.int32), n_called=np.zeros(nreads, np.int32), status=np.zeros(nreads, np.uint8))
    _join_warm_up(device)
    out = L.make_calls_out(**{name: _np_ptr(a) for name, a in res.items()})
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=_dtype_code(val.dtype))
    rc = lib.nmod_read_calls(C.byref(prm), nreads, _np_ptr(off), _np_ptr(val), _np_ptr(base), C.byref(m), C.byref(opts), C.byref(out))
    L.check(rc, 'nmod_read_calls')
    if nreads and off[0] > 0:
        for w in want:                                          # events before the first read belong to no read
            res[w][:off[0]] = np.nan
    return res


def site_calls_host(score, off, *, stride=0, alpha=0.01, device=0):
    """Per-position call counts over pivoted scores (nmod_site_calls): score float64, one row per position by `off` (int64[npos + 1])
    or, with off None, a fixed `stride`.  Returns a dict of numpy arrays: n_valid (scores in [0, 1]), n_called (valid scores <= alpha),
    both int32, and frac = n_called / n_valid (float64, NaN without a valid score)."""
    lib = L.load()
    score = np.ascontiguousarray(score, dtype=np.float64)
    alpha = float(alpha)
    if not 0.0 < alpha <= 1.0:
        raise ValueError('alpha must be in (0, 1]')
    if score.ndim != 1:
        raise ValueError('score must be a float64 vector')
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64)
        if off.ndim != 1 or off.shape[0] < 1:
            raise ValueError('off must be int64[npos + 1]')
        npos = off.shape[0] - 1
        if npos and (off[0] < 0 or bool(np.any(np.diff(off) < 0))):
            raise ValueError('off must start at or above 0 and never decrease')
        if score.shape[0] < (int(off[-1]) if npos else 0):
            raise ValueError('score is shorter than its offsets say')
    else:
        stride = int(stride)
        if stride <= 0:
            raise ValueError('either off or a positive stride')
        if score.shape[0] % stride:
            raise ValueError('score must hold whole rows of the stride')
        npos = score.shape[0] // stride
    res = dict(n_valid=np.zeros(npos, np.int32), n_called=np.zeros(npos, np.int32), frac=np.full(npos, np.nan))
    _join_warm_up(device)
    out = L.make_site_out(**{name: _np_ptr(a) for name, a in res.items()})
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64, stride0=stride if off is None else 0)
    rc = lib.nmod_site_calls(C.byref(prm), npos, _np_ptr(score), _np_ptr(off), alpha, C.byref(out))
    L.check(rc, 'nmod_site_calls')
    return res


def region_rank_host(strand_lo, strand_hi, pos, base, value, w, movesize, na, percentile, wind_ovlp, device=0):
    """myDetect.py:463-515 on array-shaped records (see nmod_region_rank): indices of the ranked window centres."""
    lib = L.load()
    n = len(pos)
    lo = np.ascontiguousarray(strand_lo, dtype=np.int32); hi = np.ascontiguousarray(strand_hi, dtype=np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.int64); value = np.ascontiguousarray(value, dtype=np.float64)
    base = bytes(base)
    assert len(base) == n
    out = np.empty(n, dtype=np.int32)
    cnt = C.c_int64(0)
    prm = L.make_params(device=device, memspace=L.MEM_HOST)
    rc = lib.nmod_region_rank(C.byref(prm), n, _np_ptr(lo), _np_ptr(hi), _np_ptr(pos), base, _np_ptr(value), int(w), int(movesize),
                              (na or '\0').encode()[:1], float(percentile), int(wind_ovlp), _np_ptr(out), C.byref(cnt))
    L.check(rc, 'nmod_region_rank')
    return out[:cnt.value]


def _first_chars(a):
    """the first character of every element (a blank for an empty one) as one bytes object, without a Python loop"""
    u = np.asarray(a)
    if u.dtype.kind != 'U':
        u = u.astype('U1') if u.dtype.kind in 'SO' or u.size == 0 else np.array([str(x) for x in u.tolist()], dtype='U1')
    elif u.dtype.itemsize != 4:
        u = u.astype('U1')
    codes = np.ascontiguousarray(u).view(np.uint32)
    if codes.size and int(codes.max()) > 127:                      # non-ASCII: the slow, general way
        return ''.join(str(x)[:1] or ' ' for x in np.asarray(a).tolist()).encode()
    c = codes.astype(np.uint8)
    c[c == 0] = 32
    return c.tobytes()


def write_sign_test_host(path, meta, res, with_comb):
    """save_test's table (myDetect.py:522-538) through nmod_write_sign_test.  meta: arrays chrom_id (int32), pos
    (int64, 0-based), strand / base (one character each), n0 / n1 (int32) + the list `names` that chrom_id indexes."""
    lib = L.load()
    npos = len(meta['pos'])
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    cid = np.ascontiguousarray(meta['chrom_id'], dtype=np.int32)
    names = b''.join(str(n).encode() + b'\0' for n in meta['names'])
    strand = _first_chars(meta['strand'])
    base = _first_chars(meta['base'])
    pos = np.ascontiguousarray(meta['pos'], dtype=np.int64)
    n0 = np.ascontiguousarray(meta['n0'], dtype=np.int32); n1 = np.ascontiguousarray(meta['n1'], dtype=np.int32)
    cols = [np.ascontiguousarray(res[k], dtype=np.float64) for k in ('mwu_u', 'mwu_p', 't_t', 't_p', 'ks_d', 'ks_p')]
    comb = [np.ascontiguousarray(res[k], dtype=np.float64) for k in ('comb_st', 'comb_p')] if with_comb else [None, None]
    rc = lib.nmod_write_sign_test(str(path).encode(), npos, p(cid), names, len(meta['names']), strand, p(pos), base,
                                  p(n0), p(n1), *[p(c) for c in cols],
                                  *(p(c) if c is not None else None for c in comb), 1 if with_comb else 0)
    L.check(rc, 'nmod_write_sign_test')


class EventTimer:
    """HIP-event timer handle (nmod_evtimer_*): per-kernel elapsed ms measured on the launch stream."""

    def __init__(self, capacity=4096):
        self._lib = L.load()
        self._h = C.c_void_p()
        L.check(self._lib.nmod_evtimer_create(capacity, C.byref(self._h)), 'nmod_evtimer_create')

    @property
    def handle(self):
        return self._h

    def reset(self):
        L.check(self._lib.nmod_evtimer_reset(self._h), 'nmod_evtimer_reset')

    def read(self, kernel):
        ms = C.c_double()
        n = C.c_int32()
        L.check(self._lib.nmod_evtimer_read(self._h, kernel, C.byref(ms), C.byref(n)), 'nmod_evtimer_read')
        return ms.value, n.value

    def close(self):
        if self._h:
            self._lib.nmod_evtimer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceDetector:
    """Device-resident form: inputs and outputs are torch CUDA tensors; nothing is copied
    and nothing synchronises unless max_n0/max_n1 are unknown for CSR inputs or allow groups beyond MAX_GROUP
    (one round trip sizes the scratch of the large-position pass)."""

    def __init__(self, device=0, nb=2, weights_dif=2.0, method='stouffer', tests=L.TEST_ALL, want_mstd=False, flags=0, deep=False):
        import torch
        self.torch = torch
        self.lib = L.load()
        self.device = device
        self.nb = nb
        self.weights_dif = weights_dif
        self.method = L.METHOD_BY_NAME[method] if isinstance(method, str) else method
        self.tests = tests
        self.want_mstd = bool(want_mstd)
        self.flags = int(flags) | (L.FLAG_DEEP if deep else 0)          # L.FLAG_* (include/nanomod_hip.h: NMOD_FLAG_*); deep: FLAG_DEEP
        self._ws = None
        self.timer = None

    def _params(self, dtype, stride0, stride1, max_n0, max_n1):
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        return L.make_params(device=self.device, stream=stream, memspace=L.MEM_DEVICE, dtype=dtype,
                             tests=self.tests, method=self.method, nb=self.nb, weights_dif=self.weights_dif,
                             want_mstd=int(self.want_mstd), stride0=stride0, stride1=stride1,
                             max_n0=max_n0, max_n1=max_n1,
                             timer=self.timer.handle if self.timer is not None else None, flags=self.flags)

    def _dtype_of(self, t):
        torch = self.torch
        if t.dtype == torch.float32:
            return L.DTYPE_F32
        if t.dtype == torch.int16:
            return L.DTYPE_I16_MILLI
        if t.dtype == torch.float64:
            return L.DTYPE_F64
        raise ValueError('signals must be float32, int16 (milli-units) or float64')

    def workspace(self, prm, npos):
        need = self.lib.nmod_workspace_bytes(C.byref(prm), npos)
        if self._ws is None or self._ws.numel() < need:
            self._ws = self.torch.empty(need, dtype=self.torch.uint8, device='cuda:%d' % self.device)
        return self._ws, need

    def alloc_outputs(self, npos):
        torch = self.torch
        dev = 'cuda:%d' % self.device
        names = []
        if self.tests & L.TEST_MWU:
            names += ['mwu_u', 'mwu_p']
        if self.tests & L.TEST_WELCH:
            names += ['t_t', 't_p']
        if (self.tests & L.TEST_KS) or self.method != L.METHOD_KS:
            names += ['ks_d', 'ks_p']
        if self.method != L.METHOD_KS:
            names += ['comb_st', 'comb_p']
        if self.want_mstd:
            names += ['mean0', 'std0', 'mean1', 'std1']
        res = {n: torch.empty(npos, dtype=torch.float64, device=dev) for n in names}
        res['status'] = torch.empty(npos, dtype=torch.uint8, device=dev)
        return res

    def dispatch_stats(self):
        """which K1 form computed the positions of the last run() (nmod_last_dispatch_stats; synchronises the stream)"""
        return L.last_dispatch_stats()

    def run(self, sig0, sig1, run_id, *, off0=None, off1=None, stride0=0, stride1=0, npos=None,
            max_n0=0, max_n1=0, out=None):
        """Enqueue the hot path on the current stream.  Either CSR offsets (int64 CUDA tensors)
        or fixed strides describe the rows.  Returns the dict of output tensors."""
        dtype = self._dtype_of(sig0)
        if self._dtype_of(sig1) != dtype:
            raise ValueError('sig0 and sig1 must share a dtype')
        if npos is None:
            npos = (off0.numel() - 1) if off0 is not None else sig0.numel() // stride0
        prm = self._params(dtype, stride0 if off0 is None else 0, stride1 if off1 is None else 0, max_n0, max_n1)
        ws, need = self.workspace(prm, npos)
        res = out if out is not None else self.alloc_outputs(npos)
        o = L.NmodOut()
        for name in L.OUT_FIELDS:
            if name in res:
                setattr(o, name, res[name].data_ptr())
        o.status = res['status'].data_ptr()
        ptr = lambda t: (t.data_ptr() if t is not None else None)
        rc = self.lib.nmod_detect_batch(C.byref(prm), npos, ptr(sig0), ptr(off0), ptr(sig1), ptr(off1),
                                        ptr(run_id), ws.data_ptr(), need, C.byref(o))
        L.check(rc, 'nmod_detect_batch')
        return res

    def fdr(self, res, tracks=('comb_p',), method='bh', alpha=0.05, out=None):
        """q-values of p-value tracks of a run() result (or of any dict of float64 CUDA tensors of one length), enqueued on the
        current stream without synchronising (nmod_fdr_adjust, NMOD_MEM_DEVICE).  Returns (list of q tensors in `tracks` order, a
        float64 CUDA tensor of ntracks x 4 words holding each track's nmod_fdr_summary: tested, excluded, rejected as int64 bit
        images and p_crit; engine.fdr_summary_dicts reads it).  A track that `res` lacks raises KeyError.  out: a dict of
        tensors to write q into (a track's own tensor for in place)."""
        torch = self.torch
        ps = [res[name] for name in tracks]                         # KeyError for a track the run did not produce
        for t in ps:
            if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 1 and t.numel() == ps[0].numel()):
                raise ValueError('fdr: tracks must be contiguous float64 CUDA vectors of one length')
        n = ps[0].numel() if ps else 0
        dev = 'cuda:%d' % self.device
        qs = [out[name] if out is not None else torch.empty(n, dtype=torch.float64, device=dev) for name in tracks]
        nt = len(ps)
        summary = torch.empty((max(nt, 1), 4), dtype=torch.float64, device=dev)
        parr = (C.c_void_p * max(nt, 1))(*[t.data_ptr() for t in ps])
        qarr = (C.c_void_p * max(nt, 1))(*[t.data_ptr() for t in qs])
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        rc = self.lib.nmod_fdr_adjust(C.byref(prm), n, nt, parr, _fdr_method(method), float(alpha), qarr, summary.data_ptr())
        L.check(rc, 'nmod_fdr_adjust')
        return qs, summary

    def mix(self, sig0, sig1, *, off0=None, off1=None, stride0=0, stride1=0, npos=None, mix_group=1, model='equal', max_iter=200,
            tol=1e-6, gate=None, gate_max=0.05, want_resp=False, out=None):
        """Per-position modified fraction (nmod_mix_fraction, NMOD_MEM_DEVICE) of rows described as in run(), enqueued on the
        current stream without synchronising.  gate: a float64 CUDA track, position i is computed iff gate[i] <= gate_max.  Returns
        a dict of CUDA tensors: pi, mu_mod, sd_mod, llr (float64), iters (int32), status (uint8, L.MIX_* bits), and with want_resp
        `resp` (float32, one posterior per read of the mixed group, in its layout).  llr is a score: it has no p-value.

        Tests, q-values and fractions of the rejected positions as one stream, nothing read on the host in between:

            res = det.run(sig0, sig1, run_id, stride0=n, stride1=n, npos=npos)
            (q,), summary = det.fdr(res, tracks=('comb_p',), method='bh', alpha=0.05)
            mix = det.mix(sig0, sig1, stride0=n, stride1=n, npos=npos, gate=q, gate_max=0.05)
        """
        torch = self.torch
        mix_group, model, max_iter, tol = _mix_args(mix_group, model, max_iter, tol)
        dtype = self._dtype_of(sig0)
        if self._dtype_of(sig1) != dtype:
            raise ValueError('sig0 and sig1 must share a dtype')
        if npos is None:
            npos = (off0.numel() - 1) if off0 is not None else ((off1.numel() - 1) if off1 is not None else sig0.numel() // stride0)
        dev = 'cuda:%d' % self.device
        if gate is not None and not (gate.is_cuda and gate.dtype == torch.float64 and gate.is_contiguous() and gate.numel() == npos):
            raise ValueError('mix: gate must be a contiguous float64 CUDA vector of npos elements')
        res = out
        if res is None:
            res = {k: torch.empty(npos, dtype=torch.float64, device=dev) for k in L.MIX_FIELDS}
            res['iters'] = torch.empty(npos, dtype=torch.int32, device=dev)
            res['status'] = torch.empty(npos, dtype=torch.uint8, device=dev)
            if want_resp:
                res['resp'] = torch.empty((sig1 if mix_group == 1 else sig0).numel(), dtype=torch.float32, device=dev)
        o = L.NmodMixOut()
        for k, t in res.items():
            setattr(o, k, t.data_ptr())
        prm = self._params(dtype, stride0 if off0 is None else 0, stride1 if off1 is None else 0, 0, 0)
        ptr = lambda t: (t.data_ptr() if t is not None else None)
        rc = self.lib.nmod_mix_fraction(C.byref(prm), npos, ptr(sig0), ptr(off0), ptr(sig1), ptr(off1), mix_group, model, max_iter,
                                        tol, ptr(gate), float(gate_max), C.byref(o))
        L.check(rc, 'nmod_mix_fraction')
        return res

    def one_sample(self, sig, ref_mean, ref_sd, ref_n=None, run_id=None, *, off=None, stride=0, npos=None, out=None):
        """One read group against a stored per-position reference (nmod_one_sample, NMOD_MEM_DEVICE) under the detector's nb /
        method / weights_dif, enqueued on the current stream without synchronising.  sig: float32, int16 or float64 CUDA rows by
        `off` (int64 CUDA tensor) or a fixed `stride`; ref_mean / ref_sd: float64 CUDA vectors; ref_n: int32 (a stored control) or
        None (a model); run_id: int32, required unless the method is 'ks'.  Returns a dict of CUDA tensors: ks_d, ks_p, t_t, t_p,
        shift, mean, std (float64), status (uint8) and, unless the method is 'ks', comb_st / comb_p — which fdr() accepts:

            res = det.one_sample(sig, mu, sd, n_ref, run_id, stride=n)
            qs, summary = det.fdr(res, tracks=('ks_p', 't_p', 'comb_p'))
        """
        torch = self.torch
        dtype = self._dtype_of(sig)
        if npos is None:
            npos = ref_mean.numel()
        dev = 'cuda:%d' % self.device
        for t, dt, name in ((ref_mean, torch.float64, 'ref_mean'), (ref_sd, torch.float64, 'ref_sd'), (ref_n, torch.int32, 'ref_n'),
                            (run_id, torch.int32, 'run_id'), (off, torch.int64, 'off')):
            if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == npos + (name == 'off')):
                raise ValueError('one_sample: %s must be a contiguous %s CUDA vector of npos%s elements' % (name, dt, ' + 1' if name == 'off' else ''))
        if self.method != L.METHOD_KS and run_id is None:
            raise ValueError('one_sample: run_id is needed for the combined track')
        res = out
        if res is None:
            names = [k for k in L.ONE_FIELDS if self.method != L.METHOD_KS or not k.startswith('comb_')]
            res = {k: torch.empty(npos, dtype=torch.float64, device=dev) for k in names}
            res['status'] = torch.empty(npos, dtype=torch.uint8, device=dev)
        o = L.make_one_out(**{k: t.data_ptr() for k, t in res.items()})
        prm = self._params(dtype, stride if off is None else 0, 0, 0, 0)
        ptr = lambda t: (t.data_ptr() if t is not None else None)
        rc = self.lib.nmod_one_sample(C.byref(prm), npos, ptr(sig), ptr(off), ptr(ref_mean), ptr(ref_sd), ptr(ref_n), ptr(run_id), C.byref(o))
        L.check(rc, 'nmod_one_sample')
        return res

    def kmer_model(self, sig, code, ncodes, keep_lo=None, keep_hi=None, *, off=None, stride=0, npos=None, out=None):
        """Per-code level models (nmod_kmer_model, NMOD_MEM_DEVICE), enqueued on the current stream without synchronising.  sig:
        float32, int16 or float64 CUDA rows by `off` (int64 CUDA tensor) or a fixed `stride`; code: int32 CUDA vector (a value outside
        [0, ncodes): the position takes no part, L.STATUS_NO_CODE); keep_lo / keep_hi: float64 CUDA vectors of ncodes inclusive bounds,
        or both None.  Returns a dict of CUDA tensors: n_positions, n_samples, n_clipped (int64), mean, sd (float64), each of ncodes,
        and pos_status (uint8, npos).  int16 is the streaming form; the float dtypes are not tuned."""
        torch = self.torch
        dtype = self._dtype_of(sig)
        if npos is None:
            npos = code.numel()
        ncodes = int(ncodes)
        dev = 'cuda:%d' % self.device
        for t, dt, name, m in ((code, torch.int32, 'code', npos), (off, torch.int64, 'off', npos + 1),
                               (keep_lo, torch.float64, 'keep_lo', ncodes), (keep_hi, torch.float64, 'keep_hi', ncodes)):
            if t is not None and not (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == m):
                raise ValueError('kmer_model: %s must be a contiguous %s CUDA vector of %d elements' % (name, dt, m))
        res = out
        if res is None:
            res = {k: torch.empty(max(ncodes, 0), dtype=torch.int64, device=dev) for k in L.KMER_COUNT_FIELDS}
            res['mean'] = torch.empty(max(ncodes, 0), dtype=torch.float64, device=dev)
            res['sd'] = torch.empty(max(ncodes, 0), dtype=torch.float64, device=dev)
            res['pos_status'] = torch.empty(npos, dtype=torch.uint8, device=dev)
        o = L.make_kmer_out(**{k: t.data_ptr() for k, t in res.items()})
        prm = self._params(dtype, stride if off is None else 0, 0, 0, 0)
        ptr = lambda t: (t.data_ptr() if t is not None else None)
        rc = self.lib.nmod_kmer_model(C.byref(prm), npos, ptr(sig), ptr(off), ptr(code), ncodes, ptr(keep_lo), ptr(keep_hi), C.byref(o))
        L.check(rc, 'nmod_kmer_model')
        return res

    def rescale_reads(self, val, off, base, mean=None, sd=None, k=None, center=None, *, mode='fit_apply', weighted=True, clip_sigma=3.0,
                      clip_rounds=2, min_events=50, scale_range=(0.5, 2.0), shift=None, scale=None, inplace=False, out=None):
        """Per-read shift and scale against a k-mer model and the rescaled events (nmod_rescale_reads, NMOD_MEM_DEVICE), enqueued on
        the current stream without synchronising or reading anything back.  val: float32, int16 or float64 CUDA vector of events,
        base: uint8 CUDA vector (one byte per event), off: int64 CUDA vector of nreads + 1 event offsets; mean / sd: float64 CUDA
        vectors of 4^k model entries.  mode 'apply_only' takes shift / scale (float64 CUDA vectors) instead of the model.  inplace:
        the rescaled events overwrite val.  Returns a dict of CUDA tensors: shift, scale, n_used (int32), status (uint8) and, unless
        mode is 'fit_only', val — which pivot_reads' device form takes on the same stream.  out: such a dict from an earlier call of
        the same shape and mode, written again instead of allocating (a timing loop)."""
        torch = self.torch
        dtype = self._dtype_of(val)
        opts = _rescale_opts(mode, weighted, clip_sigma, clip_rounds, min_events, scale_range, k, center)
        fit, apply = opts.mode != L.RESCALE_APPLY_ONLY, opts.mode != L.RESCALE_FIT_ONLY
        dev = 'cuda:%d' % self.device
        if not (off.is_cuda and off.dtype == torch.int64 and off.is_contiguous() and off.numel() >= 1):
            raise ValueError('rescale_reads: off must be a contiguous int64 CUDA vector of nreads + 1 elements')
        nreads = off.numel() - 1
        checks = [(val, None, 'val', None)]
        if fit:
            checks += [(base, torch.uint8, 'base', None), (mean, torch.float64, 'mean', 4 ** int(k)), (sd, torch.float64, 'sd', 4 ** int(k))]
        else:
            checks += [(shift, torch.float64, 'shift', nreads), (scale, torch.float64, 'scale', nreads)]
        for t, dt, name, m in checks:
            if t is None or not (t.is_cuda and t.is_contiguous() and (dt is None or t.dtype == dt) and (m is None or t.numel() == m)):
                raise ValueError('rescale_reads: %s must be a contiguous CUDA vector%s' % (name, '' if m is None else ' of %d elements' % m))
        if fit and base.numel() != val.numel():
            raise ValueError('rescale_reads: base needs one byte per event')
        res = out
        if res is not None:
            want = dict(shift=(torch.float64, nreads), scale=(torch.float64, nreads), n_used=(torch.int32, nreads), status=(torch.uint8, nreads))
            if apply:
                want['val'] = (val.dtype, val.numel())
            for name, (dt, m) in want.items():
                t = res.get(name)
                if t is None or not (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() == m):
                    raise ValueError('rescale_reads: out[%r] must be a contiguous %s CUDA vector of %d elements' % (name, dt, m))
        else:
            res = dict(n_used=torch.zeros(nreads, dtype=torch.int32, device=dev), status=torch.zeros(nreads, dtype=torch.uint8, device=dev))
            if fit:
                res['shift'] = torch.empty(nreads, dtype=torch.float64, device=dev)
                res['scale'] = torch.empty(nreads, dtype=torch.float64, device=dev)
            else:
                res['shift'], res['scale'] = shift, scale
            if apply:
                res['val'] = val if inplace else torch.empty_like(val)
        m = L.NmodRescaleModel()
        if fit:
            m.k, m.center, m.mean, m.sd = int(k), int(center), mean.data_ptr(), sd.data_ptr()
        o = L.make_rescale_out(shift=res['shift'].data_ptr(), scale=res['scale'].data_ptr(), n_used=res['n_used'].data_ptr(),
                               status=res['status'].data_ptr(), val_out=res['val'].data_ptr() if apply else None)
        prm = self._params(dtype, 0, 0, 0, 0)
        rc = self.lib.nmod_rescale_reads(C.byref(prm), nreads, off.data_ptr(), val.data_ptr(), base.data_ptr() if fit else None,
                                         C.byref(m), C.byref(opts), C.byref(o))
        L.check(rc, 'nmod_rescale_reads')
        return res

    def read_calls(self, val, off, base, mean, sd, k, center, *, nb=2, alpha=0.01, want=('z', 'p', 'p_win'), out=None):
        """Per-read modification calls against a k-mer model (nmod_read_calls, NMOD_MEM_DEVICE), enqueued on the current stream without
        synchronising or reading anything back.  val: float32, int16 or float64 CUDA vector of events (the `val` of rescale_reads, say),
        base: uint8 CUDA vector (one byte per event), off: int64 CUDA vector of nreads + 1 event offsets; mean / sd: float64 CUDA
        vectors of 4^k model entries.  Returns a dict of CUDA tensors: the per-event tracks named in `want` (float64: z, p, p_win) and per
        read n_sites, n_called (int32) and status (uint8).  p_win is what pivot_reads' device form takes as `val` for site_calls.
        out: such a dict from an earlier call of the same shape, written again instead of allocating (a timing loop)."""
        torch = self.torch
        dtype = self._dtype_of(val)
        opts, want = _calls_opts(nb, alpha, k, center, want)
        dev = 'cuda:%d' % self.device
        if not (off.is_cuda and off.dtype == torch.int64 and off.is_contiguous() and off.numel() >= 1):
            raise ValueError('read_calls: off must be a contiguous int64 CUDA vector of nreads + 1 elements')
        nreads = off.numel() - 1
        for t, dt, name, m in ((val, None, 'val', None), (base, torch.uint8, 'base', None), (mean, torch.float64, 'mean', 4 ** int(k)),
                               (sd, torch.float64, 'sd', 4 ** int(k))):
            if t is None or not (t.is_cuda and t.is_contiguous() and t.dim() == 1 and (dt is None or t.dtype == dt) and (m is None or t.numel() == m)):
                raise ValueError('read_calls: %s must be a contiguous CUDA vector%s' % (name, '' if m is None else ' of %d elements' % m))
        if base.numel() != val.numel():
            raise ValueError('read_calls: base needs one byte per event')
        shapes = {w: (torch.float64, val.numel()) for w in want}
        shapes.update(n_sites=(torch.int32, nreads), n_called=(torch.int32, nreads), status=(torch.uint8, nreads))
        res = out
        if res is not None:
            for name, (dt, m) in shapes.items():
                t = res.get(name)
                if t is None or not (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() == m):
                    raise ValueError('read_calls: out[%r] must be a contiguous %s CUDA vector of %d elements' % (name, dt, m))
        else:
            res = {name: torch.empty(m, dtype=dt, device=dev) for name, (dt, m) in shapes.items()}
        md = L.NmodRescaleModel()
        md.k, md.center, md.mean, md.sd = int(k), int(center), mean.data_ptr(), sd.data_ptr()
        o = L.make_calls_out(**{name: res[name].data_ptr() for name in shapes})
        prm = self._params(dtype, 0, 0, 0, 0)
        rc = self.lib.nmod_read_calls(C.byref(prm), nreads, off.data_ptr(), val.data_ptr(), base.data_ptr(), C.byref(md), C.byref(opts), C.byref(o))
        L.check(rc, 'nmod_read_calls')
        return res

    def site_calls(self, score, *, off=None, stride=0, npos=None, alpha=0.01, out=None):
        """Per-position call counts over pivoted scores (nmod_site_calls, NMOD_MEM_DEVICE) on the current stream: score a float64 CUDA
        vector, rows by `off` (int64 CUDA vector) or a fixed `stride`.  Returns a dict of CUDA tensors n_valid, n_called (int32) and
        frac (float64)."""
        torch = self.torch
        alpha = float(alpha)
        if not 0.0 < alpha <= 1.0:
            raise ValueError('alpha must be in (0, 1]')
        if not (score.is_cuda and score.dtype == torch.float64 and score.is_contiguous() and score.dim() == 1):
            raise ValueError('site_calls: score must be a contiguous float64 CUDA vector')
        if off is not None:
            if not (off.is_cuda and off.dtype == torch.int64 and off.is_contiguous() and off.numel() >= 1):
                raise ValueError('site_calls: off must be a contiguous int64 CUDA vector of npos + 1 elements')
            npos = off.numel() - 1
        else:
            stride = int(stride)
            if stride <= 0:
                raise ValueError('site_calls: either off or a positive stride')
            if npos is None:
                npos = score.numel() // stride
            if npos * stride > score.numel():
                raise ValueError('site_calls: score is shorter than npos rows of the stride')
        dev = 'cuda:%d' % self.device
        shapes = dict(n_valid=torch.int32, n_called=torch.int32, frac=torch.float64)
        res = out
        if res is not None:
            for name, dt in shapes.items():
                t = res.get(name)
                if t is None or not (t.is_cuda and t.is_contiguous() and t.dtype == dt and t.numel() == npos):
                    raise ValueError('site_calls: out[%r] must be a contiguous %s CUDA vector of %d elements' % (name, dt, npos))
        else:
            res = {name: torch.empty(npos, dtype=dt, device=dev) for name, dt in shapes.items()}
        o = L.make_site_out(**{name: res[name].data_ptr() for name in shapes})
        prm = self._params(L.DTYPE_F64, stride if off is None else 0, 0, 0, 0)
        rc = self.lib.nmod_site_calls(C.byref(prm), npos, score.data_ptr(), off.data_ptr() if off is not None else None, alpha, C.byref(o))
        L.check(rc, 'nmod_site_calls')
        return res

    def synth_fill(self, out, seed, pos_begin, npos, group, n_per_pos, plant_period=0, plant_shift=0.0):
        prm = self._params(self._dtype_of(out), 0, 0, 0, 0)
        rc = self.lib.nmod_synth_fill(C.byref(prm), seed, pos_begin, npos, group, n_per_pos,
                                      plant_period, plant_shift, out.data_ptr())
        L.check(rc, 'nmod_synth_fill')
        return out


    def synth_fill_csr(self, out, seed, pos_begin, off, group, plant_period=0, plant_shift=0.0):
        """ragged rows: `off` = int64 CUDA tensor of npos + 1 element offsets into `out`"""
        prm = self._params(self._dtype_of(out), 0, 0, 0, 0)
        rc = self.lib.nmod_synth_fill_csr(C.byref(prm), seed, pos_begin, off.numel() - 1, group, off.data_ptr(),
                                          plant_period, plant_shift, out.data_ptr())
        L.check(rc, 'nmod_synth_fill_csr')
        return out

    def synth_fill_events(self, out, seed, pos_begin, npos, group, n_per_pos=0, off=None, plant_period=0, plant_shift_milli=0,
                          spread_milli=200, outlier_permille=0):
        """event-like rows (nmod_synth_fill_events): a level per position, reads spread `spread_milli` around it, on the
        3-decimal grid; fixed stride (n_per_pos > 0) or ragged (`off` = int64 CUDA tensor of npos + 1 offsets); `outlier_permille`
        of 1 000 reads are replaced by a uniform draw over +-5 units (mis-segmented events)"""
        prm = self._params(self._dtype_of(out), 0, 0, 0, 0)
        rc = self.lib.nmod_synth_fill_events(C.byref(prm), seed, pos_begin, npos, group, n_per_pos,
                                             off.data_ptr() if off is not None else None, plant_period,
                                             int(plant_shift_milli), int(spread_milli), int(outlier_permille), out.data_ptr())
        L.check(rc, 'nmod_synth_fill_events')
        return out


def downsample_ks(sig0, off0, sig1, off1, positions, cov, *, iters=100, quantile=0.25, seed=0, device=0, deep=False):
    """The down-sampling branch of getKStest (myDetect.py:345-361) for the positions `positions` (indices into
    the CSR arrays) through nmod_downsample_ks: `iters` times, a group with more than cov[i] samples is resampled WITH
    replacement to cov[i] samples (np.random.choice semantics), KS is run on each resample, and the (D, p) pair at index
    int(iters * quantile) of the p-sorted resamples is reported.  The reference draws from an unseeded
    global RNG, so its numbers are not reproducible; here the draws come from a seeded counter-based device generator —
    statistically equivalent, not bit-comparable (SURVEY.md §8a row A3', §8f row 4).  The resampled rows are
    materialised chunk by chunk in HBM and go through the same KS kernel as everything else; resampling, KS and the
    quantile selection all run in the library (round 3 assembled the rows with torch indexing).
    deep: L.FLAG_DEEP, for groups and thresholds beyond L.MAX_RANKED (up to L.MAX_DEEP); without it such a group is an error.
    Returns (ks_d, ks_p) numpy arrays aligned with `positions`."""
    lib = L.load()
    _join_warm_up(device)
    sig0 = np.ascontiguousarray(sig0); sig1 = np.ascontiguousarray(sig1)
    if sig0.dtype != sig1.dtype or sig0.dtype not in (np.float32, np.int16, np.float64):
        raise ValueError('sig0/sig1 must both be float32, both int16 (milli-units) or both float64')
    dtype = {np.dtype(np.float32): L.DTYPE_F32, np.dtype(np.int16): L.DTYPE_I16_MILLI, np.dtype(np.float64): L.DTYPE_F64}[sig0.dtype]
    positions = np.ascontiguousarray(positions, dtype=np.int64)
    cov = np.ascontiguousarray(cov, dtype=np.int64)
    off0 = np.ascontiguousarray(off0, dtype=np.int64); off1 = np.ascontiguousarray(off1, dtype=np.int64)
    if positions.shape != cov.shape or (len(positions) and (positions.min() < 0 or positions.max() >= len(off0) - 1)):
        raise ValueError('positions / cov must be aligned and index the CSR rows')
    out_d = np.empty(len(positions)); out_p = np.empty(len(positions))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype, tests=L.TEST_KS, method=L.METHOD_KS,
                        flags=L.FLAG_DEEP if deep else 0)
    rc = lib.nmod_downsample_ks(C.byref(prm), len(positions), _np_ptr(sig0), _np_ptr(off0), _np_ptr(sig1), _np_ptr(off1),
                                _np_ptr(positions), _np_ptr(cov), int(iters), float(quantile), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                _np_ptr(out_d), _np_ptr(out_p))
    L.check(rc, 'nmod_downsample_ks')
    return out_d, out_p


# ---------------------------------------------------------------------------------------------------- read-level input
_TORCH_OF_DTYPE = {L.DTYPE_F32: 'float32', L.DTYPE_I16_MILLI: 'int16', L.DTYPE_F64: 'float64'}


def _dtype_code(a):
    try:
        return {np.dtype(np.float32): L.DTYPE_F32, np.dtype(np.int16): L.DTYPE_I16_MILLI, np.dtype(np.float64): L.DTYPE_F64}[np.dtype(a)]
    except KeyError:
        raise ValueError('values must be float32, int16 (milli-units) or float64')


def _torch_dtype_code(t):
    import torch
    return {torch.float32: L.DTYPE_F32, torch.int16: L.DTYPE_I16_MILLI, torch.float64: L.DTYPE_F64}[t.dtype]


def chrom_names(*read_sets):
    """the sorted chromosome names over read sets: the index space of the (chrom, strand) ids both groups must share"""
    heads = [np.unique(np.asarray(r['chrom']).astype(str)) for r in read_sets]
    return [str(n) for n in np.unique(np.concatenate(heads) if heads else np.zeros(0, str)).tolist()]


class _CallTimer:
    """HIP events around one library call on the current stream; adds its device time (s) to timer[name] when timer is a dict"""

    def __init__(self, timer, name, dev):
        self.timer, self.name, self.dev = timer, name, dev

    def __enter__(self):
        if self.timer is not None:
            import torch
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        if self.timer is not None and exc[0] is None:
            import torch
            self.b.record(torch.cuda.current_stream(self.dev))
            self.b.synchronize()
            self.timer[self.name] = self.timer.get(self.name, 0.0) + self.a.elapsed_time(self.b) / 1e3
        return False


def pivot_reads(reads, device=0, pos_lo=None, pos_hi=None, names=None, timer=None, val=None):
    """nmod_pivot_reads (myDetect.py:104-124) on a read-level set (container.READ_FIELDS): returns device tensors key
    (cs << 40 | pos, ascending), off, sig (the input dtype), base (uint8) and the host list `names` the chrom ids index.
    Inside a position the samples come in read order; the base is the last read's.  pos_lo / pos_hi: the inclusive
    event-level window (myDetect.py:112-114).  timer: a dict that collects the device time (s) of the copy ('h2d') and of
    nmod_pivot_reads ('pivot'), measured with HIP events.  val: the events as a device tensor that takes the place of
    reads['norm_mean'] (the output of DeviceDetector.rescale_reads, say): it is used where it lies, on the current stream."""
    import torch
    lib = L.load()
    _join_warm_up(device)
    names = chrom_names(reads) if names is None else list(names)
    chrom = np.asarray(reads['chrom']).astype(str)
    strand = np.asarray(reads['strand']).astype(str)
    start = np.ascontiguousarray(reads['start'], dtype=np.int64)
    off = np.ascontiguousarray(reads['off'], dtype=np.int64)
    if val is None:
        val = np.ascontiguousarray(reads['norm_mean'])
        dtype = _dtype_code(val.dtype)
    else:
        if not (val.is_cuda and val.device.index == device and val.is_contiguous() and val.dim() == 1
                and val.numel() >= (int(off[-1]) if len(off) else 0)):
            raise ValueError('val must be a contiguous CUDA vector on device %d of one value per event' % device)
        dtype = _torch_dtype_code(val)
    nreads = len(start)
    if len(off) != nreads + 1 or len(chrom) != nreads or len(strand) != nreads:
        raise ValueError('reads: chrom / strand / start need one entry per read and off nreads + 1')
    if not np.all(np.isin(strand, ('+', '-'))):
        raise ValueError("reads: strand must be '+' or '-'")
    cid = np.searchsorted(np.array(names, dtype=str), chrom) if nreads else np.zeros(0, np.int64)
    if nreads and (np.any(cid >= len(names)) or np.any(np.array(names, dtype=str)[np.minimum(cid, len(names) - 1)] != chrom)):
        raise ValueError('reads: a chromosome is missing from names')
    cs = (2 * cid + (strand == '-')).astype(np.int32)
    base = np.ascontiguousarray(np.asarray(reads['base']).astype('S1')).view(np.uint8)
    lo = -1 if pos_lo is None else int(pos_lo)
    hi = -1 if pos_hi is None else int(pos_hi)
    nev = int(off[-1]) if len(off) else 0
    # row capacity: no more rows than events, nor than positions of the covered range of every (chrom, strand)
    cap = nev
    if nreads:
        n = np.diff(off)
        a = np.maximum(start, lo) if lo >= 0 else start
        b = np.minimum(start + n - 1, hi) if hi >= 0 else start + n - 1
        ok = (n > 0) & (a <= b)
        if ok.any():
            spans = 0
            for c in np.unique(cs[ok]):
                m = ok & (cs == c)
                spans += int(b[m].max()) - int(a[m].min()) + 1
            cap = min(cap, spans)
        else:
            cap = 0
    dev = torch.device('cuda', device)
    t = lambda x: torch.from_numpy(x).to(dev)
    with _CallTimer(timer, 'h2d', dev):
        d_cs, d_start, d_off, d_base = t(cs), t(start), t(off), t(base)
        d_val = val if torch.is_tensor(val) else t(val)
    key = torch.empty(max(cap, 1), dtype=torch.int64, device=dev)
    roff = torch.empty(cap + 1, dtype=torch.int64, device=dev)
    sig = torch.empty(max(nev, 1), dtype=d_val.dtype, device=dev)
    rbase = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    npos, nsamp = C.c_int64(0), C.c_int64(0)
    prm = L.make_params(device=device, memspace=L.MEM_DEVICE, dtype=dtype, stream=torch.cuda.current_stream(dev).cuda_stream)
    with _CallTimer(timer, 'pivot', dev):
        rc = lib.nmod_pivot_reads(C.byref(prm), nreads, 2 * len(names), d_cs.data_ptr(), d_start.data_ptr(), d_off.data_ptr(),
                                  d_val.data_ptr(), d_base.data_ptr(), lo, hi, cap, key.data_ptr(), roff.data_ptr(), sig.data_ptr(),
                                  rbase.data_ptr(), C.byref(npos), C.byref(nsamp))
    L.check(rc, 'nmod_pivot_reads')
    p, ns = npos.value, nsamp.value
    return dict(key=key[:p], off=roff[:p + 1], sig=sig[:ns], base=rbase[:p], names=names)


def reads_to_group(reads, device=0, pos_lo=None, pos_hi=None):
    """A read-level set (container.READ_FIELDS) as a per-position container (container.FIELDS): pivot_reads on the device and a copy
    back.  Rows come in the reference's order (sorted chromosome, '+' before '-', ascending position), the samples of a position in
    read order, the base of a position from its last read — what fast5_ingest.GroupBuilder builds from the same reads; sig keeps the
    dtype of the events."""
    g = pivot_reads(reads, device, pos_lo, pos_hi)
    key = g['key'].cpu().numpy()
    names = np.array(g['names'], dtype=str)
    chrom = names[key >> 41] if len(key) else np.zeros(0, dtype=str)
    strand = np.where((key >> 40) & 1, '-', '+').astype('U1')
    base = g['base'].cpu().numpy().view('S1').astype('U1')
    return dict(chrom=chrom, strand=strand, pos=key & ((1 << 40) - 1), base=base, off=g['off'].cpu().numpy(), sig=g['sig'].cpu().numpy())


def group_to_device(g, names, device=0):
    """a per-position container (container.FIELDS) in the layout pivot_reads returns, rows sorted by key"""
    import torch
    chrom = np.asarray(g['chrom']).astype(str)
    cid = np.searchsorted(np.array(names, dtype=str), chrom)
    key = (cid.astype(np.int64) << 41) | ((np.asarray(g['strand']) == '-').astype(np.int64) << 40) | np.asarray(g['pos'], dtype=np.int64)
    order = np.argsort(key, kind='stable')
    from . import container
    sig, off = container.gather_rows(np.asarray(g['sig']), np.asarray(g['off'], dtype=np.int64), order)
    dev = torch.device('cuda', device)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    base = np.asarray(g['base']).astype('S1').view(np.uint8)[order]
    return dict(key=t(key[order]), off=t(off), sig=t(sig), base=t(base), names=list(names))


def select_tested(g0, g1, min_coverage, device=0, out_level=3, log=print, timer=None):
    """nmod_select_tested + nmod_gather_tested on two pivoted groups (pivot_reads, same `names`): the tested rows as
    (meta, sig0, off0, sig1, off1, run_id) like cli.select_positions, the CSR arrays and run ids on the device (the inputs of
    DeviceDetector.run), meta on the host.  timer: a dict that collects the device time (s) of nmod_select_tested ('select')
    and nmod_gather_tested ('gather'), measured with HIP events."""
    import torch
    lib = L.load()
    if list(g0['names']) != list(g1['names']):
        raise ValueError('both groups must be pivoted with the same chromosome names')
    names = list(g1['names'])
    dev = torch.device('cuda', device)
    s0, s1 = g0['sig'], g1['sig']
    if s0.dtype != s1.dtype:                       # one dtype for both: the exact float64 values (int16 means k / 1000)
        f = lambda s: s.double() / 1000.0 if s.dtype == torch.int16 else s.double()
        s0, s1 = f(s0), f(s1)
    dtype = _torch_dtype_code(s0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    prm = L.make_params(device=device, memspace=L.MEM_DEVICE, dtype=dtype, stream=stream)
    n0, n1 = g0['key'].numel(), g1['key'].numel()
    cap = min(n0, n1)
    rows0 = torch.empty(max(cap, 1), dtype=torch.int64, device=dev); rows1 = torch.empty_like(rows0)
    off0 = torch.empty(cap + 1, dtype=torch.int64, device=dev); off1 = torch.empty_like(off0)
    nt, ns0, ns1, odt = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    ptr = lambda x: x.data_ptr() if x.numel() else None
    with _CallTimer(timer, 'select', dev):
        rc = lib.nmod_select_tested(C.byref(prm), int(min_coverage), n0, ptr(g0['key']), g0['off'].data_ptr(), ptr(s0), s0.numel(),
                                    n1, ptr(g1['key']), g1['off'].data_ptr(), ptr(s1), s1.numel(), cap, rows0.data_ptr(),
                                    rows1.data_ptr(), off0.data_ptr(), off1.data_ptr(), C.byref(nt), C.byref(ns0), C.byref(ns1),
                                    C.byref(odt))
    L.check(rc, 'nmod_select_tested')
    npos = nt.value
    tdt = getattr(torch, _TORCH_OF_DTYPE[odt.value])
    sig0 = torch.empty(ns0.value, dtype=tdt, device=dev); sig1 = torch.empty(ns1.value, dtype=tdt, device=dev)
    run = torch.empty(npos, dtype=torch.int32, device=dev)
    key = torch.empty(npos, dtype=torch.int64, device=dev)
    b0 = torch.empty(npos, dtype=torch.uint8, device=dev); b1 = torch.empty_like(b0)
    off0, off1 = off0[:npos + 1], off1[:npos + 1]
    with _CallTimer(timer, 'gather', dev):
        rc = lib.nmod_gather_tested(C.byref(prm), npos, rows0.data_ptr(), rows1.data_ptr(), g0['off'].data_ptr(), ptr(s0),
                                    ptr(g0['base']), g1['off'].data_ptr(), ptr(s1), ptr(g1['base']), ptr(g1['key']), odt.value,
                                    off0.data_ptr(), off1.data_ptr(), ptr(sig0), ptr(sig1), ptr(run), ptr(key), ptr(b0), ptr(b1))
    L.check(rc, 'nmod_gather_tested')
    hkey = key.cpu().numpy()
    cid = (hkey >> 41).astype(np.int64)
    chrom = np.array(names, dtype=str)[cid] if npos else np.zeros(0, dtype=str)
    strand = np.where((hkey >> 40) & 1, '-', '+').astype('U1')
    pos = hkey & ((1 << 40) - 1)
    base = b1.cpu().numpy().view('S1').astype('U1')
    base0 = b0.cpu().numpy().view('S1').astype('U1')
    if out_level <= 3:                                                                 # myDetect.py:432-434
        for i in np.nonzero(base0 != base)[0][:20]:
            log('Error not equal', (chrom[i], strand[i]), int(pos[i]), base[i], base0[i])
    h0, h1 = off0.cpu().numpy(), off1.cpu().numpy()
    meta = dict(chrom=chrom, strand=strand, pos=pos, base=base, n0=np.diff(h0).astype(np.int32), n1=np.diff(h1).astype(np.int32),
                names=names, chrom_id=cid.astype(np.int32))
    return meta, sig0, off0, sig1, off1, run
