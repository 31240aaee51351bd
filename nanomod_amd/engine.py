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


# ------------------------------------------------------------------------------------------ the shared argument layer
# What the secondary entry points (fdr, mix, one-sample, k-mer model, rescale, read calls, site calls) have in common, in their
# *_host form over numpy arrays and their DeviceDetector form over CUDA tensors: every rule lives here once, the entry points
# keep their own specifics.  The C side's counterpart is csrc/entry_common.hpp / entry_device.hpp.
_SIGNAL_DTYPES = 'float32, int16 (milli-units) or float64'


def _dtype_code(a, name='values'):
    try:
        return {np.dtype(np.float32): L.DTYPE_F32, np.dtype(np.int16): L.DTYPE_I16_MILLI, np.dtype(np.float64): L.DTYPE_F64}[np.dtype(a)]
    except KeyError:
        raise ValueError('%s must be %s' % (name, _SIGNAL_DTYPES))


def _signal(a, name):
    """a numpy signal as a contiguous array and its L.DTYPE_* code"""
    a = np.ascontiguousarray(a)
    return a, _dtype_code(a.dtype, name)


def _rows(sig, off, stride, npos, name, off_name='off'):
    """npos rows of `sig` by `off` (int64[npos + 1]) or, with off None, a fixed `stride`: the contiguous offsets (or None) and the
    stride the params take (0 beside offsets)"""
    if off is not None:
        off = np.ascontiguousarray(off, dtype=np.int64)
    _check_csr(off, npos, off_name)
    if npos and sig.shape[0] < (int(off[-1]) if off is not None else npos * stride):
        raise ValueError('%s is shorter than its offsets / stride say' % name)
    return off, (stride if off is None else 0)


def _read_layout(val, off, name, count='nreads'):
    """event vectors by `off` (int64[nreads + 1]): the contiguous offsets, nreads, and the number of events up to the last read's end"""
    off = np.ascontiguousarray(off, dtype=np.int64)
    if off.ndim != 1 or off.shape[0] < 1:
        raise ValueError('off must be int64[%s + 1]' % count)
    n = off.shape[0] - 1
    if n and (off[0] < 0 or bool(np.any(np.diff(off) < 0))):
        raise ValueError('off must start at or above 0 and never decrease')
    nev = int(off[-1]) if n else 0
    if val.ndim != 1 or val.shape[0] < nev:
        raise ValueError('%s is shorter than its offsets say' % name)
    return off, n, nev


def _side(a, dtype, n, name, count='npos', optional=True):
    """a host side vector as a contiguous `dtype` array of n elements; None stays None when it is optional"""
    if a is None and optional:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    if a.shape != (n,):
        raise ValueError('%s must be %s[%s]' % (name, np.dtype(dtype).name, count))
    return a


def _check_kmer(k, center, center_unguarded=False):
    """k in 1 .. 8 and center in 0 .. k - 1.  center_unguarded: _rescale_opts' copy of the rule converts a missing center as it is
    (TypeError); _calls_opts' copy refuses it like any other (ValueError)"""
    if k is None or not 1 <= int(k) <= 8:
        raise ValueError('k must be in 1 .. 8')
    if (center is None and not center_unguarded) or not 0 <= int(center) < int(k):
        raise ValueError('center must be in 0 .. k - 1')


def _check_alpha(alpha):
    alpha = float(alpha)
    if not 0.0 < alpha <= 1.0:
        raise ValueError('alpha must be in (0, 1]')
    return alpha


def _model_len(k):
    return 4 ** int(k)


def _model_struct(k, center, mean_ptr, sd_ptr):
    m = L.NmodRescaleModel()
    m.k, m.center, m.mean, m.sd = int(k), int(center), mean_ptr, sd_ptr
    return m


def _host_model(model):
    """a k-mer model mapping (k, center, mean, sd) as a filled nmod_rescale_model, and the arrays it points to: keep them alive"""
    k = int(model['k'])
    mean = np.ascontiguousarray(model['mean'], dtype=np.float64)
    sd = np.ascontiguousarray(model['sd'], dtype=np.float64)
    if mean.shape != (_model_len(k),) or sd.shape != (_model_len(k),):
        raise ValueError('model mean / sd must be float64[4^k]')
    return _model_struct(k, model['center'], mean.ctypes.data, sd.ctypes.data), (mean, sd)


def _host_score_rows(score, off, stride):
    """pivoted scores (float64) by `off` (int64[npos + 1]) or, with off None, whole rows of a fixed `stride`: the contiguous scores and
    offsets (or None), the stride and npos"""
    score = np.ascontiguousarray(score, dtype=np.float64)
    if score.ndim != 1:
        raise ValueError('score must be a float64 vector')
    if off is not None:
        off, npos, _ = _read_layout(score, off, 'score', 'npos')
        return score, off, stride, npos
    stride = int(stride)
    if stride <= 0:
        raise ValueError('either off or a positive stride')
    if score.shape[0] % stride:
        raise ValueError('score must hold whole rows of the stride')
    return score, None, stride, score.shape[0] // stride


def _host_base(base, nev):
    """the bases of the events (S1 or uint8) as a contiguous uint8 vector of at least nev entries"""
    base = np.asarray(base)
    base = np.ascontiguousarray(base if base.dtype == np.uint8 else base.astype('S1').view(np.uint8))
    if base.ndim != 1 or base.shape[0] < nev:
        raise ValueError('base is shorter than its offsets say')
    return base


# The outputs of an entry, name -> (kind, length): kind is a dtype name numpy and torch share (or a dtype object of the form that is
# asked).  The numpy allocation, the torch allocation and the check of a caller's `out=` dict all read these tables.
def _mix_shapes(npos, nresp=None):
    shapes = dict({k: ('float64', npos) for k in L.MIX_FIELDS}, iters=('int32', npos), status=('uint8', npos))
    if nresp is not None:
        shapes['resp'] = ('float32', nresp)
    return shapes


def _one_shapes(method_id, npos):
    return dict({k: ('float64', npos) for k in L.ONE_FIELDS if method_id != L.METHOD_KS or not k.startswith('comb_')}, status=('uint8', npos))


def _kmer_shapes(npos, ncodes):
    m = max(ncodes, 0)
    return dict({k: ('int64', m) for k in L.KMER_COUNT_FIELDS}, mean=('float64', m), sd=('float64', m), pos_status=('uint8', npos))


def _kmix_shapes(npos, ncodes, want_hist=False):
    m = max(ncodes, 0)
    shapes = dict({k: ('int64', m) for k in L.KMIX_COUNT_FIELDS}, **{k: ('float64', m) for k in L.KMIX_FIELDS})
    shapes.update(iters=('int32', m), status=('uint8', m), pos_status=('uint8', npos))
    if want_hist:
        shapes['hist'] = ('uint32' if isinstance(want_hist, bool) else want_hist, m * L.KMIX_BINS)
    return shapes


def _rescale_shapes(nreads, val_kind=None, nval=0):
    """val_kind None: mode 'fit_only', no rescaled events"""
    shapes = dict(shift=('float64', nreads), scale=('float64', nreads), n_used=('int32', nreads), status=('uint8', nreads))
    if val_kind is not None:
        shapes['val'] = (val_kind, nval)
    return shapes


def _calls_shapes(want, nval, nreads):
    return dict({w: ('float64', nval) for w in want}, n_sites=('int32', nreads), n_called=('int32', nreads), status=('uint8', nreads))


def _site_shapes(npos):
    return dict(n_valid=('int32', npos), n_called=('int32', npos), frac=('float64', npos))


def _host_outputs(shapes, fill=()):
    """numpy arrays for a table of outputs; the names in `fill` start as 0 (NaN for a float), the others uninitialised"""
    res = {}
    for name, (kind, n) in shapes.items():
        dt = np.dtype(kind)
        res[name] = np.empty(n, dt) if name not in fill else np.full(n, np.nan if dt.kind == 'f' else 0, dt)
    return res


def _call(lib, name, prm, *args):
    """one C entry on `prm`; NanomodLibraryError with the library's message unless it returns NMOD_OK"""
    L.check(getattr(lib, name)(C.byref(prm), *args), name)


def _np_ptrs(res):
    return {k: _np_ptr(a) for k, a in res.items()}


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _cuda_vecs(where, items, one_dim=False, missing=None):
    """ValueError unless every t of `items` (name, t, dtype, n) is a contiguous CUDA tensor of `dtype` (None: any) and n elements
    (None: any).  one_dim: also of one dimension — read_calls, site_calls (its scores) and fdr ask for that, the other entries take
    any contiguous shape.  missing: what a None is: 'ok' (an optional argument), 'refused' (ValueError), or by default no case of
    its own (not a tensor).  One call per group of tensors: the device entries sit in timing loops."""
    for name, t, dtype, n in items:
        if t is None and missing == 'ok':
            continue
        if (t is None and missing == 'refused') or not (t.is_cuda and t.is_contiguous() and (dtype is None or t.dtype == dtype)
                                                        and (n is None or t.numel() == n) and (not one_dim or t.dim() == 1)):
            raise ValueError('%s: %s must be a contiguous %sCUDA vector%s' % (where, name, '' if dtype is None else '%s ' % dtype,
                                                                              '' if n is None else ' of %d elements' % n))


def _device_offsets(torch, off, what, count):
    """the number of rows (reads, positions) an int64 CUDA vector of offsets describes"""
    _cuda_vecs(what, (('off', off, torch.int64, None),))
    if off.numel() < 1:
        raise ValueError('%s: off must hold %s + 1 elements' % (what, count))
    return off.numel() - 1


def _device_model(torch, what, val, base, mean, sd, k, center, one_dim):
    """the events, bases and k-mer model of a device read entry, checked, as a filled nmod_rescale_model"""
    n = _model_len(k)
    _cuda_vecs(what, (('val', val, None, None), ('base', base, torch.uint8, None), ('mean', mean, torch.float64, n), ('sd', sd, torch.float64, n)),
               one_dim, missing='refused')
    if base.numel() != val.numel():
        raise ValueError('%s: base needs one byte per event' % what)
    return _model_struct(k, center, mean.data_ptr(), sd.data_ptr())


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
    _call(lib, 'nmod_fdr_adjust', prm, n, nt, parr, _fdr_method(method), float(alpha), qarr, C.cast(summ, C.c_void_p))
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
    sig0, dtype = _signal(sig0, 'sig0')
    sig1, dtype1 = _signal(sig1, 'sig1')
    if dtype != dtype1:
        raise ValueError('sig0 and sig1 must share a dtype')
    if off0 is not None:
        npos = len(off0) - 1
    elif off1 is not None:
        npos = len(off1) - 1
    else:
        npos = sig0.shape[0] // stride0
    off0, stride0 = _rows(sig0, off0, stride0, npos, 'sig0', 'off0')
    off1, stride1 = _rows(sig1, off1, stride1, npos, 'sig1', 'off1')
    gate = _side(gate, np.float64, npos, 'gate')
    nresp = None
    if want_resp:
        yoff, ystride = (off1, stride1) if mix_group == 1 else (off0, stride0)
        nresp = (int(yoff[-1]) if yoff is not None else npos * ystride) if npos else 0
    res = _host_outputs(_mix_shapes(npos, nresp))
    out = L.make_out(L.NmodMixOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype, stride0=stride0, stride1=stride1)
    _call(lib, 'nmod_mix_fraction', prm, npos, _np_ptr(sig0), _np_ptr(off0), _np_ptr(sig1), _np_ptr(off1), mix_group, model, max_iter, tol,
          _np_ptr(gate), float(gate_max), C.byref(out))
    return res


def one_sample_host(sig, off, ref_mean, ref_sd, ref_n=None, run_id=None, *, stride=0, nb=2, weights_dif=2.0, method='stouffer', device=0):
    """One read group against a stored per-position reference (nmod_one_sample, include/nanomod_hip.h) on host-resident rows:
    sig float32, int16 (milli-units) or float64, rows by `off` (int64[npos + 1]) or a fixed `stride`; ref_mean / ref_sd float64[npos]
    (sd with ddof = 0), ref_n int32[npos] for a stored control (Welch t from the statistics) or None for a model (one-sample t).
    Returns a dict of numpy arrays: ks_d, ks_p, t_t, t_p, shift, mean, std (float64), status (uint8, L.STATUS_* bits) and, when
    method is not 'ks' (run_id is then required), comb_st / comb_p: the window combine of the KS track."""
    lib = L.load()
    _join_warm_up(device)
    sig, dtype = _signal(sig, 'sig')
    ref_mean = np.ascontiguousarray(ref_mean, dtype=np.float64)
    npos = ref_mean.shape[0]
    off, stride = _rows(sig, off, stride, npos, 'sig')
    ref_sd = _side(ref_sd, np.float64, npos, 'ref_sd', optional=False)
    ref_n = _side(ref_n, np.int32, npos, 'ref_n')
    method_id = L.METHOD_BY_NAME[method] if isinstance(method, str) else method
    run = _side(run_id, np.int32, npos, 'run_id')
    res = _host_outputs(_one_shapes(method_id, npos))
    out = L.make_out(L.NmodOneOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype, method=method_id, nb=nb, weights_dif=weights_dif, stride0=stride)
    _call(lib, 'nmod_one_sample', prm, npos, _np_ptr(sig), _np_ptr(off), _np_ptr(ref_mean), _np_ptr(ref_sd), _np_ptr(ref_n), _np_ptr(run),
          C.byref(out))
    return res


def kmer_model_host(sig, off, code, ncodes, keep_lo=None, keep_hi=None, *, stride=0, device=0):
    """Per-code level models of host-resident rows (nmod_kmer_model, include/nanomod_hip.h): sig float32, int16 (milli-units) or
    float64, rows by `off` (int64[npos + 1]) or a fixed `stride`; code int32[npos] in [-1, ncodes) (-1: the position takes no part);
    keep_lo / keep_hi float64[ncodes] (inclusive bounds of the kept samples per code) or both None.  Returns a dict of numpy arrays:
    n_positions, n_samples, n_clipped (int64[ncodes]), mean, sd (float64[ncodes], NaN for a code without kept samples) and
    pos_status (uint8[npos], L.STATUS_* bits of the positions dropped whole)."""
    lib = L.load()
    _join_warm_up(device)
    sig, dtype = _signal(sig, 'sig')
    code = np.ascontiguousarray(code, dtype=np.int32)
    npos = code.shape[0]
    off, stride = _rows(sig, off, stride, npos, 'sig')
    if code.ndim != 1:
        raise ValueError('code must be int32[npos]')
    ncodes = int(ncodes)
    if (keep_lo is None) != (keep_hi is None):
        raise ValueError('keep_lo and keep_hi come together')
    keep_lo = _side(keep_lo, np.float64, ncodes, 'keep_lo', 'ncodes')
    keep_hi = _side(keep_hi, np.float64, ncodes, 'keep_hi', 'ncodes')
    res = _host_outputs(_kmer_shapes(npos, ncodes))
    out = L.make_out(L.NmodKmerOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype, stride0=stride)
    _call(lib, 'nmod_kmer_model', prm, npos, _np_ptr(sig), _np_ptr(off), _np_ptr(code), ncodes, _np_ptr(keep_lo), _np_ptr(keep_hi), C.byref(out))
    return res


def _kmix_opts(model, max_iter, tol, min_samples):
    """nmod_kmix_opts from the Python arguments; ValueError for what the C entry refuses"""
    _, model, max_iter, tol = _mix_args(1, model, max_iter, tol)
    if int(min_samples) != min_samples or int(min_samples) < 0:
        raise ValueError('min_samples must be an integer >= 0, not %r' % (min_samples,))
    return L.make_kmix_opts(model, max_iter, tol, int(min_samples))


def kmer_mix_host(sig, off, code, ncodes, mean0, sd0, *, stride=0, model='free', max_iter=200, tol=1e-6, min_samples=2, want_hist=False,
                  device=0):
    """The modified component per k-mer code of host-resident rows (nmod_kmer_mix, include/nanomod_hip.h): sig float32, int16
    (milli-units) or float64, rows by `off` (int64[npos + 1]) or a fixed `stride`; code int32[npos] in [-1, ncodes) (-1: the position
    takes no part); mean0 / sd0 float64[ncodes]: the unmodified component, a control's k-mer table.  model 'equal' / 'free' as
    mix_fraction_host.  Returns a dict of numpy arrays: n_positions, n_used, n_outside (int64[ncodes]), pi, mu_mod, sd_mod, llr
    (float64[ncodes]; llr is a score, not a test), iters (int32), status (uint8, L.KMIX_* bits), pos_status (uint8[npos], L.STATUS_*
    bits) and with want_hist `hist` (uint32[ncodes * L.KMIX_BINS], the pooled histogram of every code's window)."""
    lib = L.load()
    opts = _kmix_opts(model, max_iter, tol, min_samples)
    _join_warm_up(device)
    sig, dtype = _signal(sig, 'sig')
    code = np.ascontiguousarray(code, dtype=np.int32)
    if code.ndim != 1:
        raise ValueError('code must be int32[npos]')
    npos = code.shape[0]
    off, stride = _rows(sig, off, stride, npos, 'sig')
    ncodes = int(ncodes)
    mean0 = _side(mean0, np.float64, ncodes, 'mean0', 'ncodes', optional=False)
    sd0 = _side(sd0, np.float64, ncodes, 'sd0', 'ncodes', optional=False)
    res = _host_outputs(_kmix_shapes(npos, ncodes, bool(want_hist)))
    out = L.make_out(L.NmodKmixOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype, stride0=stride)
    _call(lib, 'nmod_kmer_mix', prm, npos, _np_ptr(sig), _np_ptr(off), _np_ptr(code), ncodes, _np_ptr(mean0), _np_ptr(sd0), C.byref(opts),
          C.byref(out))
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
        _check_kmer(k, center, center_unguarded=True)
    return L.make_rescale_opts(mode, weighted, clip_sigma, clip_rounds, min_events, lo, hi)


def rescale_reads_host(val, off, base, model=None, *, mode='fit_apply', weighted=True, clip_sigma=3.0, clip_rounds=2, min_events=50,
                       scale_range=(0.5, 2.0), shift=None, scale=None, device=0):
    """Per-read shift and scale against a k-mer model and the rescaled events (nmod_rescale_reads, include/nanomod_hip.h) on
    host-resident reads: val float32, int16 (milli-units) or float64 and base (S1 / uint8), one entry per event, reads by `off`
    (int64[nreads + 1]); model: a mapping with k, center, mean, sd (a kmermodel model) — not needed for mode 'apply_only', which
    takes shift / scale (float64[nreads]) instead.  Returns a dict of numpy arrays: shift, scale (float64), n_used (int32), status
    (uint8, L.RESCALE_* bits) and, unless mode is 'fit_only', val: the rescaled events in val's dtype."""
    lib = L.load()
    val, dtype = _signal(val, 'val')
    off, nreads, nev = _read_layout(val, off, 'val')
    k = center = None
    if model is not None:
        k, center = int(model['k']), int(model['center'])
    opts = _rescale_opts(mode, weighted, clip_sigma, clip_rounds, min_events, scale_range, k, center)
    fit, apply = opts.mode != L.RESCALE_APPLY_ONLY, opts.mode != L.RESCALE_FIT_ONLY
    if fit:
        m, alive = _host_model(model)
        base = _host_base(base, nev)
    else:
        if shift is None or scale is None:
            raise ValueError("mode 'apply_only' needs shift and scale")
        shift = np.array(shift, dtype=np.float64, order='C')
        scale = np.array(scale, dtype=np.float64, order='C')
        if shift.shape != (nreads,) or scale.shape != (nreads,):
            raise ValueError('shift / scale must be float64[nreads]')
        m, base = L.NmodRescaleModel(), None
    res = _host_outputs(_rescale_shapes(nreads, val.dtype if apply else None, val.shape[0]), fill=('n_used', 'status'))
    if not fit:
        res.update(shift=shift, scale=scale)                     # the pairs to apply: the entry's own copies of the caller's
    if apply:                                                    # events outside [off[0], off[-1]) belong to no read: copied through
        res['val'][nev:] = val[nev:]
        if nreads and off[0] > 0:
            res['val'][:off[0]] = val[:off[0]]
    _join_warm_up(device)
    out = L.make_out(L.NmodRescaleOut, **_np_ptrs({'val_out' if name == 'val' else name: a for name, a in res.items()}))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype)
    _call(lib, 'nmod_rescale_reads', prm, nreads, _np_ptr(off), _np_ptr(val), _np_ptr(base), C.byref(m), C.byref(opts), C.byref(out))
    return res


def _calls_opts(nb, alpha, k, center, want):
    """nmod_calls_opts from the Python arguments; ValueError for what the C entry refuses"""
    nb, alpha = int(nb), float(alpha)
    if not 0 <= nb <= L.MAX_NB:
        raise ValueError('nb must be in 0 .. %d' % L.MAX_NB)
    alpha = _check_alpha(alpha)
    _check_kmer(k, center)
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
    val, dtype = _signal(val, 'val')
    off, nreads, nev = _read_layout(val, off, 'val')
    if model is None:
        raise ValueError('read_calls needs a k-mer model')
    opts, want = _calls_opts(nb, alpha, int(model['k']), int(model['center']), want)
    m, alive = _host_model(model)
    base = _host_base(base, nev)
    shapes = _calls_shapes(want, val.shape[0], nreads)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_out(L.NmodCallsOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype)
    _call(lib, 'nmod_read_calls', prm, nreads, _np_ptr(off), _np_ptr(val), _np_ptr(base), C.byref(m), C.byref(opts), C.byref(out))
    if nreads and off[0] > 0:
        for w in want:                                          # events before the first read belong to no read
            res[w][:off[0]] = np.nan
    return res


def site_calls_host(score, off, *, stride=0, alpha=0.01, device=0):
    """Per-position call counts over pivoted scores (nmod_site_calls): score float64, one row per position by `off` (int64[npos + 1])
    or, with off None, a fixed `stride`.  Returns a dict of numpy arrays: n_valid (scores in [0, 1]), n_called (valid scores <= alpha),
    both int32, and frac = n_called / n_valid (float64, NaN without a valid score)."""
    lib = L.load()
    alpha = _check_alpha(alpha)
    score, off, stride, npos = _host_score_rows(score, off, stride)
    shapes = _site_shapes(npos)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_out(L.NmodSiteOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64, stride0=stride if off is None else 0)
    _call(lib, 'nmod_site_calls', prm, npos, _np_ptr(score), _np_ptr(off), alpha, C.byref(out))
    return res


def _check_thr(thr):
    import math
    thr = float(thr)
    if not (math.isfinite(thr) and thr > 0.0):
        raise ValueError('thr must be finite and positive')
    return thr


def _llr_opts(window, thr, prior_logit, k, center, alt_k, alt_center, want):
    """nmod_llr_opts from the Python arguments; ValueError for what the C entry refuses.  window: 'kmer' (the events whose k-mer holds
    the base: k - 1 - center before, center after) or (lo, hi)"""
    import math
    _check_kmer(k, center)
    if alt_k is None or alt_center is None or (int(alt_k), int(alt_center)) != (int(k), int(center)):
        raise ValueError('the two models must share k and center')
    if isinstance(window, str):
        if window != 'kmer':
            raise ValueError("window must be 'kmer' or (lo, hi)")
        lo, hi = int(k) - 1 - int(center), int(center)
    else:
        try:
            lo, hi = (int(v) for v in window)
        except (TypeError, ValueError):
            raise ValueError("window must be 'kmer' or (lo, hi)")
    if not (0 <= lo <= L.MAX_NB and 0 <= hi <= L.MAX_NB):
        raise ValueError('the window bounds must be in 0 .. %d' % L.MAX_NB)
    thr, prior_logit = _check_thr(thr), float(prior_logit)
    if not (math.isfinite(prior_logit) and abs(prior_logit) <= L.LLR_PRIOR_LOGIT_MAX):
        raise ValueError('prior_logit must be finite and within +-%g' % L.LLR_PRIOR_LOGIT_MAX)
    want = tuple(want)
    if any(w not in L.LLR_EVENT_FIELDS for w in want):
        raise ValueError("want must name tracks of 'llr', 'llr_win', 'p_mod'")
    return L.make_llr_opts(lo, hi, thr, prior_logit), want


def _llr_shapes(want, nval, nreads):
    return dict({w: ('float64', nval) for w in want}, n_sites=('int32', nreads), n_mod=('int32', nreads), n_can=('int32', nreads),
                status=('uint8', nreads))


def _site_llr_shapes(npos):
    return dict(n_valid=('int32', npos), n_mod=('int32', npos), n_can=('int32', npos), frac=('float64', npos))


def read_llr_host(val, off, base, model, alt, *, window='kmer', thr=2.5, prior_logit=0.0, want=('llr', 'llr_win', 'p_mod'), device=0):
    """Per-read log-likelihood ratios between two k-mer models (nmod_read_llr, include/nanomod_hip.h) on host-resident reads: val, off
    and base as for read_calls_host; model (unmodified) and alt (modified): mappings with k, center, mean, sd of one k and center.
    window: 'kmer' or (lo, hi) events of the same read before and after.  Returns a dict of numpy arrays: the per-event tracks named in
    `want` (float64, in val's layout: llr, the window sum llr_win, the posterior p_mod at prior_logit) and per read n_sites, n_mod,
    n_can (int32) and status (uint8, L.CALLS_TOO_LARGE)."""
    lib = L.load()
    val, dtype = _signal(val, 'val')
    off, nreads, nev = _read_layout(val, off, 'val')
    if model is None or alt is None:
        raise ValueError('read_llr needs two k-mer models')
    opts, want = _llr_opts(window, thr, prior_logit, int(model['k']), int(model['center']), int(alt['k']), int(alt['center']), want)
    m0, alive0 = _host_model(model)
    m1, alive1 = _host_model(alt)
    base = _host_base(base, nev)
    shapes = _llr_shapes(want, val.shape[0], nreads)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_out(L.NmodLlrOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype)
    _call(lib, 'nmod_read_llr', prm, nreads, _np_ptr(off), _np_ptr(val), _np_ptr(base), C.byref(m0), C.byref(m1), C.byref(opts), C.byref(out))
    if nreads and off[0] > 0:
        for w in want:                                          # events before the first read belong to no read
            res[w][:off[0]] = np.nan
    return res


def site_llr_host(score, off, *, stride=0, thr=2.5, device=0):
    """Per-position counts over pivoted window sums (nmod_site_llr): score float64, one row per position by `off` (int64[npos + 1]) or,
    with off None, a fixed `stride`.  Returns a dict of numpy arrays: n_valid (finite sums), n_mod (sums >= thr), n_can (sums <= -thr),
    all int32, and frac = n_mod / (n_mod + n_can) (float64, NaN without a confident read)."""
    lib = L.load()
    thr = _check_thr(thr)
    score, off, stride, npos = _host_score_rows(score, off, stride)
    shapes = _site_llr_shapes(npos)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_out(L.NmodSiteLlrOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64, stride0=stride if off is None else 0)
    _call(lib, 'nmod_site_llr', prm, npos, _np_ptr(score), _np_ptr(off), thr, C.byref(out))
    return res


def _stoich_opts(min_valid, ci_level, max_iter, tol):
    """nmod_stoich_opts from the Python arguments; ValueError for what the C entry refuses.  ci_level in (0, 1) becomes the drop of
    2 l that bounds the interval: the ci_level quantile of chi2_1, the square of a normal quantile"""
    import math
    from statistics import NormalDist
    if int(min_valid) != min_valid or int(min_valid) < 1:
        raise ValueError('min_valid must be an integer >= 1, not %r' % (min_valid,))
    if int(max_iter) != max_iter or not 1 <= int(max_iter) <= L.STOICH_MAX_ITER:
        raise ValueError('max_iter must be an integer in 1 .. %d, not %r' % (L.STOICH_MAX_ITER, max_iter))
    tol, ci_level = float(tol), float(ci_level)
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError('tol must be finite and >= 0, not %r' % (tol,))
    if not 0.0 < ci_level < 1.0:
        raise ValueError('ci_level must lie inside (0, 1), not %r' % (ci_level,))
    ci_drop = NormalDist().inv_cdf((1.0 + ci_level) / 2.0) ** 2
    if not (math.isfinite(ci_drop) and ci_drop > 0.0):
        raise ValueError('ci_level %r gives no usable interval' % (ci_level,))
    return L.make_stoich_opts(int(max_iter), int(min_valid), tol, ci_drop)


def _stoich_shapes(npos, nresp=None):
    shapes = dict({k: ('float64', npos) for k in L.STOICH_FIELDS}, n_valid=('int32', npos), iters=('int32', npos), status=('uint8', npos))
    if nresp is not None:
        shapes['resp'] = ('float64', nresp)
    return shapes


def site_stoich_host(score, off, *, stride=0, min_valid=3, ci_level=0.95, max_iter=60, tol=1e-12, resp=False, device=0):
    """Per-position modified fraction by maximum likelihood over pivoted window sums (nmod_site_stoich, include/nanomod_hip.h): score
    float64, one row per position by `off` (int64[npos + 1]) or, with off None, a fixed `stride`.  Returns a dict of numpy arrays: pi
    (the estimate), pi_lo, pi_hi (the likelihood interval at ci_level), stat (twice the log-likelihood ratio against pi = 0) and p_null
    (its asymptotic boundary p-value), float64; n_valid, iters (int32); status (uint8, L.STOICH_* bits); and with `resp` the posterior
    of every read at the estimate (float64, in the score layout)."""
    lib = L.load()
    opts = _stoich_opts(min_valid, ci_level, max_iter, tol)
    score, off, stride, npos = _host_score_rows(score, off, stride)
    shapes = _stoich_shapes(npos, score.shape[0] if resp else None)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_out(L.NmodStoichOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64, stride0=stride if off is None else 0)
    _call(lib, 'nmod_site_stoich', prm, npos, _np_ptr(score), _np_ptr(off), C.byref(opts), C.byref(out))
    if resp and npos and off is not None and off[0] > 0:
        res['resp'][:off[0]] = np.nan                               # scores before the first row belong to no row
    return res


def _llr_multi_opts(window, thr, prior_logit, k, center, alt_kc, want):
    """nmod_llr_multi_opts from the Python arguments (the window, thr and each prior through _llr_opts, K13's rules); ValueError for what
    the C entry refuses.  alt_kc: (k, center) of every alternative table; prior_logit: None (all 0), or one value per table"""
    n_alt = len(alt_kc)
    if not 1 <= n_alt <= L.MULTI_MAX:
        raise ValueError('read_llr_multi takes 1 .. %d alternative models, not %d' % (L.MULTI_MAX, n_alt))
    prior_logit = [0.0] * n_alt if prior_logit is None else [float(v) for v in np.atleast_1d(np.asarray(prior_logit, dtype=np.float64))]
    if len(prior_logit) != n_alt:
        raise ValueError('prior_logit needs one value per alternative model')
    for (ak, ac), pl in zip(alt_kc, prior_logit):
        one, _ = _llr_opts(window, thr, pl, k, center, ak, ac, ())
    want = tuple(want)
    if any(w not in L.LLR_MULTI_EVENT_FIELDS for w in want):
        raise ValueError("want must name tracks of 'llr', 'llr_win', 'post', 'call'")
    return L.make_llr_multi_opts(one.nb_lo, one.nb_hi, one.thr, prior_logit), want


_LLR_MULTI_PLANES = dict(llr=0, llr_win=0, post=1)           # planes of an event track beyond n_alt


def _llr_multi_shapes(want, nval, nreads, n_alt):
    shapes = {w: ('uint8', nval) if w == 'call' else ('float64', (n_alt + _LLR_MULTI_PLANES[w]) * nval) for w in want}
    shapes.update(n_sites=('int32', nreads), n_can=('int32', nreads), n_mod=('int32', n_alt * nreads), status=('uint8', nreads))
    return shapes


def _llr_multi_views(res, nval, nreads, n_alt):
    """the flat outputs as (planes, events) / (n_alt, nreads) views"""
    out = dict(res)
    for w in ('llr', 'llr_win', 'post'):
        if w in out:
            out[w] = out[w].reshape(n_alt + _LLR_MULTI_PLANES[w], nval)
    out['n_mod'] = out['n_mod'].reshape(n_alt, nreads)
    return out


def read_llr_multi_host(val, off, base, model, alts, *, window='kmer', thr=2.5, prior_logit=None, want=('llr', 'llr_win', 'post', 'call'), device=0):
    """Per-read log-likelihood ratios of one unmodified k-mer model against several modified ones in one walk, with a joint call and a
    posterior over the states per event (nmod_read_llr_multi, include/nanomod_hip.h), on host-resident reads: val, off, base and model
    as for read_llr_host; alts: 1 .. L.MULTI_MAX mappings with k, center, mean, sd (k and center as model's); prior_logit: the log
    prior odds of each state against canonical (None: 0).  Returns a dict of numpy arrays: the tracks named in `want` — llr, llr_win
    (float64[n_alt, events]: row m - 1 holds the bits read_llr_host gives for (model, alts[m - 1])), post (float64[n_alt + 1, events], row 0
    canonical), call (uint8: 0 canonical, m, L.MULTI_AMBIGUOUS, L.MULTI_NONE) — and per read n_sites, n_can (int32), n_mod
    (int32[n_alt, nreads]) and status (uint8, L.CALLS_TOO_LARGE)."""
    lib = L.load()
    val, dtype = _signal(val, 'val')
    off, nreads, nev = _read_layout(val, off, 'val')
    if model is None or alts is None or any(a is None for a in alts):
        raise ValueError('read_llr_multi needs a k-mer model and its alternatives')
    alts = list(alts)
    opts, want = _llr_multi_opts(window, thr, prior_logit, int(model['k']), int(model['center']), [(int(a['k']), int(a['center'])) for a in alts], want)
    n_alt = len(alts)
    m0, alive0 = _host_model(model)
    ms = [_host_model(a) for a in alts]
    arr = L.model_ptr_array([m for m, _ in ms])
    base = _host_base(base, nev)
    nval = val.shape[0]
    shapes = _llr_multi_shapes(want, nval, nreads, n_alt)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_out(L.NmodLlrMultiOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=dtype)
    _call(lib, 'nmod_read_llr_multi', prm, nreads, nval, _np_ptr(off), _np_ptr(val), _np_ptr(base), C.byref(m0), n_alt, C.addressof(arr),
          C.byref(opts), C.byref(out))
    res = _llr_multi_views(res, nval, nreads, n_alt)
    lo, hi = (int(off[0]), nev) if nreads else (nval, nval)     # events outside [off[0], off[-1]) belong to no read
    for w in want:
        res[w][..., :lo] = L.MULTI_NONE if w == 'call' else np.nan
        res[w][..., hi:] = L.MULTI_NONE if w == 'call' else np.nan
    return res


def _compose_opts(n_alt, min_valid, max_iter, tol):
    """nmod_compose_opts from the Python arguments; ValueError for what the C entry refuses"""
    import math
    if not 1 <= n_alt <= L.MULTI_MAX:
        raise ValueError('site_compose takes the scores of 1 .. %d states, not %d' % (L.MULTI_MAX, n_alt))
    if int(min_valid) != min_valid or int(min_valid) < 1:
        raise ValueError('min_valid must be an integer >= 1, not %r' % (min_valid,))
    if int(max_iter) != max_iter or not 1 <= int(max_iter) <= L.COMPOSE_MAX_ITER:
        raise ValueError('max_iter must be an integer in 1 .. %d, not %r' % (L.COMPOSE_MAX_ITER, max_iter))
    tol = float(tol)
    if not (math.isfinite(tol) and tol >= 0.0):
        raise ValueError('tol must be finite and >= 0, not %r' % (tol,))
    return L.make_compose_opts(int(max_iter), int(min_valid), tol)


def _compose_shapes(npos, n_alt, test=True, nresp=None):
    shapes = dict(pi=('float64', (n_alt + 1) * npos), ll=('float64', npos), stat=('float64', npos))
    if test:
        shapes.update(stat_m=('float64', n_alt * npos), p_m=('float64', n_alt * npos))
    shapes.update(n_valid=('int32', npos), n_partial=('int32', npos), iters=('int32', npos), open_mask=('uint8', npos), status=('uint8', npos))
    if nresp is not None:
        shapes['resp'] = ('float64', (n_alt + 1) * nresp)
    return shapes


def _compose_views(res, npos, n_alt):
    out = dict(res)
    out['pi'] = out['pi'].reshape(n_alt + 1, npos)
    for w in ('stat_m', 'p_m'):
        if w in out:
            out[w] = out[w].reshape(n_alt, npos)
    if 'resp' in out:
        out['resp'] = out['resp'].reshape(n_alt + 1, -1)
    return out


def site_compose_host(scores, off, *, stride=0, min_valid=3, max_iter=500, tol=1e-9, test=True, resp=False, device=0):
    """The shares of all states per position by maximum likelihood over pivoted window sums (nmod_site_compose, include/nanomod_hip.h):
    scores: 1 .. L.MULTI_MAX float64 vectors of one length (or a 2-d array, a row per state), all read by the one `off`
    (int64[npos + 1]) or, with off None, a fixed `stride`.  Returns a dict of numpy arrays: pi (float64[n_alt + 1, npos], row 0
    canonical), ll, stat; with `test` stat_m and p_m (float64[n_alt, npos]: the likelihood-ratio test of each state's share being 0,
    an asymptotic boundary p-value); n_valid, n_partial, iters (int32); open_mask and status (uint8, L.COMPOSE_* bits); and with `resp`
    the responsibilities of every read (float64[n_alt + 1, scores])."""
    lib = L.load()
    scores = [s for s in scores]
    opts = _compose_opts(len(scores), min_valid, max_iter, tol)
    n_alt = len(scores)
    rows = [_host_score_rows(s, off, stride) for s in scores]
    score0, off, stride, npos = rows[0]
    if any(r[0].shape != score0.shape for r in rows):
        raise ValueError('the scores of all states must have one length')
    total = score0.shape[0]
    shapes = _compose_shapes(npos, n_alt, test, total if resp else None)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_out(L.NmodComposeOut, **_np_ptrs(res))
    ptrs = (C.c_void_p * n_alt)(*[_np_ptr(r[0]) for r in rows])
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64, stride0=stride if off is None else 0)
    _call(lib, 'nmod_site_compose', prm, npos, total, n_alt, C.addressof(ptrs), _np_ptr(off), C.byref(opts), C.byref(out))
    res = _compose_views(res, npos, n_alt)
    if resp and off is not None:                                     # scores outside every row belong to no row
        lo, hi = (int(off[0]), int(off[-1])) if npos else (total, total)
        res['resp'][:, :lo] = np.nan
        res['resp'][:, hi:] = np.nan
    return res


def _diff_opts(min_valid, ci_level, max_iter, tol):
    """nmod_diff_opts from the Python arguments: the checks and the conversion of ci_level are those of _stoich_opts"""
    o = _stoich_opts(min_valid, ci_level, max_iter, tol)
    return L.make_diff_opts(o.max_iter, o.min_valid, o.tol, o.ci_drop)


def _diff_shapes(npos, interval=True):
    shapes = dict({k: ('float64', npos) for k in L.DIFF_FIELDS if interval or k not in ('delta_lo', 'delta_hi')},
                  **{k: ('int32', npos) for k in L.DIFF_INT_FIELDS})
    shapes['status'] = ('uint8', npos)
    return shapes


def site_diff_host(score0, off0, score1, off1, *, stride0=0, stride1=0, min_valid=3, ci_level=0.95, max_iter=60, tol=1e-12, interval=True,
                   device=0):
    """The modified shares of two samples compared per site (nmod_site_diff, include/nanomod_hip.h): per sample the float64 window
    sums, one row per site by its `off` (int64[npos + 1]) or, with off None, its fixed stride; both samples hold the same sites in the
    same order.  Returns a dict of numpy arrays: pi0, pi1, pi_pool, delta = pi1 - pi0, with `interval` its profile-likelihood interval
    delta_lo, delta_hi at ci_level, stat (the likelihood-ratio statistic of pi0 = pi1) and p_diff (its chi2_1 tail), float64;
    n_valid0, n_valid1, iters (int32); status (uint8, L.DIFF_* bits)."""
    lib = L.load()
    opts = _diff_opts(min_valid, ci_level, max_iter, tol)
    score0, off0, stride0, npos = _host_score_rows(score0, off0, stride0)
    score1, off1, stride1, npos1 = _host_score_rows(score1, off1, stride1)
    if npos1 != npos:
        raise ValueError('the two samples must hold the same sites: %d rows against %d' % (npos, npos1))
    shapes = _diff_shapes(npos, interval)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_out(L.NmodDiffOut, **_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64, stride0=stride0 if off0 is None else 0,
                        stride1=stride1 if off1 is None else 0)
    _call(lib, 'nmod_site_diff', prm, npos, _np_ptr(score0), _np_ptr(off0), _np_ptr(score1), _np_ptr(off1), C.byref(opts), C.byref(out))
    return res


def _t_two_sided_cdf(t, df):
    """P(|T| <= t) of Student's t on an integer df >= 1 by the finite series in theta = atan(t / sqrt(df)) (Abramowitz & Stegun
    26.7.3 / 26.7.4): no special function beyond atan, exact to rounding for the df <= 14 nmod_site_diff_rep can have"""
    import math
    theta = math.atan(t / math.sqrt(df))
    s, c2 = math.sin(theta), math.cos(theta) ** 2
    if df % 2:
        term, total = math.cos(theta), 0.0                          # cos, 2/3 cos^3, (2 4)/(3 5) cos^5, ... up to cos^(df - 2)
        for j in range(1, (df - 1) // 2 + 1):
            total += term
            term *= c2 * (2.0 * j) / (2.0 * j + 1.0)
        return 2.0 / math.pi * (theta + s * total)
    term, total = 1.0, 0.0                                          # 1, 1/2 cos^2, (1 3)/(2 4) cos^4, ... up to cos^(df - 2)
    for j in range(1, df // 2 + 1):
        total += term
        term *= c2 * (2.0 * j - 1.0) / (2.0 * j)
    return s * total


def _f1_quantile(level, df):
    """the `level` quantile of F(1, df), the square of the two-sided t quantile, by bisection on the monotone _t_two_sided_cdf: the
    package imports no scipy"""
    lo, hi = 0.0, 1.0
    while _t_two_sided_cdf(hi, df) < level:
        lo, hi = hi, 2.0 * hi
        if hi > 1e300:
            return float('inf')
    for _ in range(200):
        mid = lo + 0.5 * (hi - lo)
        if mid <= lo or mid >= hi:
            break
        if _t_two_sided_cdf(mid, df) < level:
            lo = mid
        else:
            hi = mid
    t = lo + 0.5 * (hi - lo)
    return t * t


def _rep_opts(n_samples, n_control, min_valid, ci_level, phi_floor, max_iter, tol):
    """nmod_rep_opts from the Python arguments, and (G, ncontrol): _stoich_opts' checks and ValueError for what the C entry refuses of
    G, ncontrol and phi_floor.  ci_level becomes the drop the interval of delta is scaled from: the ci_level quantile of F(1, G - 2)"""
    import math
    o = _stoich_opts(min_valid, ci_level, max_iter, tol)
    if int(n_samples) != n_samples or not 3 <= int(n_samples) <= L.REP_MAX_SAMPLES:
        raise ValueError('n_samples must be an integer in 3 .. %d (two samples: site_diff), not %r' % (L.REP_MAX_SAMPLES, n_samples))
    if int(n_control) != n_control or not 1 <= int(n_control) <= int(n_samples) - 1:
        raise ValueError('n_control must be an integer in 1 .. n_samples - 1, not %r' % (n_control,))
    phi_floor = float(phi_floor)
    if not (math.isfinite(phi_floor) and phi_floor >= 0.0):
        raise ValueError('phi_floor must be finite and >= 0, not %r' % (phi_floor,))
    ci_drop = _f1_quantile(float(ci_level), int(n_samples) - 2)
    if not (math.isfinite(ci_drop) and ci_drop > 0.0):
        raise ValueError('ci_level %r gives no usable interval' % (ci_level,))
    return L.make_rep_opts(o.max_iter, o.min_valid, o.tol, ci_drop, phi_floor), int(n_samples), int(n_control)


def _rep_shapes(npos, n_samples, interval=True, moderated=False):
    shapes = {k: ('float64', npos * n_samples) for k in L.REP_SAMPLE_FIELDS}
    shapes.update({k: ('float64', npos) for k in L.REP_FIELDS if interval or k not in ('delta_lo', 'delta_hi')})
    if moderated:
        shapes['phi_post'] = ('float64', npos)
    shapes.update({k: ('int32', npos * n_samples) for k in L.REP_SAMPLE_INT_FIELDS})
    shapes.update({k: ('int32', npos) for k in L.REP_INT_FIELDS})
    shapes['status'] = ('uint8', npos)
    return shapes


def _rep_npos(nrows, n_samples, what):
    if nrows % n_samples:
        raise ValueError('%s: off must hold n_samples rows per site: %d rows of %d samples' % (what, nrows, n_samples))
    return nrows // n_samples


def _rep_prior_args(df, ci_level):
    """(df, ci_level) as nmod_rep_prior takes them; ValueError for what it refuses"""
    if int(df) != df or not 1 <= int(df) <= L.REP_MAX_SAMPLES - 2:
        raise ValueError('df must be an integer in 1 .. %d (n_samples - 2), not %r' % (L.REP_MAX_SAMPLES - 2, df))
    ci_level = float(ci_level)
    if not 0.0 < ci_level < 1.0:
        raise ValueError('ci_level must lie strictly between 0 and 1, not %r' % (ci_level,))
    return int(df), ci_level


def rep_prior_record(prior):
    """the record of nmod_rep_prior as 8 float64: from rep_prior_host's dict, or any sequence of 8 numbers as it is"""
    rec = np.array([prior[f] for f in L.REP_PRIOR_FIELDS] if isinstance(prior, dict) else prior, dtype=np.float64)
    if rec.shape != (L.REP_PRIOR_WORDS,):
        raise ValueError('prior must hold the %d doubles of nmod_rep_prior\'s record' % L.REP_PRIOR_WORDS)
    return np.ascontiguousarray(rec)


def rep_prior_host(phi, status, df, *, ci_level=0.95, device=0):
    """The prior law of the per-site dispersions of site_diff_rep_host fitted over all sites (nmod_rep_prior, include/nanomod_hip.h):
    phi float64 and status uint8 as site_diff_rep_host returned them, df = n_samples - 2.  Returns the record as a dict of floats: d0
    (the prior's degrees of freedom; 0: no prior, inf: one dispersion for all), s0sq, df_tot = df + d0, ci_drop (the ci_level
    quantile of F(1, df_tot)), n_used, n_zero, emean, evar.  site_diff_rep_host(..., prior=) takes it as it is."""
    lib = L.load()
    df, ci_level = _rep_prior_args(df, ci_level)
    phi, status = np.ascontiguousarray(phi, dtype=np.float64), np.ascontiguousarray(status, dtype=np.uint8)
    if phi.ndim != 1 or phi.shape != status.shape:
        raise ValueError('rep_prior: phi and status must be vectors of one length')
    rec = np.full(L.REP_PRIOR_WORDS, np.nan)
    _join_warm_up(device)
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    _call(lib, 'nmod_rep_prior', prm, len(phi), df, _np_ptr(phi), _np_ptr(status), ci_level, _np_ptr(rec))
    return dict(zip(L.REP_PRIOR_FIELDS, rec.tolist()))


def site_diff_rep_host(score, off, n_samples, n_control, *, min_valid=3, ci_level=0.95, phi_floor=0.0, max_iter=60, tol=1e-12, interval=True,
                       prior=None, device=0):
    """The modified shares of two replicated conditions compared per site (nmod_site_diff_rep, include/nanomod_hip.h): score float64,
    off int64[npos * n_samples + 1], row i * n_samples + g for site i and sample g; the first n_control samples of every site are
    condition 0.  Returns a dict of numpy arrays: pi_s and n_valid per sample (npos * n_samples); per site pi0, pi1, pi_pool, delta,
    with `interval` delta_lo and delta_hi at ci_level, stat_cond and p_cond (site_diff's test of the pooled reads), stat_het, p_het and
    phi (the heterogeneity of the replicates and the dispersion), p_rep (the F(1, n_samples - 2) test of delta that carries it),
    float64; iters (int32); status (uint8, L.REP_* bits).  phi_floor: the dispersion never counts as less (1.0: never below binomial).
    prior: the record of rep_prior_host (its dict, or 8 doubles): nmod_site_diff_rep_mod — phi is moderated under it, p_rep is on the
    record's df_tot, the interval is at the record's quantile (ci_level is then unused) and the result gains phi_post."""
    lib = L.load()
    opts, n_samples, n_control = _rep_opts(n_samples, n_control, min_valid, ci_level, phi_floor, max_iter, tol)
    rec = None if prior is None else rep_prior_record(prior)
    if off is None:
        raise ValueError('site_diff_rep takes CSR rows: off is required')
    score, off, _, nrows = _host_score_rows(score, off, 0)
    npos = _rep_npos(nrows, n_samples, 'site_diff_rep')
    shapes = _rep_shapes(npos, n_samples, interval, moderated=rec is not None)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_out(L.NmodRepOut, **_np_ptrs({k: v for k, v in res.items() if k != 'phi_post'}))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    if rec is None:
        _call(lib, 'nmod_site_diff_rep', prm, npos, n_samples, n_control, _np_ptr(score), _np_ptr(off), C.byref(opts), C.byref(out))
    else:
        _call(lib, 'nmod_site_diff_rep_mod', prm, npos, n_samples, n_control, _np_ptr(score), _np_ptr(off), C.byref(opts), C.byref(out),
              _np_ptr(rec), _np_ptr(res['phi_post']))
    return res


PAIRS_OUTPUTS = L.PAIRS_INT_FIELDS + L.PAIRS_FIELDS + ('status',)


def _check_max_dist(max_dist):
    if int(max_dist) != max_dist or not 1 <= int(max_dist) <= L.PAIRS_MAX_DIST:
        raise ValueError('max_dist must be an integer in 1 .. %d, not %r' % (L.PAIRS_MAX_DIST, max_dist))
    return int(max_dist)


def _pairs_opts(thr, min_reads, force_direct, want):
    """nmod_pairs_opts from the Python arguments; ValueError for what the C entry refuses"""
    thr = _check_thr(thr)
    if int(min_reads) != min_reads or int(min_reads) < 1:
        raise ValueError('min_reads must be an integer >= 1, not %r' % (min_reads,))
    want = tuple(want)
    if any(w not in PAIRS_OUTPUTS for w in want):
        raise ValueError('want must name outputs of %s' % ', '.join(PAIRS_OUTPUTS))
    return L.make_pairs_opts(thr, int(min_reads), L.PAIRS_FORCE_DIRECT if force_direct else 0), want


def _check_pair_counts(nreads, nsites, npairs):
    if nreads > 2 ** 31 - 1:
        raise ValueError('at most 2^31 - 1 reads')
    if nsites > 2 ** 31 - 2:
        raise ValueError('at most 2^31 - 2 sites')
    if int(npairs) != npairs or not 0 <= int(npairs) <= 2 ** 31 - 1:
        raise ValueError('npairs must be an integer in 0 .. 2^31 - 1, not %r' % (npairs,))
    return int(npairs)


def _pairs_shapes(want, npairs):
    kinds = dict(counts=('int32', 4 * npairs), first=('int32', npairs), second=('int32', npairs), status=('uint8', npairs),
                 **{k: ('float64', npairs) for k in L.PAIRS_FIELDS})
    return {k: kinds[k] for k in PAIRS_OUTPUTS if k in want}


def _host_keys(key):
    key = np.ascontiguousarray(key, dtype=np.int64)
    if key.ndim != 1 or (key.shape[0] and (key[0] < 0 or bool(np.any(np.diff(key) <= 0)))):
        raise ValueError('key must be an int64 vector of cs << 40 | pos, strictly ascending')
    return key


def pair_index_host(key, max_dist=100, device=0):
    """The pairs of candidate sites at most max_dist apart on one (chrom, strand) (nmod_pair_index, include/nanomod_hip.h): key int64,
    cs << 40 | pos, strictly ascending.  Returns poff (int64[nsites + 1]): pair (a, b) has the index poff[a] + (b - a - 1), poff[-1]
    pairs in all."""
    lib = L.load()
    max_dist = _check_max_dist(max_dist)
    key = _host_keys(key)
    _check_pair_counts(0, key.shape[0], 0)
    poff = np.zeros(key.shape[0] + 1, dtype=np.int64)
    npairs = C.c_int64(0)
    _join_warm_up(device)
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    _call(lib, 'nmod_pair_index', prm, key.shape[0], _np_ptr(key), max_dist, _np_ptr(poff), C.byref(npairs))
    return poff


def site_pairs_host(cs, start, roff, score, key, poff, *, thr=2.5, min_reads=10, force_direct=False, want=PAIRS_OUTPUTS, device=0):
    """Same-read co-occurrence of calls at pairs of sites (nmod_site_pairs, include/nanomod_hip.h) on host-resident reads: cs (int32,
    2 * chrom index + (strand == '-')), start (int64) and roff (int64[nreads + 1]) as nmod_pivot_reads takes them, score (float64, one
    per event in read direction: K13's llr_win), key and poff as pair_index_host gives them.  Returns a dict of numpy arrays, those
    named in `want`: counts (int32[4 npairs]: n00, n01, n10, n11 of each pair, the first index site a's call), first, second (int32),
    log_or, se, phi, p_fisher (float64) and status (uint8, L.PAIRS_* bits)."""
    lib = L.load()
    opts, want = _pairs_opts(thr, min_reads, force_direct, want)
    cs, start, roff, score, key, poff, nreads, npairs = _host_pair_reads(cs, start, roff, score, key, poff)
    shapes = _pairs_shapes(want, npairs)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_pairs_out(**_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    _call(lib, 'nmod_site_pairs', prm, nreads, _np_ptr(cs), _np_ptr(start), _np_ptr(roff), _np_ptr(score), key.shape[0], _np_ptr(key),
          _np_ptr(poff), npairs, C.byref(opts), C.byref(out))
    return res


def _link_opts(min_reads, ci_level, max_iter, tol):
    """nmod_link_opts from the Python arguments: the checks and the conversion of ci_level are those of _stoich_opts"""
    if int(min_reads) != min_reads or int(min_reads) < 1:
        raise ValueError('min_reads must be an integer >= 1, not %r' % (min_reads,))
    o = _stoich_opts(1, ci_level, max_iter, tol)
    return L.make_link_opts(o.max_iter, int(min_reads), o.tol, o.ci_drop)


def _link_shapes(npairs, interval=True):
    shapes = dict({k: ('float64', npairs) for k in L.LINK_FIELDS if interval or k not in ('d_lo', 'd_hi')},
                  **{k: ('int32', npairs) for k in L.LINK_INT_FIELDS})
    shapes['status'] = ('uint8', npairs)
    return shapes


def _host_site_reads(cs, start, roff, score, key):
    """the reads and sites of a host call that walks the reads over candidate sites (K16, K18, K19), checked"""
    score = np.ascontiguousarray(score, dtype=np.float64)
    roff, nreads, _ = _read_layout(score, roff, 'score')
    cs = _side(cs, np.int32, nreads, 'cs', 'nreads', optional=False)
    start = _side(start, np.int64, nreads, 'start', 'nreads', optional=False)
    return cs, start, roff, score, _host_keys(key), nreads


def _host_pair_reads(cs, start, roff, score, key, poff):
    """the reads, sites and pair index of a host call as site_pairs_host checks them"""
    cs, start, roff, score, key, nreads = _host_site_reads(cs, start, roff, score, key)
    poff = _side(poff, np.int64, key.shape[0] + 1, 'poff', 'nsites + 1', optional=False)
    if poff[0] != 0 or bool(np.any(np.diff(poff) < 0)):
        raise ValueError('poff must start at 0 and never decrease')
    npairs = _check_pair_counts(nreads, key.shape[0], int(poff[-1]))
    return cs, start, roff, score, key, poff, nreads, npairs


def pair_rows_host(cs, start, roff, score, key, poff, device=0):
    """Per pair of sites the reads with a valid score at both (nmod_pair_rows_count, nmod_pair_rows_fill, include/nanomod_hip.h):
    the arguments of site_pairs_host.  Returns a dict of numpy arrays: prow_off (int64[npairs + 1]) and, per row, sa, sb (float64: the
    read's scores at the pair's two sites) and read (int32); within a pair the rows are in ascending read index."""
    lib = L.load()
    cs, start, roff, score, key, poff, nreads, npairs = _host_pair_reads(cs, start, roff, score, key, poff)
    prow_off = np.zeros(npairs + 1, dtype=np.int64)
    nrows = C.c_int64(0)
    _join_warm_up(device)
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    shared = (prm, nreads, _np_ptr(cs), _np_ptr(start), _np_ptr(roff), _np_ptr(score), key.shape[0], _np_ptr(key), _np_ptr(poff), npairs)
    _call(lib, 'nmod_pair_rows_count', *shared, _np_ptr(prow_off), C.byref(nrows))
    n = int(nrows.value)
    res = dict(prow_off=prow_off, sa=np.zeros(n), sb=np.zeros(n), read=np.zeros(n, dtype=np.int32))
    _call(lib, 'nmod_pair_rows_fill', *shared, _np_ptr(prow_off), n, _np_ptr(res['sa']), _np_ptr(res['sb']), _np_ptr(res['read']))
    return res


def pair_linkage_host(sa, sb, prow_off, *, min_reads=20, ci_level=0.95, max_iter=60, tol=1e-12, interval=True, device=0):
    """Soft same-read linkage of pairs of sites (nmod_pair_linkage, include/nanomod_hip.h) on host-resident rows: sa, sb (float64) and
    prow_off (int64[npairs + 1]) as pair_rows_host gives them.  Returns a dict of numpy arrays: pa, pb (the marginal shares, K14's
    estimates), d (the linkage), with `interval` its likelihood interval d_lo, d_hi at ci_level, r, stat (the likelihood-ratio
    statistic of independence) and p_indep (its chi2_1 tail), float64; n_valid, iters (int32); status (uint8, L.LINK_* bits)."""
    lib = L.load()
    opts = _link_opts(min_reads, ci_level, max_iter, tol)
    sa = np.ascontiguousarray(sa, dtype=np.float64)
    sb = np.ascontiguousarray(sb, dtype=np.float64)
    if sa.ndim != 1 or sb.shape != sa.shape:
        raise ValueError('sa and sb must be float64 vectors of one length')
    prow_off, npairs, _ = _read_layout(sa, prow_off, 'sa')
    if npairs > 2 ** 31 - 2:
        raise ValueError('at most 2^31 - 2 pairs')
    shapes = _link_shapes(npairs, interval)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_link_out(**_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    _call(lib, 'nmod_pair_linkage', prm, npairs, _np_ptr(sa), _np_ptr(sb), _np_ptr(prow_off), C.byref(opts), C.byref(out))
    return res


HMM_OUTPUTS = L.HMM_ENTRY_FIELDS + L.HMM_READ_FIELDS + L.HMM_SITE_FIELDS


def _check_chain(pi, length):
    """the two parameters of the read chain (K19, K20, K21) as floats; ValueError outside the ranges the C entries accept"""
    pi, length = float(pi), float(length)
    if not 1e-9 <= pi <= 1.0 - 1e-9:
        raise ValueError('pi must lie in 1e-9 .. 1 - 1e-9, not %r' % (pi,))
    if not 1e-3 <= length <= 1e9:
        raise ValueError('length must lie in 1e-3 .. 1e9 bases, not %r' % (length,))
    return pi, length


def _check_want(want, outputs):
    want = tuple(want)
    if any(w not in outputs for w in want):
        raise ValueError('want must name outputs of %s' % ', '.join(outputs))
    return want


def _hmm_opts(pi, length, call_post, want):
    """nmod_hmm_opts from the Python arguments; ValueError for what the C entry refuses"""
    call_post = float(call_post)
    pi, length = _check_chain(pi, length)
    if not 0.5 < call_post < 1.0:
        raise ValueError('call_post must lie inside (0.5, 1), not %r' % (call_post,))
    return L.make_hmm_opts(pi, length, call_post), _check_want(want, HMM_OUTPUTS)


def _check_hmm_counts(nreads, nsites, nrows):
    _check_pair_counts(nreads, nsites, 0)
    if int(nrows) != nrows or not 0 <= int(nrows) <= 2 ** 31 - 1:
        raise ValueError('nrows must be an integer in 0 .. 2^31 - 1, not %r' % (nrows,))
    return int(nrows)


def _hmm_shapes(want, nrows, nreads, nsites):
    kinds = dict(post=('float64', nrows), site=('int32', nrows), state=('uint8', nrows), ll=('float64', nreads), ll_indep=('float64', nreads),
                 status=('uint8', nreads), **{k: ('int32', nreads) for k in ('n_sites', 'n_mod', 'n_can', 'n_runs')},
                 **{k: ('int32', nsites) for k in L.HMM_SITE_FIELDS})
    return {k: kinds[k] for k in HMM_OUTPUTS if k in want}


def read_sites_host(cs, start, roff, score, key, device=0):
    """Per read the candidate sites it covers with a valid score, counted (nmod_read_sites_count, include/nanomod_hip.h): the reads,
    scores and keys of site_pairs_host.  Returns hoff (int64[nreads + 1]): the entries of read r are the rows hoff[r] .. hoff[r + 1] - 1
    of read_hmm_host's per-entry outputs."""
    lib = L.load()
    cs, start, roff, score, key, nreads = _host_site_reads(cs, start, roff, score, key)
    _check_hmm_counts(nreads, key.shape[0], 0)
    hoff = np.zeros(nreads + 1, dtype=np.int64)
    nrows = C.c_int64(0)
    _join_warm_up(device)
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    _call(lib, 'nmod_read_sites_count', prm, nreads, _np_ptr(cs), _np_ptr(start), _np_ptr(roff), _np_ptr(score), key.shape[0], _np_ptr(key),
          _np_ptr(hoff), C.byref(nrows))
    return hoff


def _check_chain_offsets(hoff, nreads):
    """hoff of a host chain entry (its last element is the entry's nrows: _check_class_offsets without the end)"""
    hoff = _side(hoff, np.int64, nreads + 1, 'hoff', 'nreads + 1', optional=False)
    if hoff[0] != 0 or bool(np.any(np.diff(hoff) < 0)):
        raise ValueError('hoff must start at 0 and never decrease')
    return hoff


def _host_site_pi(site_pi, nsites):
    """the per-site shares of a host prior entry (K23): a float64 array of nsites elements, its values as they are (the entry clamps
    them and takes a NaN for `no estimate`); nothing is converted: another dtype or length is a ValueError"""
    if not isinstance(site_pi, np.ndarray) or site_pi.dtype != np.float64 or site_pi.shape != (nsites,):
        raise ValueError('site_pi must be a numpy float64[nsites] array (nsites = %d)' % nsites)
    return np.ascontiguousarray(site_pi)


def _chain_host(entry, make_out, shapes, opts, reads, hoff, device, site_pi=None):
    """What the host wrappers of the chain entries (K19 .. K22) share after the checks of their own arguments.  entry: the C entry's
    name; make_out: its out struct from pointers by name; shapes(nrows, nreads, nsites): the table of its outputs; opts: its opts
    struct, None for an entry without one (the class rows); reads: (cs, start, roff, score, key); hoff: None, computed here;
    site_pi: None, or the per-site shares: the entry is then <entry>_prior, which takes them after key (K23).
    Returns the outputs and hoff."""
    cs, start, roff, score, key, nreads = _host_site_reads(*reads)
    if site_pi is not None:
        site_pi = _host_site_pi(site_pi, key.shape[0])
    if hoff is None:
        hoff = read_sites_host(cs, start, roff, score, key, device)
    hoff = _check_chain_offsets(hoff, nreads)
    nrows = _check_hmm_counts(nreads, key.shape[0], int(hoff[-1]))
    if opts is None and nrows > 0 and (nreads == 0 or key.shape[0] == 0):   # (with opts this refusal is the library's, as it has been)
        raise ValueError('rows need reads and sites')
    shapes = shapes(nrows, nreads, key.shape[0])
    res = _host_outputs(shapes, fill=shapes)
    lib = L.load()
    _join_warm_up(device)
    out = make_out(**_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    prior = () if site_pi is None else (_np_ptr(site_pi),)
    _call(lib, entry + ('_prior' if prior else ''), prm, nreads, _np_ptr(cs), _np_ptr(start), _np_ptr(roff), _np_ptr(score), key.shape[0],
          _np_ptr(key), *prior, _np_ptr(hoff), nrows, *(() if opts is None else (C.byref(opts),)), C.byref(out))
    res['hoff'] = hoff
    return res


def read_hmm_host(cs, start, roff, score, key, hoff=None, *, pi=0.5, length=200.0, call_post=0.9, want=HMM_OUTPUTS, device=0, site_pi=None):
    """Per-read two-state HMM smoothing of the window sums at candidate sites (nmod_read_hmm, include/nanomod_hip.h) on host-resident
    reads: the arguments of read_sites_host and the hoff it gives (None: computed here).  pi: the stationary modified share; length: the
    correlation length in bases; call_post: the posterior from which an entry is called; site_pi: None, or a float64 array of one modified
    share per candidate site (nmod_read_hmm_prior, K23: clamped to 1e-9 .. 1 - 1e-9 by the entry, a NaN stands for pi; read_viterbi_host
    and read_hmm_grad_host take it in the same way).  Returns a dict of numpy arrays, hoff and those
    named in `want`: per entry post (float64), site (int32, the index into key), state (uint8: 1 modified, 0 canonical, 2 neither); per
    read n_sites, n_mod, n_can, n_runs (int32), ll, ll_indep (float64), status (uint8, L.HMM_NO_SITE); per site site_n, site_mod,
    site_can (int32)."""
    opts, want = _hmm_opts(pi, length, call_post, want)
    return _chain_host('nmod_read_hmm', L.make_hmm_out, lambda nrows, nreads, nsites: _hmm_shapes(want, nrows, nreads, nsites), opts,
                       (cs, start, roff, score, key), hoff, device, site_pi)


VIT_OUTPUTS = L.VIT_ENTRY_FIELDS + L.VIT_READ_FIELDS + L.VIT_SITE_FIELDS


def _vit_opts(pi, length, want):
    """nmod_vit_opts from the Python arguments; ValueError for what the C entry refuses"""
    pi, length = _check_chain(pi, length)
    return L.make_vit_opts(pi, length), _check_want(want, VIT_OUTPUTS)


def _vit_shapes(want, nrows, nreads, nsites):
    kinds = dict(path=('uint8', nrows), site=('int32', nrows), delta=('float64', nrows), vit=('float64', nreads), status=('uint8', nreads),
                 **{k: ('int32', nreads) for k in ('n_sites', 'n_mod', 'n_runs')}, **{k: ('int32', nsites) for k in L.VIT_SITE_FIELDS})
    return {k: kinds[k] for k in VIT_OUTPUTS if k in want}


def read_viterbi_host(cs, start, roff, score, key, hoff=None, *, pi=0.5, length=200.0, want=VIT_OUTPUTS, device=0, site_pi=None):
    """Per-read Viterbi decoding of read_hmm_host's chain (nmod_read_viterbi, include/nanomod_hip.h) on host-resident reads: the
    arguments of read_hmm_host without call_post.  Returns a dict of numpy arrays, hoff and those named in `want`: per entry path (uint8,
    the state on the most probable path), site (int32, the index into key), delta (float64, the max-marginal margin of state 1 over
    state 0); per read n_sites, n_mod, n_runs (int32), vit (float64, the path's log-probability on ll's scale), status (uint8,
    L.HMM_NO_SITE); per site site_n, site_mod (int32)."""
    opts, want = _vit_opts(pi, length, want)
    return _chain_host('nmod_read_viterbi', L.make_vit_out, lambda nrows, nreads, nsites: _vit_shapes(want, nrows, nreads, nsites), opts,
                       (cs, start, roff, score, key), hoff, device, site_pi)


HMM_GRAD_OUTPUTS = L.HMM_GRAD_READ_FIELDS + ('sums',)


def _hmm_grad_opts(pi, length, want):
    """nmod_hmm_grad_opts from the Python arguments; ValueError for what the C entry refuses"""
    pi, length = _check_chain(pi, length)
    return L.make_hmm_grad_opts(pi, length), _check_want(want, HMM_GRAD_OUTPUTS)


def _hmm_grad_shapes(want, nreads):
    kinds = dict({k: ('float64', nreads) for k in L.HMM_GRAD_READ_FIELDS}, status=('uint8', nreads), sums=('float64', len(L.HMM_GRAD_SUMS)))
    return {k: kinds[k] for k in HMM_GRAD_OUTPUTS if k in want}


def read_hmm_grad_host(cs, start, roff, score, key, hoff=None, *, pi=0.5, length=200.0, want=HMM_GRAD_OUTPUTS, device=0, site_pi=None):
    """The log-likelihood of read_hmm_host's chain and its gradient in eta = logit(pi) and lam = ln(length) (nmod_read_hmm_grad,
    include/nanomod_hip.h) on host-resident reads: the arguments of read_hmm_host without call_post.  Returns a dict of numpy arrays, hoff
    and those named in `want`: per read ll (read_hmm_host's, bit for bit), g_eta, g_lam, abs_eta, abs_lam (float64), status (uint8,
    L.HMM_NO_SITE); sums (float64[8], L.HMM_GRAD_SUMS: the sums over the reads of ll, the gradient and its products, the reads with an
    entry and the entries) — what readllr.fit_hmm takes per evaluation.  With site_pi (nmod_read_hmm_grad_prior) g_eta is the derivative
    in a common logit offset of all shares, at the shares given."""
    opts, want = _hmm_grad_opts(pi, length, want)
    return _chain_host('nmod_read_hmm_grad', L.make_hmm_grad_out, lambda nrows, nreads, nsites: _hmm_grad_shapes(want, nreads), opts,
                       (cs, start, roff, score, key), hoff, device, site_pi)


CLASS_ROWS_OUTPUTS = L.CLASS_ROWS_FIELDS
CLASSES_OUTPUTS = L.CLASSES_READ_FIELDS + L.CLASSES_SITE_FIELDS + ('w_out', 'sums')
_CLASSES_LO, _CLASSES_HI = 1e-9, 1.0 - 1e-9


def _class_rows_shapes(nrows, nsites):
    return dict(site=('int32', nrows), s=('float64', nrows), rread=('int32', nrows), soff=('int64', nsites + 1), srow=('int32', nrows))


def _classes_opts(n_classes, want):
    """nmod_classes_opts from the Python arguments; ValueError for what the C entry refuses"""
    if int(n_classes) != n_classes or not 1 <= int(n_classes) <= L.CLASSES_MAX:
        raise ValueError('n_classes must be an integer in 1 .. %d, not %r' % (L.CLASSES_MAX, n_classes))
    return L.make_classes_opts(int(n_classes)), _check_want(want, CLASSES_OUTPUTS)


def _classes_shapes(want, nreads, nsites, nc):
    kinds = dict(gamma=('float64', nreads * nc), ll=('float64', nreads), cls=('int32', nreads), status=('uint8', nreads),
                 theta_out=('float64', nsites * nc), n_site=('float64', nsites * nc), w_out=('float64', nc), sums=('float64', 4 + nc))
    return {k: kinds[k] for k in CLASSES_OUTPUTS if k in want}


def _check_class_params(theta, w, nsites):
    """theta (float64[nsites, C] or flat) and w (float64[C]) of a host call, checked as the C entry checks them -> theta, w, C"""
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.ndim != 1 or not 1 <= w.shape[0] <= L.CLASSES_MAX:
        raise ValueError('w must hold 1 .. %d class weights' % L.CLASSES_MAX)
    nc = w.shape[0]
    theta = np.ascontiguousarray(theta, dtype=np.float64)
    if theta.size != nsites * nc:
        raise ValueError('theta must be float64[nsites * n_classes], the classes of a site contiguous')
    theta = theta.reshape(-1)
    if not bool(np.all((theta >= _CLASSES_LO) & (theta <= _CLASSES_HI))):
        raise ValueError('theta must lie in 1e-9 .. 1 - 1e-9')
    if not (bool(np.all((w >= _CLASSES_LO) & (w <= _CLASSES_HI))) or (nc == 1 and w[0] == 1.0)):
        raise ValueError('w must lie in 1e-9 .. 1 - 1e-9')
    if not abs(float(w.sum()) - 1.0) <= 1e-9:
        raise ValueError('w must sum to 1 within 1e-9')
    return theta, w, nc


def _check_class_offsets(off, n, nrows, name):
    off = _side(off, np.int64, n + 1, name, 'n + 1', optional=False)
    if off[0] != 0 or bool(np.any(np.diff(off) < 0)) or int(off[-1]) != nrows:
        raise ValueError('%s must start at 0, never decrease and end at nrows' % name)
    return off


def read_class_rows_host(cs, start, roff, score, key, hoff=None, *, want=CLASS_ROWS_OUTPUTS, device=0):
    """The rows of the latent-class fit (nmod_read_class_rows, include/nanomod_hip.h) on host-resident reads: the arguments of
    read_hmm_host.  Returns a dict of numpy arrays, hoff and those named in `want`: per row site (int32), s (float64, the read's
    window sum there) and rread (int32, the row's read); soff (int64[nsites + 1]) and srow (int32[nrows]): the rows of site j are
    srow[soff[j]:soff[j + 1]] in ascending row index."""
    want = _check_want(want, CLASS_ROWS_OUTPUTS)
    return _chain_host('nmod_read_class_rows', L.make_class_rows_out,
                       lambda nrows, nreads, nsites: {k: v for k, v in _class_rows_shapes(nrows, nsites).items() if k in want}, None,
                       (cs, start, roff, score, key), hoff, device)


def read_classes_step_host(rows, theta, w, *, want=CLASSES_OUTPUTS, device=0):
    """One EM step of the latent-class mixture over the reads (nmod_read_classes_step, include/nanomod_hip.h) on host-resident rows:
    `rows` as read_class_rows_host gives them (hoff, site, s, rread, soff, srow); theta float64[nsites, C] (the share of every class at
    every site, within 1e-9 .. 1 - 1e-9), w float64[C] (the class weights, summing to 1).  Returns a dict of numpy arrays, those named
    in `want`: per read gamma (float64[nreads * C]), ll (float64), cls (int32, -1 without an entry), status (uint8, L.HMM_NO_SITE);
    theta_out and n_site (float64[nsites * C]); w_out (float64[C]); sums (float64[4 + C], L.CLASSES_SUMS and the classes' sums of
    gamma)."""
    hoff = np.ascontiguousarray(rows['hoff'], dtype=np.int64)
    soff = np.ascontiguousarray(rows['soff'], dtype=np.int64)
    if hoff.ndim != 1 or hoff.shape[0] < 1 or soff.ndim != 1 or soff.shape[0] < 1:
        raise ValueError('hoff and soff must be int64 vectors of nreads + 1 and nsites + 1 offsets')
    nreads, nsites = hoff.shape[0] - 1, soff.shape[0] - 1
    theta, w, nc = _check_class_params(theta, w, nsites)
    opts, want = _classes_opts(nc, want)
    nrows = _check_hmm_counts(nreads, nsites, int(hoff[-1]))
    if nrows > 0 and (nreads == 0 or nsites == 0):
        raise ValueError('rows need reads and sites')
    hoff = _check_class_offsets(hoff, nreads, nrows, 'hoff')
    soff = _check_class_offsets(soff, nsites, nrows, 'soff')
    site = _side(rows['site'], np.int32, nrows, 'site', 'nrows', optional=False)
    s = _side(rows['s'], np.float64, nrows, 's', 'nrows', optional=False)
    rread = _side(rows['rread'], np.int32, nrows, 'rread', 'nrows', optional=False)
    srow = _side(rows['srow'], np.int32, nrows, 'srow', 'nrows', optional=False)
    lib = L.load()
    shapes = _classes_shapes(want, nreads, nsites, nc)
    res = _host_outputs(shapes, fill=shapes)
    _join_warm_up(device)
    out = L.make_classes_out(**_np_ptrs(res))
    prm = L.make_params(device=device, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    _call(lib, 'nmod_read_classes_step', prm, nreads, nsites, nrows, _np_ptr(hoff), _np_ptr(site), _np_ptr(s), _np_ptr(rread), _np_ptr(soff),
          _np_ptr(srow), C.byref(opts), _np_ptr(theta), _np_ptr(w), C.byref(out))
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
        self._kinds = {n: getattr(torch, n) for n in ('float64', 'float32', 'int64', 'int32', 'int16', 'uint8')}

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
        raise ValueError('signals must be %s' % _SIGNAL_DTYPES)

    @property
    def _dev(self):
        return 'cuda:%d' % self.device

    def _outputs(self, out, shapes, what, validate=True, zero=(), given=None):
        """The dict of output tensors for a table of outputs (_*_shapes): the caller's `out` as it is — checked against the table
        when `validate` (rescale_reads, read_calls, site_calls; mix, one_sample and kmer_model never checked theirs) — or fresh
        CUDA tensors, those named in `zero` zeroed, those in `given` taken from there instead."""
        torch, kind = self.torch, self._kinds.get                   # (a dtype name as torch's dtype, a dtype object as it is)
        if out is None:
            given = given or {}
            return {name: given[name] if name in given else (torch.zeros if name in zero else torch.empty)(n, dtype=kind(k, k), device=self._dev)
                    for name, (k, n) in shapes.items()}
        if validate:
            _cuda_vecs(what + ': out', ((name, out.get(name), kind(k, k), n) for name, (k, n) in shapes.items()), missing='refused')
        return out

    def workspace(self, prm, npos):
        need = self.lib.nmod_workspace_bytes(C.byref(prm), npos)
        if self._ws is None or self._ws.numel() < need:
            self._ws = self.torch.empty(need, dtype=self.torch.uint8, device=self._dev)
        return self._ws, need

    def alloc_outputs(self, npos):
        torch = self.torch
        dev = self._dev
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
        rc = self.lib.nmod_detect_batch(C.byref(prm), npos, _ptr(sig0), _ptr(off0), _ptr(sig1), _ptr(off1),
                                        _ptr(run_id), ws.data_ptr(), need, C.byref(o))
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
        _cuda_vecs('fdr', (('every track (all of one length)', t, torch.float64, ps[0].numel()) for t in ps), one_dim=True)
        n = ps[0].numel() if ps else 0
        qs = [out[name] if out is not None else torch.empty(n, dtype=torch.float64, device=self._dev) for name in tracks]
        nt = len(ps)
        summary = torch.empty((max(nt, 1), 4), dtype=torch.float64, device=self._dev)
        parr = (C.c_void_p * max(nt, 1))(*[t.data_ptr() for t in ps])
        qarr = (C.c_void_p * max(nt, 1))(*[t.data_ptr() for t in qs])
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        _call(self.lib, 'nmod_fdr_adjust', prm, n, nt, parr, _fdr_method(method), float(alpha), qarr, summary.data_ptr())
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
        mix_group, model, max_iter, tol = _mix_args(mix_group, model, max_iter, tol)
        dtype = self._dtype_of(sig0)
        if self._dtype_of(sig1) != dtype:
            raise ValueError('sig0 and sig1 must share a dtype')
        if npos is None:
            npos = (off0.numel() - 1) if off0 is not None else ((off1.numel() - 1) if off1 is not None else sig0.numel() // stride0)
        _cuda_vecs('mix', (('gate', gate, self.torch.float64, npos),), missing='ok')
        shapes = _mix_shapes(npos, (sig1 if mix_group == 1 else sig0).numel() if want_resp else None)
        res = self._outputs(out, shapes, 'mix', validate=False)
        o = L.make_out(L.NmodMixOut, **{k: t.data_ptr() for k, t in res.items()})
        prm = self._params(dtype, stride0 if off0 is None else 0, stride1 if off1 is None else 0, 0, 0)
        _call(self.lib, 'nmod_mix_fraction', prm, npos, _ptr(sig0), _ptr(off0), _ptr(sig1), _ptr(off1), mix_group, model, max_iter, tol,
              _ptr(gate), float(gate_max), C.byref(o))
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
        _cuda_vecs('one_sample', (('ref_mean', ref_mean, torch.float64, npos), ('ref_sd', ref_sd, torch.float64, npos),
                                  ('ref_n', ref_n, torch.int32, npos), ('run_id', run_id, torch.int32, npos),
                                  ('off', off, torch.int64, npos + 1)), missing='ok')
        if self.method != L.METHOD_KS and run_id is None:
            raise ValueError('one_sample: run_id is needed for the combined track')
        res = self._outputs(out, _one_shapes(self.method, npos), 'one_sample', validate=False)
        o = L.make_out(L.NmodOneOut, **{k: t.data_ptr() for k, t in res.items()})
        prm = self._params(dtype, stride if off is None else 0, 0, 0, 0)
        _call(self.lib, 'nmod_one_sample', prm, npos, _ptr(sig), _ptr(off), _ptr(ref_mean), _ptr(ref_sd), _ptr(ref_n), _ptr(run_id), C.byref(o))
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
        _cuda_vecs('kmer_model', (('code', code, torch.int32, npos), ('off', off, torch.int64, npos + 1), ('keep_lo', keep_lo, torch.float64, ncodes),
                                  ('keep_hi', keep_hi, torch.float64, ncodes)), missing='ok')
        res = self._outputs(out, _kmer_shapes(npos, ncodes), 'kmer_model', validate=False)
        o = L.make_out(L.NmodKmerOut, **{k: t.data_ptr() for k, t in res.items()})
        prm = self._params(dtype, stride if off is None else 0, 0, 0, 0)
        _call(self.lib, 'nmod_kmer_model', prm, npos, _ptr(sig), _ptr(off), _ptr(code), ncodes, _ptr(keep_lo), _ptr(keep_hi), C.byref(o))
        return res

    def kmer_mix(self, sig, code, ncodes, mean0, sd0, *, off=None, stride=0, npos=None, model='free', max_iter=200, tol=1e-6, min_samples=2,
                 want_hist=False, out=None):
        """The modified component per k-mer code (nmod_kmer_mix, NMOD_MEM_DEVICE), enqueued on the current stream without
        synchronising.  sig: float32, int16 or float64 CUDA rows by `off` (int64 CUDA tensor) or a fixed `stride`; code: int32 CUDA
        vector (a value outside [0, ncodes): the position takes no part, L.STATUS_NO_CODE); mean0 / sd0: float64 CUDA vectors of
        ncodes, the unmodified component.  Returns a dict of CUDA tensors: n_positions, n_used, n_outside (int64), pi, mu_mod, sd_mod,
        llr (float64; a score, not a test), iters (int32), status (uint8, L.KMIX_* bits), each of ncodes, pos_status (uint8, npos) and
        with want_hist `hist` (int32 holding the uint32 counts, ncodes * L.KMIX_BINS).  int16 is the tuned form."""
        torch = self.torch
        opts = _kmix_opts(model, max_iter, tol, min_samples)
        dtype = self._dtype_of(sig)
        if npos is None:
            npos = code.numel()
        ncodes = int(ncodes)
        _cuda_vecs('kmer_mix', (('code', code, torch.int32, npos), ('mean0', mean0, torch.float64, ncodes), ('sd0', sd0, torch.float64, ncodes)),
                   missing='refused')
        _cuda_vecs('kmer_mix', (('off', off, torch.int64, npos + 1),), missing='ok')
        res = self._outputs(out, _kmix_shapes(npos, ncodes, 'int32' if want_hist else False), 'kmer_mix', validate=False)
        o = L.make_out(L.NmodKmixOut, **{k: t.data_ptr() for k, t in res.items()})
        prm = self._params(dtype, stride if off is None else 0, 0, 0, 0)
        _call(self.lib, 'nmod_kmer_mix', prm, npos, _ptr(sig), _ptr(off), _ptr(code), ncodes, _ptr(mean0), _ptr(sd0), C.byref(opts), C.byref(o))
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
        nreads = _device_offsets(torch, off, 'rescale_reads', 'nreads')
        if fit:
            m = _device_model(torch, 'rescale_reads', val, base, mean, sd, k, center, one_dim=False)
        else:
            m = L.NmodRescaleModel()
            _cuda_vecs('rescale_reads', (('val', val, None, None), ('shift', shift, torch.float64, nreads), ('scale', scale, torch.float64, nreads)),
                       missing='refused')
        given = {}
        if out is None:                                             # what is not allocated: the caller's pairs, val itself in place
            if not fit:
                given.update(shift=shift, scale=scale)
            if apply:
                given['val'] = val if inplace else torch.empty_like(val)
        res = self._outputs(out, _rescale_shapes(nreads, val.dtype if apply else None, val.numel()), 'rescale_reads',
                            zero=('n_used', 'status'), given=given)
        o = L.make_out(L.NmodRescaleOut, shift=res['shift'].data_ptr(), scale=res['scale'].data_ptr(), n_used=res['n_used'].data_ptr(),
                       status=res['status'].data_ptr(), val_out=_ptr(res['val'] if apply else None))
        prm = self._params(dtype, 0, 0, 0, 0)
        _call(self.lib, 'nmod_rescale_reads', prm, nreads, off.data_ptr(), val.data_ptr(), _ptr(base) if fit else None, C.byref(m),
              C.byref(opts), C.byref(o))
        return res

    def read_calls(self, val, off, base, mean, sd, k, center, *, nb=2, alpha=0.01, want=('z', 'p', 'p_win'), out=None):
        """Per-read modification calls against a k-mer model (nmod_read_calls, NMOD_MEM_DEVICE), enqueued on the current stream without
        synchronising or reading anything back.  val: float32, int16 or float64 CUDA vector of events (the `val` of rescale_reads, say),
        base: uint8 CUDA vector (one byte per event), off: int64 CUDA vector of nreads + 1 event offsets; mean / sd: float64 CUDA
        vectors of 4^k model entries.  Returns a dict of CUDA tensors: the per-event tracks named in `want` (float64: z, p, p_win) and per
        read n_sites, n_called (int32) and status (uint8).  p_win is what pivot_reads' device form takes as `val` for site_calls.
        out: such a dict from an earlier call of the same shape, written again instead of allocating (a timing loop)."""
        dtype = self._dtype_of(val)
        opts, want = _calls_opts(nb, alpha, k, center, want)
        nreads = _device_offsets(self.torch, off, 'read_calls', 'nreads')
        md = _device_model(self.torch, 'read_calls', val, base, mean, sd, k, center, one_dim=True)
        shapes = _calls_shapes(want, val.numel(), nreads)
        res = self._outputs(out, shapes, 'read_calls')
        o = L.make_out(L.NmodCallsOut, **{name: res[name].data_ptr() for name in shapes})
        prm = self._params(dtype, 0, 0, 0, 0)
        _call(self.lib, 'nmod_read_calls', prm, nreads, off.data_ptr(), val.data_ptr(), base.data_ptr(), C.byref(md), C.byref(opts), C.byref(o))
        return res

    def site_calls(self, score, *, off=None, stride=0, npos=None, alpha=0.01, out=None):
        """Per-position call counts over pivoted scores (nmod_site_calls, NMOD_MEM_DEVICE) on the current stream: score a float64 CUDA
        vector, rows by `off` (int64 CUDA vector) or a fixed `stride`.  Returns a dict of CUDA tensors n_valid, n_called (int32) and
        frac (float64)."""
        alpha = _check_alpha(alpha)
        stride, npos = self._score_rows('site_calls', score, off, stride, npos)
        shapes = _site_shapes(npos)
        res = self._outputs(out, shapes, 'site_calls')
        o = L.make_out(L.NmodSiteOut, **{name: res[name].data_ptr() for name in shapes})
        prm = self._params(L.DTYPE_F64, stride if off is None else 0, 0, 0, 0)
        _call(self.lib, 'nmod_site_calls', prm, npos, score.data_ptr(), _ptr(off), alpha, C.byref(o))
        return res

    def _score_rows(self, what, score, off, stride, npos):
        """the rows of a float64 CUDA vector of pivoted scores, by `off` or a fixed `stride`: (stride, npos), checked"""
        _cuda_vecs(what, (('score', score, self.torch.float64, None),), one_dim=True)
        if off is not None:
            return stride, _device_offsets(self.torch, off, what, 'npos')
        stride = int(stride)
        if stride <= 0:
            raise ValueError('%s: either off or a positive stride' % what)
        if npos is None:
            npos = score.numel() // stride
        if npos * stride > score.numel():
            raise ValueError('%s: score is shorter than npos rows of the stride' % what)
        return stride, npos

    def read_llr(self, val, off, base, mean, sd, alt_mean, alt_sd, k, center, *, window='kmer', thr=2.5, prior_logit=0.0,
                 want=('llr', 'llr_win', 'p_mod'), out=None):
        """Per-read log-likelihood ratios between two k-mer models (nmod_read_llr, NMOD_MEM_DEVICE), enqueued on the current stream
        without synchronising or reading anything back.  val, off, base as for read_calls; mean / sd (unmodified) and alt_mean / alt_sd
        (modified): float64 CUDA vectors of 4^k entries each; window: 'kmer' or (lo, hi).  Returns a dict of CUDA tensors: the per-event
        tracks named in `want` (float64: llr, llr_win, p_mod) and per read n_sites, n_mod, n_can (int32) and status (uint8).  llr_win is
        what pivot_reads' device form takes as `val` for site_llr.  out: such a dict from an earlier call of the same shape."""
        dtype = self._dtype_of(val)
        opts, want = _llr_opts(window, thr, prior_logit, k, center, k, center, want)
        nreads = _device_offsets(self.torch, off, 'read_llr', 'nreads')
        m0 = _device_model(self.torch, 'read_llr', val, base, mean, sd, k, center, one_dim=True)
        m1 = _device_model(self.torch, 'read_llr', val, base, alt_mean, alt_sd, k, center, one_dim=True)
        shapes = _llr_shapes(want, val.numel(), nreads)
        res = self._outputs(out, shapes, 'read_llr')
        o = L.make_out(L.NmodLlrOut, **{name: res[name].data_ptr() for name in shapes})
        prm = self._params(dtype, 0, 0, 0, 0)
        _call(self.lib, 'nmod_read_llr', prm, nreads, off.data_ptr(), val.data_ptr(), base.data_ptr(), C.byref(m0), C.byref(m1), C.byref(opts),
              C.byref(o))
        return res

    def site_llr(self, score, *, off=None, stride=0, npos=None, thr=2.5, out=None):
        """Per-position counts over pivoted window sums (nmod_site_llr, NMOD_MEM_DEVICE) on the current stream: score a float64 CUDA
        vector, rows by `off` (int64 CUDA vector) or a fixed `stride`.  Returns a dict of CUDA tensors n_valid, n_mod, n_can (int32) and
        frac (float64)."""
        thr = _check_thr(thr)
        stride, npos = self._score_rows('site_llr', score, off, stride, npos)
        shapes = _site_llr_shapes(npos)
        res = self._outputs(out, shapes, 'site_llr')
        o = L.make_out(L.NmodSiteLlrOut, **{name: res[name].data_ptr() for name in shapes})
        prm = self._params(L.DTYPE_F64, stride if off is None else 0, 0, 0, 0)
        _call(self.lib, 'nmod_site_llr', prm, npos, score.data_ptr(), _ptr(off), thr, C.byref(o))
        return res

    def site_stoich(self, score, *, off=None, stride=0, npos=None, min_valid=3, ci_level=0.95, max_iter=60, tol=1e-12, resp=False, out=None):
        """Per-position modified fraction by maximum likelihood over pivoted window sums (nmod_site_stoich, NMOD_MEM_DEVICE) on the
        current stream, nothing read back: score a float64 CUDA vector, rows by `off` (int64 CUDA vector) or a fixed `stride`.  Returns
        a dict of CUDA tensors pi, pi_lo, pi_hi, stat, p_null (float64), n_valid, iters (int32), status (uint8, L.STOICH_* bits) and
        with `resp` the posterior of every read (float64, in the score layout; a score outside every row keeps NaN).  p_null is a
        track fdr() takes as it is:

            st = det.site_stoich(piv['sig'], off=piv['off'])
            (q,), summary = det.fdr(st, tracks=('p_null',))
        """
        opts = _stoich_opts(min_valid, ci_level, max_iter, tol)
        stride, npos = self._score_rows('site_stoich', score, off, stride, npos)
        shapes = _stoich_shapes(npos, score.numel() if resp else None)
        given = {'resp': self.torch.full((score.numel(),), float('nan'), dtype=self.torch.float64, device=self._dev)} if resp and out is None else None
        res = self._outputs(out, shapes, 'site_stoich', given=given)
        o = L.make_out(L.NmodStoichOut, **{name: res[name].data_ptr() for name in shapes})
        prm = self._params(L.DTYPE_F64, stride if off is None else 0, 0, 0, 0)
        _call(self.lib, 'nmod_site_stoich', prm, npos, score.data_ptr(), _ptr(off), C.byref(opts), C.byref(o))
        return res

    def read_llr_multi(self, val, off, base, mean, sd, alt_means, alt_sds, k, center, *, window='kmer', thr=2.5, prior_logit=None,
                       want=('llr', 'llr_win', 'post', 'call'), out=None):
        """Per-read log-likelihood ratios against several modified k-mer models in one walk (nmod_read_llr_multi, NMOD_MEM_DEVICE),
        enqueued on the current stream without synchronising or reading anything back.  val, off, base, mean, sd as for read_llr;
        alt_means / alt_sds: 1 .. L.MULTI_MAX float64 CUDA vectors of 4^k entries each.  Returns a dict of CUDA tensors: the tracks
        named in `want` — llr, llr_win (float64[n_alt, events]; row m - 1 holds read_llr's bits for alt m - 1 and is what pivot_reads'
        device form takes as `val`), post (float64[n_alt + 1, events]), call (uint8) — and per read n_sites, n_can (int32), n_mod
        (int32[n_alt, nreads]) and status (uint8).  Events outside every read keep what the tensors held (NaN / L.MULTI_NONE when they
        are allocated here).  out: such a dict from an earlier call of the same shape."""
        torch = self.torch
        dtype = self._dtype_of(val)
        alt_means, alt_sds = list(alt_means), list(alt_sds)
        if len(alt_means) != len(alt_sds):
            raise ValueError('read_llr_multi: one alt_sd per alt_mean')
        opts, want = _llr_multi_opts(window, thr, prior_logit, k, center, [(k, center)] * len(alt_means), want)
        n_alt = len(alt_means)
        nreads = _device_offsets(torch, off, 'read_llr_multi', 'nreads')
        m0 = _device_model(torch, 'read_llr_multi', val, base, mean, sd, k, center, one_dim=True)
        ms = [_device_model(torch, 'read_llr_multi', val, base, am, asd, k, center, one_dim=True) for am, asd in zip(alt_means, alt_sds)]
        arr = L.model_ptr_array(ms)
        nval = val.numel()
        shapes = _llr_multi_shapes(want, nval, nreads, n_alt)
        given = None
        if out is None:
            given = {w: torch.full((shapes[w][1],), L.MULTI_NONE if w == 'call' else float('nan'), dtype=self._kinds[shapes[w][0]], device=self._dev)
                     for w in want}
        res = self._outputs({name: t.reshape(-1) for name, t in out.items()} if out is not None else None, shapes, 'read_llr_multi', given=given)
        o = L.make_out(L.NmodLlrMultiOut, **{name: res[name].data_ptr() for name in shapes})
        prm = self._params(dtype, 0, 0, 0, 0)
        _call(self.lib, 'nmod_read_llr_multi', prm, nreads, nval, off.data_ptr(), val.data_ptr(), base.data_ptr(), C.byref(m0), n_alt,
              C.addressof(arr), C.byref(opts), C.byref(o))
        return out if out is not None else _llr_multi_views(res, nval, nreads, n_alt)

    def site_compose(self, scores, *, off=None, stride=0, npos=None, min_valid=3, max_iter=500, tol=1e-9, test=True, resp=False, out=None):
        """The shares of all states per position by maximum likelihood (nmod_site_compose, NMOD_MEM_DEVICE) on the current stream,
        nothing read back: scores: 1 .. L.MULTI_MAX float64 CUDA vectors of one length (the pivoted llr_win planes of read_llr_multi),
        rows by the one `off` (int64 CUDA vector) or a fixed `stride`.  Returns a dict of CUDA tensors pi (float64[n_alt + 1, npos]),
        ll, stat, with `test` stat_m and p_m (float64[n_alt, npos]), n_valid, n_partial, iters (int32), open_mask, status (uint8,
        L.COMPOSE_* bits) and with `resp` the responsibilities (float64[n_alt + 1, scores]; a score outside every row keeps NaN).  A row
        of p_m is a track fdr() takes."""
        torch = self.torch
        scores = list(scores)
        opts = _compose_opts(len(scores), min_valid, max_iter, tol)
        n_alt = len(scores)
        for s in scores:
            stride, n = self._score_rows('site_compose', s, off, stride, npos)
            if s.numel() != scores[0].numel():
                raise ValueError('site_compose: the scores of all states must have one length')
        npos, total = n, scores[0].numel()
        shapes = _compose_shapes(npos, n_alt, test, total if resp else None)
        given = {'resp': torch.full((shapes['resp'][1],), float('nan'), dtype=torch.float64, device=self._dev)} if resp and out is None else None
        res = self._outputs({name: t.reshape(-1) for name, t in out.items()} if out is not None else None, shapes, 'site_compose', given=given)
        o = L.make_out(L.NmodComposeOut, **{name: res[name].data_ptr() for name in shapes})
        ptrs = (C.c_void_p * n_alt)(*[s.data_ptr() for s in scores])
        prm = self._params(L.DTYPE_F64, stride if off is None else 0, 0, 0, 0)
        _call(self.lib, 'nmod_site_compose', prm, npos, total, n_alt, C.addressof(ptrs), _ptr(off), C.byref(opts), C.byref(o))
        return out if out is not None else _compose_views(res, npos, n_alt)

    def site_diff(self, score0, score1, *, off0=None, off1=None, stride0=0, stride1=0, npos=None, min_valid=3, ci_level=0.95, max_iter=60,
                  tol=1e-12, interval=True, out=None):
        """The modified shares of two samples compared per site (nmod_site_diff, NMOD_MEM_DEVICE) on the current stream, nothing read
        back: score0 / score1 float64 CUDA vectors, the rows of each by its `off` (int64 CUDA vector) or fixed stride, the same sites
        in the same order (engine.match_score_rows makes them).  Returns a dict of CUDA tensors pi0, pi1, pi_pool, delta, with
        `interval` delta_lo and delta_hi, stat, p_diff (float64), n_valid0, n_valid1, iters (int32) and status (uint8, L.DIFF_*
        bits).  p_diff is a track fdr() takes as it is."""
        opts = _diff_opts(min_valid, ci_level, max_iter, tol)
        stride0, npos0 = self._score_rows('site_diff', score0, off0, stride0, npos)
        stride1, npos1 = self._score_rows('site_diff', score1, off1, stride1, npos)
        if npos0 != npos1:
            raise ValueError('site_diff: the two samples must hold the same sites: %d rows against %d' % (npos0, npos1))
        shapes = _diff_shapes(npos0, interval)
        res = self._outputs(out, shapes, 'site_diff')
        o = L.make_out(L.NmodDiffOut, **{name: res[name].data_ptr() for name in shapes})
        prm = self._params(L.DTYPE_F64, stride0 if off0 is None else 0, stride1 if off1 is None else 0, 0, 0)
        _call(self.lib, 'nmod_site_diff', prm, npos0, score0.data_ptr(), _ptr(off0), score1.data_ptr(), _ptr(off1), C.byref(opts), C.byref(o))
        return res

    def rep_prior(self, phi, status, df, *, ci_level=0.95, out=None):
        """The prior law of site_diff_rep's dispersions (nmod_rep_prior, NMOD_MEM_DEVICE) on the current stream, nothing read back: phi
        a float64 and status a uint8 CUDA vector of one length, as site_diff_rep returned them.  Returns the record, a float64 CUDA
        vector of L.REP_PRIOR_WORDS (`out` if given), which site_diff_rep(prior=) reads on the device."""
        torch = self.torch
        df, ci_level = _rep_prior_args(df, ci_level)
        _cuda_vecs('rep_prior', (('phi', phi, torch.float64, None), ('status', status, torch.uint8, phi.numel())), one_dim=True)
        if out is None:
            out = torch.empty(L.REP_PRIOR_WORDS, dtype=torch.float64, device=self._dev)
        else:
            _cuda_vecs('rep_prior: out', (('out', out, torch.float64, L.REP_PRIOR_WORDS),), one_dim=True)
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        _call(self.lib, 'nmod_rep_prior', prm, phi.numel(), df, phi.data_ptr(), status.data_ptr(), ci_level, out.data_ptr())
        return out

    def site_diff_rep(self, score, off, n_samples, n_control, *, min_valid=3, ci_level=0.95, phi_floor=0.0, max_iter=60, tol=1e-12,
                      interval=True, prior=None, out=None):
        """The modified shares of two replicated conditions compared per site (nmod_site_diff_rep, NMOD_MEM_DEVICE) on the current
        stream, nothing read back: score a float64 CUDA vector, off an int64 CUDA vector of npos * n_samples + 1 offsets, row
        i * n_samples + g for site i and sample g, the first n_control samples condition 0 (engine.match_score_rows_multi makes them).
        Returns a dict of CUDA tensors as site_diff_rep_host's arrays.  p_rep, p_cond and p_het are tracks fdr() takes as they are.
        prior: the record rep_prior() left on the device (nmod_site_diff_rep_mod: the result gains phi_post); the kernels read it, the
        host never does."""
        opts, n_samples, n_control = _rep_opts(n_samples, n_control, min_valid, ci_level, phi_floor, max_iter, tol)
        _cuda_vecs('site_diff_rep', (('score', score, self.torch.float64, None),), one_dim=True)
        if prior is not None:
            _cuda_vecs('site_diff_rep', (('prior', prior, self.torch.float64, L.REP_PRIOR_WORDS),), one_dim=True)
        npos = _rep_npos(_device_offsets(self.torch, off, 'site_diff_rep', 'npos * n_samples'), n_samples, 'site_diff_rep')
        shapes = _rep_shapes(npos, n_samples, interval, moderated=prior is not None)
        res = self._outputs(out, shapes, 'site_diff_rep')
        o = L.make_out(L.NmodRepOut, **{name: res[name].data_ptr() for name in shapes if name != 'phi_post'})
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        if prior is None:
            _call(self.lib, 'nmod_site_diff_rep', prm, npos, n_samples, n_control, score.data_ptr(), off.data_ptr(), C.byref(opts), C.byref(o))
        else:
            _call(self.lib, 'nmod_site_diff_rep_mod', prm, npos, n_samples, n_control, score.data_ptr(), off.data_ptr(), C.byref(opts), C.byref(o),
                  prior.data_ptr(), res['phi_post'].data_ptr())
        return res

    def pair_index(self, key, max_dist=100):
        """The pairs of candidate sites at most max_dist apart on one (chrom, strand) (nmod_pair_index, NMOD_MEM_DEVICE) on the current
        stream: key an int64 CUDA vector of cs << 40 | pos, strictly ascending (not checked).  Synchronises the stream once to learn
        the number of pairs.  Returns (poff, npairs): poff an int64 CUDA vector of nsites + 1 offsets."""
        torch = self.torch
        max_dist = _check_max_dist(max_dist)
        _cuda_vecs('pair_index', (('key', key, torch.int64, None),), one_dim=True)
        _check_pair_counts(0, key.numel(), 0)
        poff = torch.empty(key.numel() + 1, dtype=torch.int64, device=self._dev)
        npairs = C.c_int64(0)
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        _call(self.lib, 'nmod_pair_index', prm, key.numel(), key.data_ptr(), max_dist, poff.data_ptr(), C.byref(npairs))
        return poff, int(npairs.value)

    def site_pairs(self, cs, start, roff, score, key, poff, npairs, *, thr=2.5, min_reads=10, force_direct=False, want=PAIRS_OUTPUTS,
                   out=None):
        """Same-read co-occurrence of calls at pairs of sites (nmod_site_pairs, NMOD_MEM_DEVICE), enqueued on the current stream without
        synchronising or reading anything back.  cs (int32), start (int64), roff (int64, nreads + 1) and score (float64, one per event:
        read_llr's llr_win) are CUDA vectors in pivot_reads' layout of the reads; key, poff and npairs as pair_index gives them.
        Returns a dict of CUDA tensors, those named in `want`: counts (int32, 4 per pair: n00, n01, n10, n11), first, second (int32),
        log_or, se, phi, p_fisher (float64), status (uint8, L.PAIRS_* bits).  p_fisher is a track fdr() takes as it is.  out: such a
        dict from an earlier call of the same shape."""
        torch = self.torch
        opts, want = _pairs_opts(thr, min_reads, force_direct, want)
        nreads = _device_offsets(torch, roff, 'site_pairs', 'nreads')
        _cuda_vecs('site_pairs', (('cs', cs, torch.int32, nreads), ('start', start, torch.int64, nreads), ('score', score, torch.float64, None),
                                  ('key', key, torch.int64, None), ('poff', poff, torch.int64, key.numel() + 1 if key is not None else None)),
                   one_dim=True, missing='refused')
        npairs = _check_pair_counts(nreads, key.numel(), npairs)
        shapes = _pairs_shapes(want, npairs)
        res = self._outputs(out, shapes, 'site_pairs')
        o = L.make_pairs_out(**{name: res[name].data_ptr() for name in shapes})
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        _call(self.lib, 'nmod_site_pairs', prm, nreads, cs.data_ptr(), start.data_ptr(), roff.data_ptr(), score.data_ptr(), key.numel(),
              key.data_ptr(), poff.data_ptr(), npairs, C.byref(opts), C.byref(o))
        return res

    def pair_rows(self, cs, start, roff, score, key, poff, npairs):
        """Per pair of sites the reads with a valid score at both (nmod_pair_rows_count, nmod_pair_rows_fill, NMOD_MEM_DEVICE) on the
        current stream: the arguments of site_pairs.  Synchronises the stream once to learn the number of rows.  Returns a dict of CUDA
        tensors: prow_off (int64, npairs + 1) and, per row, sa, sb (float64) and read (int32); within a pair the rows are in ascending
        read index."""
        torch = self.torch
        nreads = _device_offsets(torch, roff, 'pair_rows', 'nreads')
        _cuda_vecs('pair_rows', (('cs', cs, torch.int32, nreads), ('start', start, torch.int64, nreads), ('score', score, torch.float64, None),
                                 ('key', key, torch.int64, None), ('poff', poff, torch.int64, key.numel() + 1 if key is not None else None)),
                   one_dim=True, missing='refused')
        npairs = _check_pair_counts(nreads, key.numel(), npairs)
        prow_off = torch.empty(npairs + 1, dtype=torch.int64, device=self._dev)
        nrows = C.c_int64(0)
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        shared = (prm, nreads, cs.data_ptr(), start.data_ptr(), roff.data_ptr(), score.data_ptr(), key.numel(), key.data_ptr(), poff.data_ptr(), npairs)
        _call(self.lib, 'nmod_pair_rows_count', *shared, prow_off.data_ptr(), C.byref(nrows))
        n = int(nrows.value)
        # (a tensor of no elements has no address: one spare row keeps the pointers real)
        sa, sb = (torch.empty(n + 1, dtype=torch.float64, device=self._dev)[:n] for _ in range(2))
        read = torch.empty(n + 1, dtype=torch.int32, device=self._dev)[:n]
        _call(self.lib, 'nmod_pair_rows_fill', *shared, prow_off.data_ptr(), n, sa.data_ptr(), sb.data_ptr(), read.data_ptr())
        return dict(prow_off=prow_off, sa=sa, sb=sb, read=read)

    def pair_linkage(self, sa, sb, prow_off, *, min_reads=20, ci_level=0.95, max_iter=60, tol=1e-12, interval=True, out=None):
        """Soft same-read linkage of pairs of sites (nmod_pair_linkage, NMOD_MEM_DEVICE), enqueued on the current stream without
        synchronising or reading anything back: sa, sb (float64) and prow_off (int64, npairs + 1) CUDA vectors as pair_rows gives
        them.  Returns a dict of CUDA tensors pa, pb, d, with `interval` d_lo and d_hi, r, stat, p_indep (float64), n_valid, iters
        (int32) and status (uint8, L.LINK_* bits).  p_indep is a track fdr() takes as it is."""
        torch = self.torch
        opts = _link_opts(min_reads, ci_level, max_iter, tol)
        npairs = _device_offsets(torch, prow_off, 'pair_linkage', 'npairs')
        _cuda_vecs('pair_linkage', (('sa', sa, torch.float64, None), ('sb', sb, torch.float64, sa.numel() if sa is not None else None)),
                   one_dim=True, missing='refused')
        if npairs > 2 ** 31 - 2:
            raise ValueError('pair_linkage: at most 2^31 - 2 pairs')
        shapes = _link_shapes(npairs, interval)
        res = self._outputs(out, shapes, 'pair_linkage')
        o = L.make_link_out(**{name: res[name].data_ptr() for name in shapes})
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        _call(self.lib, 'nmod_pair_linkage', prm, npairs, sa.data_ptr(), sb.data_ptr(), prow_off.data_ptr(), C.byref(opts), C.byref(o))
        return res

    def _site_reads(self, what, cs, start, roff, score, key):
        """the reads and sites of a device entry that walks the reads over candidate sites without a pair index, checked"""
        torch = self.torch
        nreads = _device_offsets(torch, roff, what, 'nreads')
        _cuda_vecs(what, (('cs', cs, torch.int32, nreads), ('start', start, torch.int64, nreads), ('score', score, torch.float64, None),
                          ('key', key, torch.int64, None)), one_dim=True, missing='refused')
        return nreads, (nreads, cs.data_ptr(), start.data_ptr(), roff.data_ptr(), score.data_ptr(), key.numel(), key.data_ptr())

    def read_sites(self, cs, start, roff, score, key):
        """Per read the candidate sites it covers with a valid score, counted (nmod_read_sites_count, NMOD_MEM_DEVICE) on the current
        stream: the reads, scores and keys of site_pairs.  Synchronises the stream once to learn the number of rows.  Returns
        (hoff, nrows): hoff an int64 CUDA vector of nreads + 1 offsets."""
        nreads, shared = self._site_reads('read_sites', cs, start, roff, score, key)
        _check_hmm_counts(nreads, key.numel(), 0)
        hoff = self.torch.empty(nreads + 1, dtype=self.torch.int64, device=self._dev)
        nrows = C.c_int64(0)
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        _call(self.lib, 'nmod_read_sites_count', prm, *shared, hoff.data_ptr(), C.byref(nrows))
        return hoff, int(nrows.value)

    def _chain(self, what, make_out, shapes, opts, reads, hoff, nrows, out, site_pi=None):
        """What the device methods of the chain entries (K19 .. K22) share after the checks of their own arguments: _chain_host's
        arguments, `what` the method's name (the entry is nmod_<what>, nmod_<what>_prior with site_pi: a float64 CUDA vector of
        nsites shares), hoff and nrows as read_sites gives them, out the caller's."""
        nreads, shared = self._site_reads(what, *reads)
        _cuda_vecs(what, (('hoff', hoff, self.torch.int64, nreads + 1),), one_dim=True, missing='refused')
        nsites = reads[4].numel()
        if site_pi is not None:
            if not hasattr(site_pi, 'is_cuda'):
                raise ValueError('%s: site_pi must be a contiguous torch.float64 CUDA vector of %d elements' % (what, nsites))
            _cuda_vecs(what, (('site_pi', site_pi, self.torch.float64, nsites),), one_dim=True)
            if site_pi.device != reads[4].device:
                raise ValueError('%s: site_pi must live on the device of the reads' % what)
        nrows = _check_hmm_counts(nreads, nsites, nrows)
        shapes = shapes(nrows, nreads, nsites)
        res = self._outputs(out, shapes, what)
        o = make_out(**{name: res[name].data_ptr() for name in shapes})
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        prior = () if site_pi is None else (site_pi.data_ptr(),)
        _call(self.lib, 'nmod_' + what + ('_prior' if prior else ''), prm, *shared, *prior, hoff.data_ptr(), nrows,
              *(() if opts is None else (C.byref(opts),)), C.byref(o))
        return res

    def read_hmm(self, cs, start, roff, score, key, hoff, nrows, *, pi=0.5, length=200.0, call_post=0.9, want=HMM_OUTPUTS, out=None,
                 site_pi=None):
        """Per-read two-state HMM smoothing of the window sums at candidate sites (nmod_read_hmm, NMOD_MEM_DEVICE), enqueued on the
        current stream without synchronising or reading anything back: the arguments of read_sites, hoff and nrows as it gives them.
        Returns a dict of CUDA tensors, those named in `want`: per entry post (float64), site (int32), state (uint8); per read n_sites,
        n_mod, n_can, n_runs (int32), ll, ll_indep (float64), status (uint8, L.HMM_NO_SITE); per site site_n, site_mod, site_can
        (int32).  out: such a dict from an earlier call of the same shape.  site_pi: None, or a float64 CUDA vector of one share per
        candidate site (nmod_read_hmm_prior, K23; read_viterbi and read_hmm_grad take it in the same way)."""
        opts, want = _hmm_opts(pi, length, call_post, want)
        return self._chain('read_hmm', L.make_hmm_out, lambda nrows, nreads, nsites: _hmm_shapes(want, nrows, nreads, nsites), opts,
                           (cs, start, roff, score, key), hoff, nrows, out, site_pi)

    def read_viterbi(self, cs, start, roff, score, key, hoff, nrows, *, pi=0.5, length=200.0, want=VIT_OUTPUTS, out=None, site_pi=None):
        """Per-read Viterbi decoding of read_hmm's chain (nmod_read_viterbi, NMOD_MEM_DEVICE), enqueued on the current stream without
        synchronising or reading anything back: the arguments of read_hmm without call_post.  Returns a dict of CUDA tensors, those
        named in `want`: per entry path (uint8), site (int32), delta (float64); per read n_sites, n_mod, n_runs (int32), vit (float64),
        status (uint8, L.HMM_NO_SITE); per site site_n, site_mod (int32).  out: such a dict from an earlier call of the same shape."""
        opts, want = _vit_opts(pi, length, want)
        return self._chain('read_viterbi', L.make_vit_out, lambda nrows, nreads, nsites: _vit_shapes(want, nrows, nreads, nsites), opts,
                           (cs, start, roff, score, key), hoff, nrows, out, site_pi)

    def read_hmm_grad(self, cs, start, roff, score, key, hoff, nrows, *, pi=0.5, length=200.0, want=HMM_GRAD_OUTPUTS, out=None, site_pi=None):
        """The log-likelihood of read_hmm's chain and its gradient in logit(pi) and ln(length) (nmod_read_hmm_grad, NMOD_MEM_DEVICE),
        enqueued on the current stream without synchronising or reading anything back: the arguments of read_hmm without call_post.
        Returns a dict of CUDA tensors, those named in `want`: per read ll, g_eta, g_lam, abs_eta, abs_lam (float64), status (uint8,
        L.HMM_NO_SITE); sums (float64[8], L.HMM_GRAD_SUMS).  out: such a dict from an earlier call of the same shape."""
        opts, want = _hmm_grad_opts(pi, length, want)
        return self._chain('read_hmm_grad', L.make_hmm_grad_out, lambda nrows, nreads, nsites: _hmm_grad_shapes(want, nreads), opts,
                           (cs, start, roff, score, key), hoff, nrows, out, site_pi)

    def read_class_rows(self, cs, start, roff, score, key, hoff, nrows, *, want=CLASS_ROWS_OUTPUTS, out=None):
        """The rows of the latent-class fit (nmod_read_class_rows, NMOD_MEM_DEVICE), enqueued on the current stream without
        synchronising or reading anything back: the arguments of read_hmm.  Returns a dict of CUDA tensors, those named in `want`: per
        row site (int32), s (float64), rread (int32); soff (int64, nsites + 1) and srow (int32): the rows of site j are
        srow[soff[j]:soff[j + 1]] in ascending row index.  out: such a dict from an earlier call of the same shape."""
        want = _check_want(want, CLASS_ROWS_OUTPUTS)
        return self._chain('read_class_rows', L.make_class_rows_out,
                           lambda nrows, nreads, nsites: {k: v for k, v in _class_rows_shapes(nrows, nsites).items() if k in want}, None,
                           (cs, start, roff, score, key), hoff, nrows, out)

    def read_classes_step(self, rows, hoff, theta, w, *, want=CLASSES_OUTPUTS, out=None):
        """One EM step of the latent-class mixture over the reads (nmod_read_classes_step, NMOD_MEM_DEVICE), enqueued on the current
        stream without synchronising or reading anything back: `rows` as read_class_rows gives them (all five), hoff as read_sites
        does; theta (float64, nsites * C, the classes of a site contiguous) and w (float64, C) CUDA vectors, not checked.  Returns a
        dict of CUDA tensors, those named in `want`: gamma (float64, nreads * C), ll (float64), cls (int32), status (uint8); theta_out,
        n_site (float64, nsites * C); w_out (float64, C); sums (float64, 4 + C).  out: such a dict from an earlier call of the same
        shape."""
        torch = self.torch
        _cuda_vecs('read_classes_step', (('w', w, torch.float64, None),), one_dim=True, missing='refused')
        opts, want = _classes_opts(w.numel(), want)
        nc = w.numel()
        nreads = _device_offsets(torch, hoff, 'read_classes_step', 'nreads')
        for name in CLASS_ROWS_OUTPUTS:
            if rows.get(name) is None:
                raise ValueError('read_classes_step: rows must hold %s' % ', '.join(CLASS_ROWS_OUTPUTS))
        nsites = _device_offsets(torch, rows['soff'], 'read_classes_step', 'nsites')
        nrows = rows['site'].numel()
        _check_hmm_counts(nreads, nsites, nrows)
        _cuda_vecs('read_classes_step', (('site', rows['site'], torch.int32, nrows), ('s', rows['s'], torch.float64, nrows),
                                         ('rread', rows['rread'], torch.int32, nrows), ('srow', rows['srow'], torch.int32, nrows),
                                         ('theta', theta, torch.float64, nsites * nc)), missing='refused')
        if nrows > 0 and (nreads == 0 or nsites == 0):
            raise ValueError('read_classes_step: rows need reads and sites')
        shapes = _classes_shapes(want, nreads, nsites, nc)
        res = self._outputs(out, shapes, 'read_classes_step')
        o = L.make_classes_out(**{name: res[name].data_ptr() for name in shapes})
        prm = self._params(L.DTYPE_F64, 0, 0, 0, 0)
        _call(self.lib, 'nmod_read_classes_step', prm, nreads, nsites, nrows, hoff.data_ptr(), rows['site'].data_ptr(), rows['s'].data_ptr(),
              rows['rread'].data_ptr(), rows['soff'].data_ptr(), rows['srow'].data_ptr(), C.byref(opts), theta.data_ptr(), w.data_ptr(),
              C.byref(o))
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
                                             _ptr(off), plant_period,
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


def _torch_dtype_code(t):
    import torch
    return {torch.float32: L.DTYPE_F32, torch.int16: L.DTYPE_I16_MILLI, torch.float64: L.DTYPE_F64}[t.dtype]


def chrom_names(*read_sets):
    """the sorted chromosome names over read sets: the index space of the (chrom, strand) ids both groups must share"""
    heads = [np.unique(np.asarray(r['chrom']).astype(str)) for r in read_sets]
    return [str(n) for n in np.unique(np.concatenate(heads) if heads else np.zeros(0, str)).tolist()]


def chrom_strand_ids(chrom, strand, names, what='reads'):
    """the (chrom, strand) ids 2 * index in `names` + (strand == '-') of str arrays chrom and strand (int32): nmod_pivot_reads' cs and the
    upper bits of its keys"""
    n = len(chrom)
    if not np.all(np.isin(strand, ('+', '-'))):
        raise ValueError("%s: strand must be '+' or '-'" % what)
    cid = np.searchsorted(np.array(names, dtype=str), chrom) if n else np.zeros(0, np.int64)
    if n and (np.any(cid >= len(names)) or np.any(np.array(names, dtype=str)[np.minimum(cid, len(names) - 1)] != chrom)):
        raise ValueError('%s: a chromosome is missing from names' % what)
    return (2 * cid + (strand == '-')).astype(np.int32)


def key_sites(key, names):
    """chrom, strand and pos (a dict of numpy arrays, in that order) of a host vector of nmod_pivot_reads' keys cs << 40 | pos over the
    chromosome list `names`; chrom of no key is a zero-length str array"""
    key = np.asarray(key)
    return dict(chrom=np.array(names, dtype=str)[key >> 41] if len(key) else np.zeros(0, dtype=str),
                strand=np.where((key >> 40) & 1, '-', '+').astype('U1'), pos=key & ((1 << 40) - 1))


def read_head(reads, nreads, off=None):
    """the leading columns of a per-read table of a read-level set: index, chrom, strand and, with the reads' offsets, start and events"""
    head = dict(index=np.arange(nreads, dtype=np.int64), chrom=np.asarray(reads['chrom']).astype(str), strand=np.asarray(reads['strand']).astype(str))
    if off is not None:
        head.update(start=np.asarray(reads['start'], dtype=np.int64), events=np.diff(off))
    return head


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
    cs = chrom_strand_ids(chrom, strand, names)
    base =np.ascontiguousarray(np.asarray(reads['base']).astype('S1')).view(np.uint8)
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


def match_score_rows(g0, g1, min_coverage, device=0):
    """The rows of two pivoted score tracks (pivot_reads(..., val=llr_win) of two samples, the same `names`) that both hold with at
    least min_coverage scores, in key order (nmod_select_tested), gathered as float64 (nmod_gather_tested): the inputs of
    DeviceDetector.site_diff.  The dtype nmod_select_tested proposes is ignored: it is meant for signal levels and would narrow score
    rows that happen to be float32-exact or to lie on the 0.001 grid.  Returns device tensors key, base (sample 1's), off0, off1,
    sig0, sig1."""
    import torch
    lib = L.load()
    if list(g0['names']) != list(g1['names']):
        raise ValueError('both samples must be pivoted with the same chromosome names')
    s0, s1 = g0['sig'], g1['sig']
    if s0.dtype != torch.float64 or s1.dtype != torch.float64:
        raise ValueError('match_score_rows takes float64 score rows (pivot_reads with val=llr_win)')
    dev = torch.device('cuda', device)
    prm = L.make_params(device=device, memspace=L.MEM_DEVICE, dtype=L.DTYPE_F64, stream=torch.cuda.current_stream(dev).cuda_stream)
    n0, n1 = g0['key'].numel(), g1['key'].numel()
    cap = min(n0, n1)
    rows0 = torch.empty(max(cap, 1), dtype=torch.int64, device=dev); rows1 = torch.empty_like(rows0)
    off0 = torch.empty(cap + 1, dtype=torch.int64, device=dev); off1 = torch.empty_like(off0)
    nt, ns0, ns1, odt = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
    ptr = lambda x: x.data_ptr() if x.numel() else None
    L.check(lib.nmod_select_tested(C.byref(prm), int(min_coverage), n0, ptr(g0['key']), g0['off'].data_ptr(), ptr(s0), s0.numel(),
                                   n1, ptr(g1['key']), g1['off'].data_ptr(), ptr(s1), s1.numel(), cap, rows0.data_ptr(),
                                   rows1.data_ptr(), off0.data_ptr(), off1.data_ptr(), C.byref(nt), C.byref(ns0), C.byref(ns1),
                                   C.byref(odt)), 'nmod_select_tested')
    npos = nt.value
    sig0 = torch.empty(ns0.value, dtype=torch.float64, device=dev); sig1 = torch.empty(ns1.value, dtype=torch.float64, device=dev)
    run = torch.empty(npos, dtype=torch.int32, device=dev)
    key = torch.empty(npos, dtype=torch.int64, device=dev)
    b0 = torch.empty(npos, dtype=torch.uint8, device=dev); b1 = torch.empty_like(b0)
    off0, off1 = off0[:npos + 1], off1[:npos + 1]
    L.check(lib.nmod_gather_tested(C.byref(prm), npos, rows0.data_ptr(), rows1.data_ptr(), g0['off'].data_ptr(), ptr(s0),
                                   ptr(g0['base']), g1['off'].data_ptr(), ptr(s1), ptr(g1['base']), ptr(g1['key']), L.DTYPE_F64,
                                   off0.data_ptr(), off1.data_ptr(), ptr(sig0), ptr(sig1), ptr(run), ptr(key), ptr(b0), ptr(b1)),
            'nmod_gather_tested')
    return dict(key=key, base=b1, off0=off0, off1=off1, sig0=sig0, sig1=sig1, names=list(g1['names']))


def match_score_rows_multi(pivots, n_control, min_coverage, device=0):
    """The sites that every one of several pivoted score tracks (pivot_reads(..., val=llr_win) per sample, the same `names`; the first
    n_control of them condition 0) holds with at least min_coverage scores, in key order, gathered site-major as float64: the inputs
    of DeviceDetector.site_diff_rep.  Off the hot path: torch as plumbing, with the synchronisations its data-dependent shapes take.
    Returns device tensors key, base (the last sample's), off (npos * G + 1, row i * G + g), sig, and names, n_samples, n_control."""
    import torch
    G = len(pivots)
    if not 3 <= G <= L.REP_MAX_SAMPLES or not 1 <= int(n_control) <= G - 1:
        raise ValueError('match_score_rows_multi takes 3 .. %d samples with 1 .. G - 1 of them controls' % L.REP_MAX_SAMPLES)
    names = list(pivots[0]['names'])
    if any(list(g['names']) != names for g in pivots):
        raise ValueError('all samples must be pivoted with the same chromosome names')
    if any(g['sig'].dtype != torch.float64 for g in pivots):
        raise ValueError('match_score_rows_multi takes float64 score rows (pivot_reads with val=llr_win)')
    dev = torch.device('cuda', device)
    cov = [g['off'][1:] - g['off'][:-1] for g in pivots]
    kept = [g['key'][c >= int(min_coverage)] for g, c in zip(pivots, cov)]
    allk, cnt = torch.unique(torch.cat(kept), sorted=True, return_counts=True)        # (a pivot's keys are distinct)
    key = allk[cnt == G]
    npos = key.numel()
    rows = [torch.searchsorted(g['key'], key) for g in pivots]
    lens = torch.stack([c[r] for c, r in zip(cov, rows)], dim=1) if npos else torch.zeros((0, G), dtype=torch.int64, device=dev)
    off = torch.zeros(npos * G + 1, dtype=torch.int64, device=dev)
    torch.cumsum(lens.reshape(-1), 0, out=off[1:])
    sig = torch.empty(int(off[-1]), dtype=torch.float64, device=dev)
    for g, (piv, r) in enumerate(zip(pivots, rows)):
        n = lens[:, g]
        tot = int(n.sum())
        if not tot:
            continue
        first = torch.cumsum(n, 0) - n
        within = torch.arange(tot, dtype=torch.int64, device=dev) - torch.repeat_interleave(first, n)
        src = torch.repeat_interleave(piv['off'][:-1][r], n) + within
        dst = torch.repeat_interleave(off[:-1].reshape(npos, G)[:, g], n) + within
        sig[dst] = piv['sig'][src]
    base = pivots[-1]['base'][rows[-1]] if npos else torch.zeros(0, dtype=torch.uint8, device=dev)
    return dict(key=key, base=base, off=off, sig=sig, names=names, n_samples=G, n_control=int(n_control))
