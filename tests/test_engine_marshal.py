"""What the host entry points of nanomod_amd.engine hand to the C ABI, and what they refuse before calling it (CPU only).

The first half replaces the loaded library by a stand-in that records the arguments of every nmod_* call and returns 0, calls
each secondary host entry once per layout it supports at tiny shapes, and compares what reached the C call with expectations
written down by hand from include/nanomod_hip.h: struct sizes, which members and pointer arguments are NULL, which are the
caller's (or the returned) arrays, the scalars and every field of the option structs.  The second half is a table of calls
the real library must never see: each raises ValueError with device=NO_SUCH_DEVICE, where a call that got through would
raise NanomodLibraryError instead."""
import ctypes as C

import numpy as np
import pytest

from nanomod_amd import _lib as L, engine

NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine

# include/nanomod_hip.h, counted by hand (LP64: pointers and doubles are 8 bytes and 8-aligned)
SIZEOF_PARAMS = 88           # 2 x i32, ptr, 6 x i32, double, 2 x i64, 2 x i32, ptr, 2 x i32
SIZEOF_ONE_OUT = 88          # 2 x i32 + 10 pointers
SIZEOF_KMER_OUT = 56         # 2 x i32 + 6 pointers
SIZEOF_RESCALE_OPTS = 48     # 6 x i32 + 3 doubles
SIZEOF_RESCALE_OUT = 48      # 2 x i32 + 5 pointers
SIZEOF_CALLS_OPTS = 16       # 2 x i32 + double
SIZEOF_CALLS_OUT = 56        # 2 x i32 + 6 pointers
SIZEOF_SITE_OUT = 32         # 2 x i32 + 3 pointers
MEM_HOST, F32, I16, F64 = 0, 0, 1, 2
KS, STOUFFER = 0, 1

NPOS, ROW, NCODES, NREADS, READ_LEN = 4, 10, 4, 3, 6


def _snap(a):
    """an argument of a recorded call as plain Python: a struct passed by reference as a dict of its fields, a pointer as its
    address (None for NULL), an array of pointers as a list"""
    if hasattr(a, '_obj'):
        s = a._obj
        return {n: getattr(s, n) for n, *_ in s._fields_}
    if isinstance(a, C.Array):
        return [(x.tolist() if hasattr(x, 'tolist') else x) for x in a] if a._type_ is C.c_void_p else a
    if isinstance(a, C.c_void_p):
        return a.value
    return a


class Recorder:
    """stands in for the loaded library: every nmod_* attribute records its arguments and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('nmod_'):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, [_snap(a) for a in args]))
            return 0
        return fn

    def only(self, name):
        assert [c[0] for c in self.calls] == [name]
        return self.calls[0][1]


@pytest.fixture
def rec(monkeypatch):
    r = Recorder()
    monkeypatch.setattr(L, 'load', lambda: r)
    monkeypatch.setattr(engine, '_join_warm_up', lambda device: None)
    return r


def addr(a):
    return a.ctypes.data


def check_params(prm, *, dtype, device, method=STOUFFER, nb=2, stride0=0, stride1=0):
    """nmod_params of a host call; method / nb default to what an entry that does not use them leaves (stouffer, 2)"""
    got = {k: prm[k] for k in ('struct_size', 'memspace', 'dtype', 'method', 'nb', 'device', 'stride0', 'stride1')}
    assert got == dict(struct_size=SIZEOF_PARAMS, memspace=MEM_HOST, dtype=dtype, method=method, nb=nb, device=device,
                       stride0=stride0, stride1=stride1)
    assert prm['stream'] is None and prm['reserved'] == 0


def check_out(out, res, size=None, rename=None):
    """the out struct: its struct_size, and exactly the members of `res` non-NULL, each the address of the returned array"""
    rename = rename or {}
    want = {rename.get(k, k): addr(a) for k, a in res.items()}
    members = {k: v for k, v in out.items() if k not in ('struct_size', 'reserved')}
    if size is None:
        assert 'struct_size' not in out
    else:
        assert out['struct_size'] == size and out['reserved'] == 0
    assert {k for k, v in members.items() if v is not None} == set(want)
    for k, v in want.items():
        assert members[k] == v, k


def check_arrays(res, spec):
    """keys, dtypes and shapes of a returned dict: spec is name -> (dtype, shape)"""
    assert set(res) == set(spec)
    for k, (dt, shape) in spec.items():
        assert isinstance(res[k], np.ndarray) and res[k].dtype == np.dtype(dt) and res[k].shape == shape, k
        assert res[k].flags.c_contiguous


def rows(dtype=np.float32, extra=0, seed=1):
    x = np.random.default_rng(seed).normal(size=NPOS * ROW + extra)
    return (x * 1000).astype(np.int16) if dtype == np.int16 else x.astype(dtype)


def row_off():
    return np.arange(NPOS + 1, dtype=np.int64) * ROW


# ------------------------------------------------------------------------------------------------------------------- fdr
def test_fdr_adjust_host(rec):
    p0, p1 = np.linspace(0, 1, 5), np.linspace(1, 0, 5)
    qs, summ = engine.fdr_adjust_host([p0, p1], method='by', alpha=0.1, device=3)
    prm, n, nt, parr, method, alpha, qarr, summary = rec.only('nmod_fdr_adjust')
    check_params(prm, dtype=F32, device=3)
    assert (n, nt, method, alpha) == (5, 2, 1, 0.1)                      # NMOD_FDR_BY = 1
    assert parr == [addr(p0), addr(p1)]
    assert qarr == [addr(q) for q in qs]
    assert summary is not None
    assert len(qs) == 2 and all(q.dtype == np.float64 and q.shape == (5,) for q in qs)
    assert [sorted(s) for s in summ] == [['excluded', 'p_crit', 'rejected', 'tested']] * 2


def test_fdr_adjust_host_one_track_and_empty(rec):
    p = np.linspace(0, 1, 5)
    qs, summ = engine.fdr_adjust_host(p)
    prm, n, nt, parr, method, alpha, qarr, summary = rec.only('nmod_fdr_adjust')
    check_params(prm, dtype=F32, device=0)
    assert (n, nt, method, alpha) == (5, 1, 0, 0.05) and parr == [addr(p)] and qarr == [addr(qs[0])]
    rec.calls.clear()
    qs, summ = engine.fdr_adjust_host([np.zeros(0)])
    assert rec.only('nmod_fdr_adjust')[1:3] == [0, 1]
    assert len(qs) == 1 and qs[0].dtype == np.float64 and qs[0].shape == (0,) and len(summ) == 1


# ------------------------------------------------------------------------------------------------------------------- mix
@pytest.mark.parametrize('mix_group', [0, 1])
@pytest.mark.parametrize('layout', ['csr', 'stride', 'mixed'])
def test_mix_fraction_host(rec, layout, mix_group):
    sig0, sig1 = rows(extra=5, seed=1), rows(extra=3, seed=2)            # longer than the rows: resp has the rows' length
    off0 = row_off() if layout in ('csr', 'mixed') else None
    off1 = row_off() if layout == 'csr' else None
    gate = np.array([0.0, 0.5, np.nan, 0.01])
    res = engine.mix_fraction_host(sig0, off0, sig1, off1, mix_group=mix_group, model='free', max_iter=50, tol=1e-4, gate=gate,
                                   gate_max=0.2, want_resp=True, device=2, stride0=ROW, stride1=ROW)
    prm, npos, s0, o0, s1, o1, grp, model, max_iter, tol, g, gate_max, out = rec.only('nmod_mix_fraction')
    check_params(prm, dtype=F32, device=2, stride0=0 if off0 is not None else ROW, stride1=0 if off1 is not None else ROW)
    assert (npos, grp, model, max_iter, tol, gate_max) == (NPOS, mix_group, 1, 50, 1e-4, 0.2)          # NMOD_MIX_FREE_VAR = 1
    assert (s0, s1, g) == (addr(sig0), addr(sig1), addr(gate))
    assert o0 == (addr(off0) if off0 is not None else None) and o1 == (addr(off1) if off1 is not None else None)
    f8 = (np.float64, (NPOS,))
    check_arrays(res, dict(pi=f8, mu_mod=f8, sd_mod=f8, llr=f8, iters=(np.int32, (NPOS,)), status=(np.uint8, (NPOS,)),
                           resp=(np.float32, (NPOS * ROW,))))
    check_out(out, res)


def test_mix_fraction_host_plain_and_empty(rec):
    sig0, sig1 = rows(np.int16, seed=1), rows(np.int16, seed=2)
    res = engine.mix_fraction_host(sig0, None, sig1, None, stride0=ROW, stride1=ROW)
    prm, npos, s0, o0, s1, o1, grp, model, max_iter, tol, g, gate_max, out = rec.only('nmod_mix_fraction')
    check_params(prm, dtype=I16, device=0, stride0=ROW, stride1=ROW)
    assert (npos, o0, o1, grp, model, max_iter, tol, g, gate_max) == (NPOS, None, None, 1, 0, 200, 1e-6, None, 0.05)
    assert set(res) == {'pi', 'mu_mod', 'sd_mod', 'llr', 'iters', 'status'}
    check_out(out, res)                                                  # resp stays NULL
    rec.calls.clear()
    z = np.zeros(1, np.int64)
    res = engine.mix_fraction_host(np.zeros(0, np.float32), z, np.zeros(0, np.float32), z, want_resp=True)
    assert rec.only('nmod_mix_fraction')[1] == 0
    f8 = (np.float64, (0,))
    check_arrays(res, dict(pi=f8, mu_mod=f8, sd_mod=f8, llr=f8, iters=(np.int32, (0,)), status=(np.uint8, (0,)), resp=(np.float32, (0,))))


# ------------------------------------------------------------------------------------------------------------ one sample
ONE_TRACKS = ('ks_d', 'ks_p', 't_t', 't_p', 'shift', 'mean', 'std')


@pytest.mark.parametrize('with_n', [False, True])
@pytest.mark.parametrize('method', ['ks', 'stouffer'])
@pytest.mark.parametrize('layout', ['csr', 'stride'])
def test_one_sample_host(rec, layout, method, with_n):
    sig = rows(np.int16)
    off = row_off() if layout == 'csr' else None
    mu, sd = np.zeros(NPOS), np.ones(NPOS)
    n = np.full(NPOS, 30, np.int32) if with_n else None
    run = np.zeros(NPOS, np.int32) if method != 'ks' else None
    res = engine.one_sample_host(sig, off, mu, sd, n, run, stride=ROW, nb=3, weights_dif=1.5, method=method, device=1)
    prm, npos, s, o, m, d, rn, ri, out = rec.only('nmod_one_sample')
    check_params(prm, dtype=I16, device=1, method=KS if method == 'ks' else STOUFFER, nb=3, stride0=0 if off is not None else ROW)
    assert prm['weights_dif'] == 1.5
    assert (npos, s, m, d) == (NPOS, addr(sig), addr(mu), addr(sd))
    assert o == (addr(off) if off is not None else None)
    assert rn == (addr(n) if with_n else None) and ri == (addr(run) if run is not None else None)
    tracks = ONE_TRACKS + (() if method == 'ks' else ('comb_st', 'comb_p'))
    spec = {k: (np.float64, (NPOS,)) for k in tracks}
    spec['status'] = (np.uint8, (NPOS,))
    check_arrays(res, spec)
    check_out(out, res, SIZEOF_ONE_OUT)


def test_one_sample_host_empty(rec):
    res = engine.one_sample_host(np.zeros(0, np.float64), np.zeros(1, np.int64), np.zeros(0), np.zeros(0), method='ks')
    prm, npos = rec.only('nmod_one_sample')[:2]
    check_params(prm, dtype=F64, device=0, method=KS)
    assert npos == 0
    spec = {k: (np.float64, (0,)) for k in ONE_TRACKS}
    spec['status'] = (np.uint8, (0,))
    check_arrays(res, spec)


# ------------------------------------------------------------------------------------------------------------ k-mer model
def kmer_spec(npos, ncodes):
    spec = {k: (np.int64, (ncodes,)) for k in ('n_positions', 'n_samples', 'n_clipped')}
    spec.update(mean=(np.float64, (ncodes,)), sd=(np.float64, (ncodes,)), pos_status=(np.uint8, (npos,)))
    return spec


@pytest.mark.parametrize('keep', [False, True])
@pytest.mark.parametrize('layout', ['csr', 'stride'])
def test_kmer_model_host(rec, layout, keep):
    sig = rows(np.float64)
    off = row_off() if layout == 'csr' else None
    code = np.array([0, 3, -1, 1], np.int32)
    lo, hi = (np.full(NCODES, -2.0), np.full(NCODES, 2.0)) if keep else (None, None)
    res = engine.kmer_model_host(sig, off, code, NCODES, lo, hi, stride=ROW, device=1)
    prm, npos, s, o, c, ncodes, klo, khi, out = rec.only('nmod_kmer_model')
    check_params(prm, dtype=F64, device=1, stride0=0 if off is not None else ROW)
    assert (npos, s, c, ncodes) == (NPOS, addr(sig), addr(code), NCODES)
    assert o == (addr(off) if off is not None else None)
    assert (klo, khi) == ((addr(lo), addr(hi)) if keep else (None, None))
    check_arrays(res, kmer_spec(NPOS, NCODES))
    check_out(out, res, SIZEOF_KMER_OUT)


def test_kmer_model_host_empty(rec):
    res = engine.kmer_model_host(np.zeros(0, np.float32), np.zeros(1, np.int64), np.zeros(0, np.int32), NCODES)
    assert rec.only('nmod_kmer_model')[1] == 0
    check_arrays(res, kmer_spec(0, NCODES))


# --------------------------------------------------------------------------------------------------------- reads: K11, K12
def reads(first=0, dtype=np.float32, tail=2):
    """NREADS reads of READ_LEN events from event `first` on, `tail` events after the last read"""
    off = first + np.arange(NREADS + 1, dtype=np.int64) * READ_LEN
    n = int(off[-1]) + tail
    val = np.random.default_rng(3).normal(size=n)
    val = (val * 1000).astype(np.int16) if dtype == np.int16 else val.astype(dtype)
    base = np.frombuffer(b'ACGT' * n, np.uint8)[:n].copy()
    return val, off, base


def kmer_model():
    return dict(k=1, center=0, mean=np.array([-1.0, 0.0, 1.0, 2.0]), sd=np.full(4, 0.5))


RESCALE_MODES = {'fit_apply': 0, 'fit_only': 1, 'apply_only': 2}


@pytest.mark.parametrize('first', [0, 2])
@pytest.mark.parametrize('mode', sorted(RESCALE_MODES))
def test_rescale_reads_host(rec, mode, first):
    val, off, base = reads(first, np.int16)
    model = kmer_model()
    shift, scale = np.array([0.1, 0.2, 0.3]), np.array([1.0, 1.1, 0.9])
    kw = dict(shift=shift, scale=scale) if mode == 'apply_only' else {}
    res = engine.rescale_reads_host(val, off, base, None if mode == 'apply_only' else model, mode=mode, weighted=False, clip_sigma=2.5,
                                    clip_rounds=1, min_events=2, scale_range=(0.25, 4.0), device=1, **kw)
    prm, nreads, o, v, b, m, opts, out = rec.only('nmod_rescale_reads')
    check_params(prm, dtype=I16, device=1)
    assert (nreads, o, v) == (NREADS, addr(off), addr(val))
    if mode == 'apply_only':
        assert b is None and m == dict(k=0, center=0, mean=None, sd=None)
    else:
        assert b == addr(base) and m == dict(k=1, center=0, mean=addr(model['mean']), sd=addr(model['sd']))
    assert opts == dict(struct_size=SIZEOF_RESCALE_OPTS, mode=RESCALE_MODES[mode], weighted=0, clip_rounds=1, min_events=2, reserved=0,
                        clip_sigma=2.5, scale_lo=0.25, scale_hi=4.0)
    spec = dict(shift=(np.float64, (NREADS,)), scale=(np.float64, (NREADS,)), n_used=(np.int32, (NREADS,)), status=(np.uint8, (NREADS,)))
    if mode != 'fit_only':
        spec['val'] = (np.int16, val.shape)
    check_arrays(res, spec)
    check_out(out, res, SIZEOF_RESCALE_OUT, rename={'val': 'val_out'})
    assert not res['n_used'].any() and not res['status'].any()           # zeroed before the call
    if mode == 'apply_only':                                             # the caller's pairs, as copies of the entry's own
        assert res['shift'] is not shift and res['scale'] is not scale
        assert np.array_equal(res['shift'], shift) and np.array_equal(res['scale'], scale)
    if mode != 'fit_only':                                               # events outside [off[0], off[-1]) are copied through
        assert res['val'] is not val
        assert np.array_equal(res['val'][:first], val[:first]) and np.array_equal(res['val'][off[-1]:], val[off[-1]:])


def test_rescale_reads_host_s1_base_and_empty(rec):
    val, off, base = reads(0, np.float64)
    res = engine.rescale_reads_host(val, off, base.view('S1'), kmer_model(), min_events=2)
    prm, nreads, o, v, b, m, opts, out = rec.only('nmod_rescale_reads')
    check_params(prm, dtype=F64, device=0)
    assert b is not None and m['k'] == 1
    assert opts == dict(struct_size=SIZEOF_RESCALE_OPTS, mode=0, weighted=1, clip_rounds=2, min_events=2, reserved=0,
                        clip_sigma=3.0, scale_lo=0.5, scale_hi=2.0)
    rec.calls.clear()
    res = engine.rescale_reads_host(np.zeros(0, np.float32), np.zeros(1, np.int64), np.zeros(0, np.uint8), kmer_model(), min_events=2)
    assert rec.only('nmod_rescale_reads')[1] == 0
    check_arrays(res, dict(shift=(np.float64, (0,)), scale=(np.float64, (0,)), n_used=(np.int32, (0,)), status=(np.uint8, (0,)),
                           val=(np.float32, (0,))))


@pytest.mark.parametrize('first', [0, 2])
@pytest.mark.parametrize('want', [('p_win',), ('z', 'p', 'p_win')])
def test_read_calls_host(rec, want, first):
    val, off, base = reads(first)
    model = kmer_model()
    res = engine.read_calls_host(val, off, base, model, nb=3, alpha=0.02, want=want, device=1)
    prm, nreads, o, v, b, m, opts, out = rec.only('nmod_read_calls')
    check_params(prm, dtype=F32, device=1)
    assert (nreads, o, v, b) == (NREADS, addr(off), addr(val), addr(base))
    assert m == dict(k=1, center=0, mean=addr(model['mean']), sd=addr(model['sd']))
    assert opts == dict(struct_size=SIZEOF_CALLS_OPTS, nb=3, alpha=0.02)
    spec = {w: (np.float64, val.shape) for w in want}
    spec.update(n_sites=(np.int32, (NREADS,)), n_called=(np.int32, (NREADS,)), status=(np.uint8, (NREADS,)))
    check_arrays(res, spec)
    check_out(out, res, SIZEOF_CALLS_OUT)
    for w in want:                                                       # nothing was written: the padding (and all else) is NaN
        assert np.isnan(res[w]).all()
    assert not res['n_sites'].any() and not res['n_called'].any() and not res['status'].any()


def test_read_calls_host_empty(rec):
    res = engine.read_calls_host(np.zeros(0, np.float32), np.zeros(1, np.int64), np.zeros(0, np.uint8), kmer_model())
    prm, nreads, o, v, b, m, opts, out = rec.only('nmod_read_calls')
    assert nreads == 0 and opts == dict(struct_size=SIZEOF_CALLS_OPTS, nb=2, alpha=0.01)
    spec = {w: (np.float64, (0,)) for w in ('z', 'p', 'p_win')}
    spec.update(n_sites=(np.int32, (0,)), n_called=(np.int32, (0,)), status=(np.uint8, (0,)))
    check_arrays(res, spec)


@pytest.mark.parametrize('layout', ['csr', 'stride'])
def test_site_calls_host(rec, layout):
    score = np.random.default_rng(4).uniform(size=NPOS * ROW)
    off = row_off() if layout == 'csr' else None
    res = engine.site_calls_host(score, off, stride=ROW, alpha=0.02, device=1)
    prm, npos, s, o, alpha, out = rec.only('nmod_site_calls')
    check_params(prm, dtype=F64, device=1, stride0=0 if off is not None else ROW)
    assert (npos, s, alpha) == (NPOS, addr(score), 0.02)
    assert o == (addr(off) if off is not None else None)
    check_arrays(res, dict(n_valid=(np.int32, (NPOS,)), n_called=(np.int32, (NPOS,)), frac=(np.float64, (NPOS,))))
    check_out(out, res, SIZEOF_SITE_OUT)
    assert not res['n_valid'].any() and not res['n_called'].any() and np.isnan(res['frac']).all()


def test_site_calls_host_empty(rec):
    res = engine.site_calls_host(np.zeros(0), np.zeros(1, np.int64))
    assert rec.only('nmod_site_calls')[1] == 0
    check_arrays(res, dict(n_valid=(np.int32, (0,)), n_called=(np.int32, (0,)), frac=(np.float64, (0,))))


def test_warm_up_is_joined_before_the_call(monkeypatch):
    """every host entry that waits for warm_up() does so before its C call (fdr_adjust_host never did)"""
    order = []

    class Lib(Recorder):
        def __getattr__(self, name):
            fn = Recorder.__getattr__(self, name)
            return lambda *a: (order.append(name), fn(*a))[1]
    monkeypatch.setattr(L, 'load', lambda: Lib())
    monkeypatch.setattr(engine, '_join_warm_up', lambda device: order.append(('join', device)))
    sig, off = rows(), row_off()
    val, roff, base = reads()
    engine.mix_fraction_host(sig, off, sig, off, device=5)
    engine.one_sample_host(sig, off, np.zeros(NPOS), np.ones(NPOS), method='ks', device=5)
    engine.kmer_model_host(sig, off, np.zeros(NPOS, np.int32), NCODES, device=5)
    engine.rescale_reads_host(val, roff, base, kmer_model(), min_events=2, device=5)
    engine.read_calls_host(val, roff, base, kmer_model(), device=5)
    engine.site_calls_host(np.zeros(NPOS * ROW), off, device=5)
    calls = ['nmod_mix_fraction', 'nmod_one_sample', 'nmod_kmer_model', 'nmod_rescale_reads', 'nmod_read_calls', 'nmod_site_calls']
    assert order == [x for c in calls for x in (('join', 5), c)]


# ------------------------------------------------------------------------------------------------------------ refused calls
def _refused():
    """(id, function, args, kwargs): calls a shared argument rule refuses; the real library must not be reached"""
    sig, off = rows(), row_off()
    mu, sd = np.zeros(NPOS), np.ones(NPOS)
    code = np.zeros(NPOS, np.int32)
    val, roff, base = reads()
    model = kmer_model()
    score = np.zeros(NPOS * ROW)
    bad_off = {'long': np.arange(NPOS + 2, dtype=np.int64) * ROW, 'short': row_off()[:-1]}
    down = np.array([0, 12, 6, 18], np.int64)
    neg = np.array([-1, 6, 12, 18], np.int64)
    past = roff + 4                                                      # the last read ends beyond val, base and the scores
    mix, one, kmer = engine.mix_fraction_host, engine.one_sample_host, engine.kmer_model_host
    rescale, calls, site = engine.rescale_reads_host, engine.read_calls_host, engine.site_calls_host
    i32 = lambda a: a.astype(np.int32)
    m_with = lambda **kw: dict(model, **kw)
    return [
        # the signal dtype
        ('dtype-mix', mix, (i32(sig), off, i32(sig), off), {}),
        ('dtype-mix-differ', mix, (sig, off, sig.astype(np.float64), off), {}),
        ('dtype-one', one, (i32(sig), off, mu, sd), {}),
        ('dtype-kmer', kmer, (i32(sig), off, code, NCODES), {}),
        ('dtype-rescale', rescale, (i32(val), roff, base, model), dict(min_events=2)),
        ('dtype-calls', calls, (i32(val), roff, base, model), {}),
        # offsets of the wrong length
        ('off-long-mix0', mix, (sig, bad_off['long'], sig, None), dict(stride1=ROW)),
        ('off-long-mix1', mix, (sig, off, sig, bad_off['long']), {}),
        ('off-long-one', one, (sig, bad_off['long'], mu, sd), {}),
        ('off-short-one', one, (sig, bad_off['short'], mu, sd), {}),
        ('off-long-kmer', kmer, (sig, bad_off['long'], code, NCODES), {}),
        ('off-2d-rescale', rescale, (val, roff.reshape(2, 2), base, model), dict(min_events=2)),
        ('off-empty-calls', calls, (val, roff[:0], base, model), {}),
        ('off-empty-site', site, (score, off[:0]), {}),
        # offsets that decrease or start below 0 (the read layout)
        ('off-down-rescale', rescale, (val, down, base, model), dict(min_events=2)),
        ('off-down-calls', calls, (val, down, base, model), {}),
        ('off-down-site', site, (score, down), {}),
        ('off-neg-rescale', rescale, (val, neg, base, model), dict(min_events=2)),
        ('off-neg-calls', calls, (val, neg, base, model), {}),
        ('off-neg-site', site, (score, neg), {}),
        # a signal shorter than its offsets say
        ('short-off-mix0', mix, (sig[:-1], off, sig, off), {}),
        ('short-off-mix1', mix, (sig, off, sig[:-1], off), {}),
        ('short-off-one', one, (sig[:-1], off, mu, sd), {}),
        ('short-off-kmer', kmer, (sig[:-1], off, code, NCODES), {}),
        ('short-off-rescale', rescale, (val, past, base, model), dict(min_events=2)),
        ('short-off-calls', calls, (val, past, base, model), {}),
        ('short-off-site', site, (score[:-1], off), {}),
        # a signal shorter than npos rows of the stride
        ('short-stride-mix1', mix, (sig, None, sig[:-1], None), dict(stride0=ROW, stride1=ROW)),
        ('short-stride-one', one, (sig[:-1], None, mu, sd), dict(stride=ROW)),
        ('short-stride-kmer', kmer, (sig[:-1], None, code, NCODES), dict(stride=ROW)),
        # side vectors of the wrong length
        ('ref_sd', one, (sig, off, mu, sd[:-1]), {}),
        ('ref_n', one, (sig, off, mu, sd, np.full(NPOS + 1, 9, np.int32)), dict(method='ks')),
        ('run_id', one, (sig, off, mu, sd, None, np.zeros(NPOS - 1, np.int32)), {}),
        ('gate', mix, (sig, off, sig, off), dict(gate=np.zeros(NPOS + 1))),
        ('keep_lo', kmer, (sig, off, code, NCODES, np.zeros(NCODES - 1), np.ones(NCODES)), {}),
        ('keep_hi', kmer, (sig, off, code, NCODES, np.zeros(NCODES), np.ones(NCODES + 1)), {}),
        ('keep_lo-alone', kmer, (sig, off, code, NCODES, np.zeros(NCODES), None), {}),
        ('keep_hi-alone', kmer, (sig, off, code, NCODES, None, np.ones(NCODES)), {}),
        ('shift', rescale, (val, roff, base), dict(mode='apply_only', shift=np.zeros(NREADS + 1), scale=np.ones(NREADS))),
        ('scale', rescale, (val, roff, base), dict(mode='apply_only', shift=np.zeros(NREADS), scale=np.ones(NREADS - 1))),
        ('shift-missing', rescale, (val, roff, base), dict(mode='apply_only', scale=np.ones(NREADS))),
        ('code-2d', kmer, (sig, off, code.reshape(2, 2), NCODES), {}),
        # the model block
        ('mean-rescale', rescale, (val, roff, base, m_with(mean=np.zeros(5))), dict(min_events=2)),
        ('sd-rescale', rescale, (val, roff, base, m_with(sd=np.ones(16))), dict(min_events=2)),
        ('mean-calls', calls, (val, roff, base, m_with(mean=np.zeros(3))), {}),
        ('sd-calls', calls, (val, roff, base, m_with(sd=np.ones(16))), {}),
        ('base-rescale', rescale, (val, roff, base[:int(roff[-1]) - 1], model), dict(min_events=2)),
        ('base-calls', calls, (val, roff, base[:int(roff[-1]) - 1], model), {}),
        ('no-model-rescale', rescale, (val, roff, base, None), dict(min_events=2)),
        ('no-model-calls', calls, (val, roff, base, None), {}),
        # the scalar rules
        ('k0-rescale', rescale, (val, roff, base, m_with(k=0)), dict(min_events=2)),
        ('k9-rescale', rescale, (val, roff, base, m_with(k=9)), dict(min_events=2)),
        ('k0-calls', calls, (val, roff, base, m_with(k=0)), {}),
        ('k9-calls', calls, (val, roff, base, m_with(k=9)), {}),
        ('center-rescale', rescale, (val, roff, base, m_with(center=1)), dict(min_events=2)),
        ('center-calls', calls, (val, roff, base, m_with(center=1)), {}),
        ('center-neg-calls', calls, (val, roff, base, m_with(center=-1)), {}),
        ('alpha0-calls', calls, (val, roff, base, model), dict(alpha=0.0)),
        ('alpha1.5-calls', calls, (val, roff, base, model), dict(alpha=1.5)),
        ('alpha0-site', site, (score, off), dict(alpha=0.0)),
        ('alpha1.5-site', site, (score, off), dict(alpha=1.5)),
        ('alpha-nan-site', site, (score, off), dict(alpha=float('nan'))),
        # site_calls_host's fixed-stride form
        ('stride0-site', site, (score, None), dict(stride=0)),
        ('ragged-site', site, (score[:-1], None), dict(stride=ROW)),
        ('score-2d-site', site, (score.reshape(NPOS, ROW), off), {}),
        # the per-entry option checkers stay in front of the library too
        ('mix-model', mix, (sig, off, sig, off), dict(model='storey')),
        ('fdr-method', engine.fdr_adjust_host, (mu,), dict(method='storey')),
        ('fdr-lengths', engine.fdr_adjust_host, ([mu, mu[:-1]],), {}),
        ('rescale-mode', rescale, (val, roff, base, model), dict(mode='refit')),
        ('calls-want', calls, (val, roff, base, model), dict(want=('q',))),
    ]


@pytest.mark.parametrize('fn,args,kw', [pytest.param(f, a, k, id=i) for i, f, a, k in _refused()])
def test_refused_before_the_library(fn, args, kw):
    L.load()                                     # the real library: a call that reached it would be a NanomodLibraryError
    with pytest.raises(ValueError):
        fn(*args, device=NO_SUCH_DEVICE, **kw)


def test_accepted_calls_reach_the_library():
    """the counterpart of the table above: a well-formed call gets past the checks and fails in the library, on the device"""
    sig, off = rows(), row_off()
    val, roff, base = reads()
    with pytest.raises(L.NanomodLibraryError):
        engine.one_sample_host(sig, off, np.zeros(NPOS), np.ones(NPOS), method='ks', device=NO_SUCH_DEVICE)
    with pytest.raises(L.NanomodLibraryError):
        engine.read_calls_host(val, roff, base, kmer_model(), device=NO_SUCH_DEVICE)


# ------------------------------------------------------------------------------------------------------------ the chain entries
# (K19 .. K22: one argument layer, engine._chain_host) the four host wrappers, the outputs `want` may name and whether the entry has
# the chain's two parameters
CHAIN_HOSTS = [('hmm', engine.read_hmm_host, engine.HMM_OUTPUTS, True), ('viterbi', engine.read_viterbi_host, engine.VIT_OUTPUTS, True),
               ('grad', engine.read_hmm_grad_host, engine.HMM_GRAD_OUTPUTS, True),
               ('class_rows', engine.read_class_rows_host, engine.CLASS_ROWS_OUTPUTS, False)]
# three reads (the second without an event) over three sites of (chrom, strand) id 0, and their offsets of rows
CHAIN_READS = (np.zeros(3, np.int32), np.array([10, 30, 50], np.int64), np.array([0, 4, 4, 9], np.int64), np.zeros(9),
               np.array([11, 12, 52], np.int64))
CHAIN_HOFF = np.array([0, 2, 2, 3], np.int64)
CHAIN_BAD = [
    ('pi-0', dict(pi=0.0), 'pi must lie in 1e-9 .. 1 - 1e-9, not 0.0'),
    ('pi-nan', dict(pi=float('nan')), 'pi must lie in 1e-9 .. 1 - 1e-9, not nan'),
    ('length-small', dict(length=1e-4), 'length must lie in 1e-3 .. 1e9 bases, not 0.0001'),
    ('length-inf', dict(length=float('inf')), 'length must lie in 1e-3 .. 1e9 bases, not inf'),
    ('want', dict(want=('status', 'nope')), 'want must name outputs of %s'),
    ('hoff-from-1', dict(hoff=CHAIN_HOFF + 1), 'hoff must start at 0 and never decrease'),
    ('hoff-down', dict(hoff=np.array([0, 2, 1, 3], np.int64)), 'hoff must start at 0 and never decrease'),
    ('hoff-short', dict(hoff=CHAIN_HOFF[:-1]), 'hoff must be int64[nreads + 1]'),
    ('hoff-long', dict(hoff=np.append(CHAIN_HOFF, 3)), 'hoff must be int64[nreads + 1]'),
]


@pytest.mark.parametrize('bad,kw,text', [pytest.param(*b, id=b[0]) for b in CHAIN_BAD])
@pytest.mark.parametrize('name,fn,outputs,has_chain', [pytest.param(*h, id=h[0]) for h in CHAIN_HOSTS])
def test_chain_hosts_refuse_alike_before_the_library(rec, name, fn, outputs, has_chain, bad, kw, text):
    if not has_chain and ('pi' in kw or 'length' in kw):
        with pytest.raises(TypeError):                                   # the class rows take neither
            fn(*CHAIN_READS, CHAIN_HOFF, **kw)
    else:
        with pytest.raises(ValueError) as e:
            fn(*CHAIN_READS, **dict(dict(hoff=CHAIN_HOFF), **kw))
        assert str(e.value) == (text % ', '.join(outputs) if '%s' in text else text)
    assert rec.calls == []


@pytest.mark.parametrize('name,fn,outputs,has_chain', [pytest.param(*h, id=h[0]) for h in CHAIN_HOSTS])
def test_chain_hosts_hand_the_same_reads_to_the_library(rec, name, fn, outputs, has_chain):
    """the counterpart: the well-formed call reaches its entry once, with the reads, hoff and nrows in the shared places"""
    res = fn(*CHAIN_READS, CHAIN_HOFF, want=outputs[:1], device=1)
    entry = {'hmm': 'nmod_read_hmm', 'viterbi': 'nmod_read_viterbi', 'grad': 'nmod_read_hmm_grad', 'class_rows': 'nmod_read_class_rows'}[name]
    got = rec.only(entry)
    assert len(got) == (12 if has_chain else 11) and got[1] == 3 and got[6] == 3 and got[8] == addr(res['hoff']) and got[9] == 3
    assert sorted(res) == sorted(('hoff',) + tuple(outputs[:1])) and np.array_equal(res['hoff'], CHAIN_HOFF)
    assert got[-1]['struct_size'] > 0 and (not has_chain or (got[-2]['pi'], got[-2]['length']) == (0.5, 200.0))
