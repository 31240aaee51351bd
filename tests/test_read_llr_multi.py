"""nmod_read_llr_multi (K26) without a GPU: the call rule against a brute-force enumeration, the softmax against mpmath out to u = +-700,
the restatement's planes being K13's, the conditions the shared inputs must meet, the declarations, struct layouts and the table
placement rule, and the argument checks of every layer (before any device work)."""
import ctypes as C
import itertools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import multi_ref as M
import readllr_ref as F
import rescale_ref as R
from nanomod_amd import _lib as L, engine
from nanomod_amd import readllr as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'nanomod_hip.h')
NO_SUCH_DEVICE = 99          # beyond any device count: NMOD_ERR_NO_DEVICE with or without a GPU in the machine
INVALID, NO_DEVICE = -1, -5
THR = 2.5
nan = float('nan')


# ------------------------------------------------------------------------------------------------------------------ the call rule
def _brute(Ls, thr):
    """the definition read as sets, not as a scan: the call of one event from its window sums (None: closed)"""
    open_ = {m: v for m, v in enumerate(Ls, 1) if v is not None}
    if not open_:
        return M.NONE
    top = max(open_.values())
    b = min(m for m, v in open_.items() if v == top)
    second = max([0.0] + [v for m, v in open_.items() if m != b])
    if open_[b] - second >= thr:
        return b
    if all(v <= -thr for v in open_.values()):
        return 0
    return M.AMBIGUOUS


GRID = (None, -6.0, -THR, np.nextafter(-THR, 0.0), -1.0, -0.0, 0.0, 1.0, np.nextafter(THR, 0.0), THR, 3.0, 3.0 + THR, 9.0)


@pytest.mark.parametrize('n_alt', [1, 2, 3, 4])
def test_call_rule_against_brute_force(n_alt):
    """every combination of 13 values per state (closed, on and beside both thresholds, both zeros, ties, a margin of exactly thr): the
    restated scan, its vectorised form and the definition read as sets agree; every call occurs"""
    combos = list(itertools.product(GRID, repeat=n_alt))
    Lm = np.array([[nan if v is None else v for v in c] for c in combos]).T
    want = np.array([_brute(c, THR) for c in combos], np.uint8)
    assert np.array_equal(M.joint_call(Lm, THR), want) and np.array_equal(M.joint_call_fast(Lm, THR), want)
    assert set(want.tolist()) == set(range(n_alt + 1)) | {M.AMBIGUOUS, M.NONE}
    if n_alt == 1:                                                           # K13's MOD / CAN rule exactly
        v = Lm[0]
        with np.errstate(invalid='ignore'):
            k13 = np.where(np.isnan(v), M.NONE, np.where(v >= THR, 1, np.where(v <= -THR, 0, M.AMBIGUOUS)))
        assert np.array_equal(want, k13)
    if n_alt >= 2:
        at = lambda *c: int(want[combos.index(tuple(c) + (None,) * (n_alt - 2))])
        assert at(3.0, 3.0) == M.AMBIGUOUS and at(3.0 + THR, 3.0) == 1 and at(3.0, 3.0 + THR) == 2      # a tie; a margin of exactly thr
        assert at(THR, -6.0) == 1 and at(-THR, -6.0) == 0 and at(-THR, -1.0) == M.AMBIGUOUS and at(None, 3.0) == 2 and at(None, -THR) == 0


# ------------------------------------------------------------------------------------------------------------------- the softmax
def test_softmax_against_mpmath():
    """post against 50-digit mpmath at u in {-700, -40, 0, 40, 700} per state, closed states among them: within 1e-13 relative where the
    value is a normal double, absolutely within DBL_MIN below; the planes sum to 1 within 4 ulp.  Measured: 4.4e-16 relative"""
    import mpmath as mp
    mp.mp.dps = 50
    us = (None, -700.0, -40.0, 0.0, 40.0, 700.0)
    worst = 0.0
    for n_alt in (1, 2, 3, 4):
        prior = np.array(M.PARITY_PRIORS[:n_alt])
        combos = [c for c in itertools.product(us, repeat=n_alt) if any(v is not None for v in c)]
        Lm = np.array([[nan if v is None else v for v in c] for c in combos]).T - prior[:, None]      # u = L + prior: +-700 to rounding
        post = M.posterior(Lm, prior)
        assert np.abs(post.sum(axis=0) - 1.0).max() <= 4 * 2.0 ** -52
        for j, c in enumerate(combos):
            u = [None if v is None else mp.mpf(float(Lm[m, j])) + mp.mpf(float(prior[m])) for m, v in enumerate(c)]
            e = [mp.mpf(1)] + [mp.mpf(0) if v is None else mp.exp(v) for v in u]
            Z = sum(e)
            for m in range(n_alt + 1):
                want, got = e[m] / Z, float(post[m, j])
                if want == 0:
                    assert got == 0.0
                elif want < F.DBL_MIN:
                    assert abs(got - float(want)) <= F.DBL_MIN
                else:
                    worst = max(worst, abs(float(got / want - 1)))
    print('softmax against mpmath: worst relative deviation %.3g' % worst)
    assert worst <= 1e-13
    gone = M.posterior(np.array([[nan], [nan]]), [0.0, 0.0])
    assert np.isnan(gone).all()


def test_n_alt_1_posterior_is_k13s():
    t = np.array([-800.0, -40.0, -1e-3, 0.0, 1e-3, 40.0, 800.0])
    post = M.posterior(t[None, :] - 0.375, [0.375])
    k13 = F.posterior((t - 0.375) + 0.375)
    assert np.allclose(post[1], k13, rtol=4 * 2.0 ** -52, atol=0.0) and np.allclose(post[0], 1.0 - k13, rtol=0, atol=2.0 ** -52)


# -------------------------------------------------------------------------------------------------------------- the shared inputs
@pytest.mark.parametrize('k,center,window', [(3, 1, (0, 0)), (3, 1, (1, 1)), (4, 1, (64, 64))])
def test_shared_inputs_meet_the_conditions(k, center, window):
    """the restatement's planes are readllr_ref's per pair; the open sets differ along a read and between the tables; every call occurs;
    both read classes and a read of 3 tiles per wave are there"""
    p = M.parity_inputs(k, center, window, 'float64')
    alts = p['alts']
    exp = M.restate(p['val'], p['off'], p['base'], k, center, p['mean'], p['sd'], alts, window, M.PARITY_THR, M.PARITY_PRIORS)
    for m, (m1, s1) in enumerate(alts):
        one = F.restate(p['val'], p['off'], p['base'], k, center, p['mean'], p['sd'], m1, s1, window, M.PARITY_THR, M.PARITY_PRIORS[m])
        assert exp['llr'][m].tobytes() == one['llr'].tobytes() and exp['llr_win'][m].tobytes() == one['llr_win'].tobytes()
    open_ = ~np.isnan(exp['llr_win'])
    masks = set(np.packbits(open_, axis=0, bitorder='little')[0].tolist())
    assert len(masks) >= 6 and 0 in masks and 15 in masks                    # closed in some tables and open in others, along the reads
    assert set(exp['call'].tolist()) == {0, 1, 2, 3, 4, M.AMBIGUOUS, M.NONE}
    lens = np.diff(p['off'])
    inner = M.inner_of(window)
    assert {1, 63, 64, 65, inner - 1, inner, inner + 1, M.WAVE_MAX - 1, M.WAVE_MAX, M.WAVE_MAX + 1} <= set(lens.tolist())
    assert lens.max() > 11 * inner and lens.max() <= 12 * inner              # 3 tiles per wave of the workgroup form
    assert np.array_equal(exp['n_sites'], [int(open_[:, a:b].any(axis=0).sum()) for a, b in zip(p['off'][:-1], p['off'][1:])])
    assert (exp['n_sites'] == exp['n_can'] + exp['n_mod'].sum(axis=0) + [int((exp['call'][a:b] == M.AMBIGUOUS).sum())
                                                                          for a, b in zip(p['off'][:-1], p['off'][1:])]).all()
    ok = ~np.isnan(exp['post'][0])
    assert np.abs(exp['post'][:, ok].sum(axis=0) - 1.0).max() <= 4 * 2.0 ** -52 and (exp['post'][1:][~open_ & ok[None, :]] == 0.0).all()


def test_parity_cases_cover_both_table_placements():
    lib = L.load()
    for n_alt in range(1, M.MULTI_MAX + 1):
        for k in range(1, 9):
            assert lib.nmod_read_llr_multi_table_in_lds(n_alt, k) == int(M.table_in_lds(n_alt, k)), (n_alt, k)
        ks = {c[1] for c in M.parity_cases() if c[0] == n_alt}
        assert any(M.table_in_lds(n_alt, k) for k in ks) and any(not M.table_in_lds(n_alt, k) for k in ks) and 3 in ks
        assert min(k for k in ks if not M.table_in_lds(n_alt, k)) == M.l2_side_k(n_alt)
    assert M.table_in_lds(1, 4) and not M.table_in_lds(1, 5)                 # K13's switch at one table
    assert lib.nmod_read_llr_multi_table_in_lds(0, 3) == -1 and lib.nmod_read_llr_multi_table_in_lds(5, 3) == -1 and lib.nmod_read_llr_multi_table_in_lds(2, 9) == -1


# ------------------------------------------------------------------------------------------------- declarations and struct layouts
def test_entries_are_declared_and_exported():
    lib = L.load()
    header = open(HEADER).read()
    declared = set(re.findall(r'\b(nmod_[a-z_]+)\s*\(', header))
    for name in ('nmod_read_llr_multi', 'nmod_read_llr_multi_table_in_lds', 'nmod_site_compose', 'nmod_site_compose_stage_reads'):
        assert name in declared and name in L._SIGNATURES and hasattr(lib, name)
    assert '#define NMOD_MULTI_MAX 4' in header and L.MULTI_MAX == M.MULTI_MAX == 4
    assert '#define NMOD_MULTI_AMBIGUOUS 255' in header and '#define NMOD_MULTI_NONE 254' in header
    assert (L.MULTI_AMBIGUOUS, L.MULTI_NONE) == (M.AMBIGUOUS, M.NONE) == (255, 254)
    assert '#define NMOD_ABI_VERSION 4' in header and lib.nmod_abi_version() == 4 == L.NMOD_ABI_VERSION      # purely additive entries
    import nanomod_amd
    assert nanomod_amd.read_llr_multi_host is engine.read_llr_multi_host and nanomod_amd.site_compose_host is engine.site_compose_host
    assert nanomod_amd.call_reads_llr_multi is RL.call_reads_llr_multi and nanomod_amd.write_site_compose is RL.write_site_compose


def test_struct_layouts_match_the_header():
    fields = [('nmod_llr_multi_opts', L.NmodLlrMultiOpts, ('struct_size', 'nb_lo', 'nb_hi', 'reserved', 'thr', 'prior_logit')),
              ('nmod_llr_multi_out', L.NmodLlrMultiOut, ('struct_size', 'reserved', 'llr', 'llr_win', 'post', 'call', 'n_sites', 'n_can', 'n_mod', 'status')),
              ('nmod_compose_opts', L.NmodComposeOpts, ('struct_size', 'max_iter', 'min_valid', 'reserved', 'tol')),
              ('nmod_compose_out', L.NmodComposeOut, ('struct_size', 'reserved', 'pi', 'll', 'stat', 'stat_m', 'p_m', 'n_valid', 'n_partial', 'iters',
                                                      'open_mask', 'status', 'resp'))]
    exprs, want = [], []
    for cname, cls, names in fields:
        exprs.append('sizeof(%s)' % cname); want.append(C.sizeof(cls))
        assert [n for n, _ in cls._fields_] == list(names)
        for n in names:
            exprs.append('offsetof(%s, %s)' % (cname, n)); want.append(getattr(cls, n).offset)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){size_t v[] = {%s};\nfor (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) ' \
          'printf("%%zu ", v[i]);\nreturn 0;}' % (HEADER, ', '.join(exprs))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, 't.c')
        open(c, 'w').write(src)
        subprocess.check_call(['gcc', c, '-o', os.path.join(d, 't')])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, 't')]).split()]
    assert got == want
    assert (C.sizeof(L.NmodLlrMultiOpts), C.sizeof(L.NmodLlrMultiOut), C.sizeof(L.NmodComposeOpts), C.sizeof(L.NmodComposeOut)) == (56, 72, 24, 96)


# ------------------------------------------------------------------------------------------------- the C entry's own refusals
def c_call(lib, nreads=3, *, device=NO_SUCH_DEVICE, n_alt=2, total=None, off='x', val='x', base='x', model='x', alt='x', alt_null=None, k=3, center=1,
           alt_k=None, alt_center=None, mean='x', sd='x', alt_mean='x', alt_sd='x', opts='x', out='x', nb_lo=2, nb_hi=1, thr=2.5,
           prior_logit=(0.0, 0.0, 0.0, 0.0), dtype=None, memspace=None, prm=None, opts_size=None, out_size=None):
    """nmod_read_llr_multi on three reads of 60 events with one argument changed; the return code.  (tests/test_read_llr_multi_gpu.py
    runs the same cases against a device that exists)"""
    n = nreads if 0 <= nreads < 1000 else 3
    offs = np.arange(n + 1, dtype=np.int64) * 60
    nev = max(n, 1) * 60
    x, b = np.zeros(nev, np.int16), np.full(nev, ord('A'), np.uint8)
    mu, s = np.zeros(4 ** 8), np.ones(4 ** 8)
    planes, cnt = np.zeros(5 * nev), np.zeros(4 * max(n, 1), np.int32)
    pick = lambda v, d: d.ctypes.data if isinstance(v, str) else (v.ctypes.data if v is not None else None)
    m0 = L.NmodRescaleModel()
    m0.k, m0.center, m0.mean, m0.sd = k, center, pick(mean, mu), pick(sd, s)
    ms = []
    for m in range(4):
        m1 = L.NmodRescaleModel()
        last = m == max(min(n_alt, 4), 1) - 1                                # the changed table is the last one the call reads
        m1.k, m1.center = (k if alt_k is None or not last else alt_k), (center if alt_center is None or not last else alt_center)
        m1.mean, m1.sd = (pick(alt_mean, mu) if last else mu.ctypes.data), (pick(alt_sd, s) if last else s.ctypes.data)
        ms.append(m1)
    arr = L.model_ptr_array(ms)
    if alt_null is not None:
        arr[alt_null] = None
    o = L.make_llr_multi_opts(nb_lo, nb_hi, thr, prior_logit)
    if opts_size is not None:
        o.struct_size = opts_size
    r = L.make_llr_multi_out(llr_win=planes.ctypes.data, n_sites=cnt.ctypes.data, n_mod=cnt.ctypes.data)
    if out_size is not None:
        r.struct_size = out_size
    if prm is None:
        prm = L.make_params(device=device, memspace=L.MEM_HOST if memspace is None else memspace, dtype=L.DTYPE_I16_MILLI if dtype is None else dtype)
    return lib.nmod_read_llr_multi(C.byref(prm), nreads, nev if total is None else total, pick(off, offs), pick(val, x), pick(base, b),
                                   C.byref(m0) if model is not None else None, n_alt, C.addressof(arr) if alt is not None else None,
                                   C.byref(o) if opts is not None else None, C.byref(r) if out is not None else None)


def refused_c_cases():
    """(name, keyword arguments of c_call) of every refusal the header lists"""
    inf = float('inf')
    cases = [('nb_lo_neg', dict(nb_lo=-1)), ('nb_lo_65', dict(nb_lo=65)), ('nb_hi_neg', dict(nb_hi=-1)), ('nb_hi_65', dict(nb_hi=65))]
    cases += [('thr_%r' % v, dict(thr=v)) for v in (0.0, -2.5, nan, inf, -inf)]
    cases += [('prior_%r_%d' % (v, m), dict(prior_logit=tuple(v if i == m else 0.0 for i in range(4)))) for v in (700.0000001, -701.0, nan, inf) for m in (0, 1)]
    cases += [('n_alt_%d' % v, dict(n_alt=v)) for v in (0, -1, 5, 100)]
    cases += [('alt_null', dict(alt=None)), ('alt_entry_null_0', dict(alt_null=0)), ('alt_entry_null_1', dict(alt_null=1))]
    cases += [('alt_k', dict(alt_k=4)), ('alt_center_0', dict(alt_center=0)), ('alt_center_2', dict(alt_center=2)),
              ('alt_k_third', dict(n_alt=3, alt_k=2)), ('alt_center_fourth', dict(n_alt=4, alt_center=0))]
    cases += [('k_0', dict(k=0, center=0)), ('k_9', dict(k=9)), ('center_3', dict(center=3)), ('center_neg', dict(center=-1))]
    cases += [(name + '_null', {name: None}) for name in ('off', 'val', 'base', 'model', 'mean', 'sd', 'alt_mean', 'alt_sd', 'opts', 'out')]
    cases += [('opts_size_48', dict(opts_size=48)), ('opts_size_64', dict(opts_size=64)), ('out_size_64', dict(out_size=64)), ('out_size_80', dict(out_size=80))]
    cases += [('dtype_3', dict(dtype=3)), ('dtype_neg', dict(dtype=-1)), ('memspace_2', dict(memspace=2))]
    cases += [('nreads_neg', dict(nreads=-1)), ('nreads_2_32', dict(nreads=2 ** 32 - 1)), ('total_neg', dict(total=-1)), ('total_short', dict(total=179))]
    cases += [('off_down', dict(off=np.array([0, 60, 40, 180], np.int64))), ('off_neg', dict(off=np.array([-1, 60, 120, 180], np.int64)))]
    return cases


def test_read_llr_multi_refuses_invalid_arguments_before_any_device_work():
    """every case of the header returns NMOD_ERR_INVALID_ARG although the device does not exist (which alone is NMOD_ERR_NO_DEVICE)"""
    lib = L.load()
    call = lambda *a, **kw: c_call(lib, *a, **kw)
    assert call() == NO_DEVICE                                               # the well-formed call reaches the device check
    assert all(call(n_alt=v) == NO_DEVICE for v in (1, 2, 3, 4)) and call(memspace=L.MEM_DEVICE) == NO_DEVICE
    assert call(prior_logit=(700.0, -700.0, 0.0, 0.0)) == NO_DEVICE and call(n_alt=1, prior_logit=(0.0, nan, nan, nan)) == NO_DEVICE   # beyond n_alt: not read
    assert call(n_alt=1, alt_null=1) == NO_DEVICE and call(total=180) == NO_DEVICE and call(total=10 ** 6) == NO_DEVICE
    assert call(memspace=L.MEM_DEVICE, total=0) == NO_DEVICE                 # (a device call's offsets are not the host's to read)
    assert call(0) == 0 and call(0, off=None, val=None, base=None, mean=None, sd=None, alt_mean=None, alt_sd=None) == 0   # no reads: no device needed
    for name, kw in refused_c_cases():
        kw = dict(kw)
        assert call(kw.pop('nreads', 3), **kw) == INVALID, name
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert call(prm=bad) == INVALID
    assert lib.nmod_read_llr_multi(None, 3, 180, None, None, None, None, 2, None, None, None) == INVALID


# --------------------------------------------------------------------------------------------- the Python layers: refusals
def _reads(first=0, dtype=np.float32, tail=2):
    off = first + np.arange(4, dtype=np.int64) * 6
    n = int(off[-1]) + tail
    val = np.random.default_rng(3).normal(size=n).astype(dtype)
    return val, off, np.frombuffer(b'ACGT' * n, np.uint8)[:n].copy()


def _models(k=3, center=1, n_alt=2):
    mean, sd = R.make_model(k, holes=False)
    return dict(k=k, center=center, mean=mean, sd=sd), [dict(k=k, center=center, mean=mean + 0.5 * (m + 1), sd=sd * 1.5) for m in range(n_alt)]


def _refused_host():
    val, off, base = _reads()
    m0, alts = _models()
    inf = float('inf')
    w = lambda **kw: ((kw.pop('val', val), kw.pop('off', off), kw.pop('base', base), kw.pop('model', m0), kw.pop('alts', alts)), kw)
    cases = dict(
        lo_neg=w(window=(-1, 0)), lo_65=w(window=(65, 0)), hi_65=w(window=(0, 65)), window_word=w(window='cover'), window_none=w(window=None),
        thr_0=w(thr=0.0), thr_nan=w(thr=nan), thr_inf=w(thr=inf),
        prior_nan=w(prior_logit=(0.0, nan)), prior_701=w(prior_logit=(701.0, 0.0)), prior_count=w(prior_logit=(0.0,)), prior_three=w(prior_logit=(0.0, 0.0, 0.0)),
        no_alts=w(alts=[]), five_alts=w(alts=_models(n_alt=5)[1]), alt_none=w(alts=[alts[0], None]), alts_none=w(alts=None), no_model=w(model=None),
        k_0=w(model=dict(m0, k=0), alts=[dict(a, k=0) for a in alts]), center_3=w(model=dict(m0, center=3), alts=[dict(a, center=3) for a in alts]),
        k_differs=w(alts=[alts[0], _models(2, 1)[1][0]]), center_differs=w(alts=[alts[0], dict(alts[1], center=0)]),
        want=w(want=('p_mod',)), dtype=w(val=val.astype(np.int32)), off_down=w(off=np.array([0, 12, 6, 18], np.int64)), off_past=w(off=off + 4),
        base_short=w(base=base[:int(off[-1]) - 1]), alt_sd_len=w(alts=[alts[0], dict(alts[1], sd=np.ones(16))]))
    return [pytest.param(a, kw, id=name) for name, (a, kw) in cases.items()]


@pytest.mark.parametrize('args,kw', _refused_host())
def test_refused_before_the_library(args, kw):
    L.load()                                     # the real library: a call that reached it would be a NanomodLibraryError
    with pytest.raises((ValueError, TypeError)) as e:
        engine.read_llr_multi_host(*args, device=NO_SUCH_DEVICE, **kw)
    assert e.type is ValueError or kw == {} and args[4] is None              # (alts=None: not a sequence)


def test_accepted_calls_reach_the_library():
    val, off, base = _reads()
    m0, alts = _models()
    with pytest.raises(L.NanomodLibraryError, match='nmod_read_llr_multi'):
        engine.read_llr_multi_host(val, off, base, m0, alts, device=NO_SUCH_DEVICE)
    res = engine.read_llr_multi_host(val[:0], np.zeros(1, np.int64), base[:0], m0, alts, want=('llr_win', 'call'), device=NO_SUCH_DEVICE)   # no reads: no device
    assert res['llr_win'].shape == (2, 0) and res['call'].shape == (0,) and res['n_mod'].shape == (2, 0) and 'post' not in res


def test_call_reads_llr_multi_refuses_before_any_device_work():
    reads, model, alts, _ = M.chain_inputs(n_reads=4)
    call = lambda **kw: RL.call_reads_llr_multi(kw.pop('reads', reads), kw.pop('model', model), kw.pop('alts', alts), device=NO_SUCH_DEVICE, log=None, **kw)
    a0 = alts[0]
    for kw, msg in ((dict(alts=[a0, dict(a0, k=2, mean=a0['mean'][:16], sd=a0['sd'][:16], n_positions=a0['n_positions'][:16])]), 'share k and center'),
                    (dict(alts=[]), 'alternative models'), (dict(alts=alts * 3), 'alternative models'),
                    (dict(names=['a']), 'names'), (dict(names=['a', 'a']), 'names'), (dict(names=['a', 'b c']), 'names'), (dict(names=['can', 'b']), 'names'),
                    (dict(priors=[0.5]), 'priors'), (dict(priors=[0.5, 0.5]), 'priors'), (dict(priors=[0.0, 0.1]), 'priors'),
                    (dict(thr=0.0), 'thr'), (dict(window=(65, 0)), 'window'), (dict(rescale=dict(bogus=1)), 'rescale'),
                    (dict(compose=dict(bogus=1)), 'compose'), (dict(compose=dict(max_iter=0)), 'max_iter'), (dict(compose=dict(tol=-1.0)), 'tol'),
                    (dict(compose=dict(min_valid=0)), 'min_valid'), (dict(fdr='bh'), 'compose'), (dict(compose={}, fdr='holm'), 'method|fdr'),
                    (dict(reads={k: v for k, v in reads.items() if k != 'base'}), 'read-level')):
        with pytest.raises(ValueError, match=msg):
            call(**kw)


def test_cli_parser_and_checks(capsys):
    from nanomod_amd import cli
    p = cli.build_parser()
    base = ['readllr', '--wrkBase1', HEADER, '--kmerModel', HEADER]
    a = p.parse_args(base + ['--altModel', 'a.npz'])
    assert (a.modNames, a.modPrior, a.siteCompose, a.fdr, a.composeMaxIter, a.composeTol) == ('', '', 0, 'none', 500, 1e-9)
    assert cli.parse_mod_prior('0.3,0.1', 2) == [0.3, 0.1] and cli.parse_mod_prior('0.3', 2) is None and cli.parse_mod_prior('0.6,0.4', 2) is None
    assert cli.parse_mod_prior('0.3,x', 2) is None and cli.parse_mod_prior('0,0.1', 2) is None
    two = HEADER + ',' + HEADER
    bad = lambda *more: [e for e in cli.validate_readllr(p.parse_args(base + list(more))) if 'read-level' not in e]
    assert bad('--altModel', two) == [] and bad('--altModel', two, '--siteCompose', '1', '--fdr', 'bh', '--modNames', 'm6A,m5C', '--modPrior', '0.3,0.1') == []
    assert bad('--altModel', HEADER) == []
    for more, word in ((('--altModel', HEADER, '--siteCompose', '1'), 'several'), (('--altModel', HEADER, '--modNames', 'a'), 'several'),
                       (('--altModel', HEADER, '--fdr', 'bh'), 'several'), (('--altModel', ','.join([HEADER] * 5)), 'at most'),
                       (('--altModel', two, '--modNames', 'a'), '--modNames'), (('--altModel', two, '--modPrior', '0.9,0.2'), '--modPrior'),
                       (('--altModel', two, '--fdr', 'bh'), '--siteCompose'), (('--altModel', two, '--siteFraction', '1'), 'single'),
                       (('--altModel', two, '--siteCompose', '1', '--composeMaxIter', '0'), '--composeMaxIter'),
                       (('--altModel', two, '--siteCompose', '1', '--composeTol', '-1'), '--composeTol'),
                       (('--altModel', two + ',/nonexistent/b.npz'), 'does not exist')):
        errs = bad(*more)
        assert len(errs) == 1 and word in errs[0], (more, errs)
    capsys.readouterr()


def test_writers(tmp_path):
    table = dict(index=np.arange(2), chrom=np.array(['chr1', 'chr2']), strand=np.array(['+', '-']), start=np.array([5, 70], np.int64),
                 events=np.array([200, 1]), n_sites=np.array([198, 0], np.int32), n_can=np.array([150, 0], np.int32),
                 n_mod_m6A=np.array([4, 0], np.int32), n_mod_m5C=np.array([31, 0], np.int32), status=np.array([0, 16], np.uint8), names=['m6A', 'm5C'])
    path = str(tmp_path / 'r.txt')
    RL.write_read_llr_multi(path, table)
    assert open(path).read() == ('#index chrom strand start events n_sites n_can n_mod_m6A n_mod_m5C status\n'
                                 '0 chr1 + 5 200 198 150 4 31 0\n1 chr2 - 70 1 0 0 0 0 16\n')
    sites = dict(chrom=np.array(['chr1', 'chr1']), strand=np.array(['+', '+']), pos=np.array([9, 10]), base=np.array(['A', 'C']),
                 n_reads=np.array([30, 2], np.int32), n_valid=np.array([28, 0], np.int32), n_can=np.array([10, 0], np.int32),
                 n_m6A=np.array([12, 0], np.int32), n_m5C=np.array([1, 0], np.int32), n_ambiguous=np.array([5, 0], np.int32), names=['m6A', 'm5C'])
    RL.write_site_llr_multi(path, sites)
    assert open(path).read() == ('#chrom strand pos base n_reads n_valid n_can n_m6A n_m5C n_ambiguous\n'
                                 'chr1 + 10 A 30 28 10 12 1 5\nchr1 + 11 C 2 0 0 0 0 0\n')
    sites.update(n_fit=np.array([28, 0], np.int32), n_partial=np.array([0, 0], np.int32), pi_can=np.array([0.5, nan]), pi_m6A=np.array([0.45, nan]),
                 stat_m6A=np.array([30.25, nan]), p_m6A=np.array([1.9e-8, nan]), pi_m5C=np.array([0.05, nan]), stat_m5C=np.array([0.0, nan]),
                 p_m5C=np.array([1.0, nan]), ll=np.array([15.5, nan]), stat=np.array([31.0, nan]), iters=np.array([40, 0], np.int32),
                 open_mask=np.array([3, 0], np.uint8), compose_status=np.array([0, 2], np.uint8))
    RL.write_site_compose(path, sites)
    assert open(path).read() == ('#chrom strand pos base n_reads n_fit n_partial pi_can pi_m6A stat_m6A p_m6A pi_m5C stat_m5C p_m5C ll stat iters open_mask status\n'
                                 'chr1 + 10 A 30 28 0 0.500000 0.450000 30.250 1.900E-08 0.050000 0.000 1.000E+00 15.500000 31.000 40 3 0\n'
                                 'chr1 + 11 C 2 0 0 nan nan nan nan nan nan nan nan nan 0 0 2\n')
    sites.update(q_m6A=np.array([3.8e-8, nan]), q_m5C=np.array([1.0, nan]))
    RL.write_site_compose(path, sites)
    lines = open(path).read().splitlines()
    assert lines[0].split()[8:12] == ['pi_m6A', 'stat_m6A', 'p_m6A', 'q_m6A'] and lines[1].split()[8:12] == ['0.450000', '30.250', '1.900E-08', '3.800E-08']
