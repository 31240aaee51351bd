"""nmod_rep_prior and nmod_site_diff_rep_mod (K25) on the GPU against the numpy restatement of their definitions (tests/diff_mod_ref.py,
pinned against mpmath in tests/test_site_diff_mod.py) and against nmod_site_diff_rep, whose bytes everything but phi_post, p_rep and
the interval must keep: the prior over the sizes at which its sums take another path, every excluded kind of site interleaved, the
three cases of the solve and the bits of the record; the moderated entry under a d0 = 0 record byte for byte against K24, under a
finite fractional prior and under d0 = inf against the restatement; the records that cannot be used; the independence of a site's
bits from the batch; the refusals of both entries; the stream contract of the three-call chain; the read-level chain and the
command line.  The gates are diff_mod_ref's."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import diff_mod_ref as M
import diff_rep_ref as R
import stoich_ref as SR
from nanomod_amd import _lib as L
from nanomod_amd import engine
from nanomod_amd.engine import rep_prior_host, site_diff_rep_host          # rep_prior_host is K25's: without it nothing here can pass

pytestmark = pytest.mark.gpu

CHUNK = L.REP_PRIOR_CHUNK
UNCHANGED = ('pi_s', 'n_valid', 'pi0', 'pi1', 'pi_pool', 'delta', 'stat_cond', 'p_cond', 'stat_het', 'p_het', 'phi', 'iters')


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _rec_bits(p):
    return _bits(engine.rep_prior_record(p))


# ------------------------------------------------------------------------------------------------------------------------ the prior
def _phi_case(npos, df, kind, seed):
    """phi and status of npos sites.  'mixed': phi = s0^2 F(df, 8) with s0^2 = 2.5; 'spread': log-normal over e^+-3 (a small d0);
    'equal': one value (evar < 0: d0 = inf).  From site 2 on every kind of site the fit leaves out is interleaved: the three
    no-estimate bits (with a NaN and with a usable phi behind them), zeros, -0.0, NaN, +inf and a negative phi with an estimate; the
    bits that keep a site in (NOT_CONVERGED, POOL_AT_END, PHI_ZERO) are spread over the rest"""
    rng = np.random.default_rng(seed)
    if kind == 'equal':
        phi = np.full(npos, 1.7)
    elif kind == 'spread':
        phi = np.exp(rng.normal(0.0, 3.0, npos))
    else:
        phi = 2.5 * (rng.chisquare(df, npos) / df) / (rng.chisquare(8, npos) / 8)
    status = np.zeros(npos, np.uint8)
    i = np.arange(npos)
    free = i >= 2
    status[free & (i % 17 == 3)] = R.NOT_CONVERGED | R.POOL_AT_END
    status[free & (i % 19 == 4)] = R.PHI_ZERO
    for m, r, st, v in ((7, 2, R.TOO_FEW, np.nan), (11, 5, R.FLAT, 3.0), (13, 6, R.TOO_LARGE, np.nan), (23, 7, R.TOO_FEW | R.NOT_CONVERGED, 0.0),
                        (5, 4, 0, 0.0), (29, 9, 0, -0.0), (31, 10, 0, np.nan), (37, 11, 0, np.inf), (41, 12, R.POOL_AT_END, -1.5)):
        sel = free & (i % m == r % m)
        status[sel] = st
        phi[sel] = v
    return phi, status


def _big():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 4 * CHUNK + CHUNK + 1      # beyond the persistent grid x chunk


def _check_prior(got, phi, status, df, level=0.95):
    p = M.rep_prior(phi, status, df, level)
    g = M.prior_gates(p, df, level)
    assert got['n_used'] == p['n_used'] and got['n_zero'] == p['n_zero'], (got, p['n_used'], p['n_zero'])
    n = int(p['n_used'])
    print('n %d, zeros %d; emean %r (off by %.3g, gate %.3g); evar %r (off by %.3g, gate %.3g); d0 %r (%r), s0sq %r (%r), ci_drop %r (%r)'
          % (n, p['n_zero'], got['emean'], abs(got['emean'] - p['emean']), g['emean'], got['evar'], abs(got['evar'] - p['evar']), g['evar'],
             got['d0'], p['d0'], got['s0sq'], p['s0sq'], got['ci_drop'], p['ci_drop']))
    if n == 0:
        assert math.isnan(got['emean'])
    else:
        assert abs(got['emean'] - p['emean']) <= g['emean']
    if n < 2:
        assert got['d0'] == 0.0 and math.isnan(got['s0sq']) and math.isnan(got['evar']) and got['df_tot'] == df
    else:
        assert abs(got['evar'] - p['evar']) <= g['evar']
        assert abs(p['evar']) > 4.0 * g['evar'], 'the case sits on the step between a finite d0 and inf'
        if math.isinf(p['d0']):
            assert got['d0'] == math.inf and got['df_tot'] == math.inf
        else:
            assert abs(got['d0'] - p['d0']) <= g['d0'] and got['df_tot'] == df + got['d0']
        assert abs(got['s0sq'] - p['s0sq']) <= g['s0sq']
    assert abs(got['ci_drop'] - p['ci_drop']) <= g['ci_drop']
    return p


PRIOR_CASES = [(0, 4, 'mixed'), (1, 1, 'mixed'), (2, 2, 'mixed'), (CHUNK - 1, 14, 'mixed'), (CHUNK, 1, 'mixed'), (CHUNK + 1, 2, 'mixed'),
               ('big', 4, 'mixed'), (3 * CHUNK + 5, 2, 'equal'), (2 * CHUNK + 77, 1, 'spread'), (300, 14, 'spread'), (300, 14, 'equal')]


@pytest.mark.parametrize('npos,df,kind', PRIOR_CASES, ids=lambda v: str(v))
def test_rep_prior_against_the_restatement(npos, df, kind):
    import torch
    npos = _big() if npos == 'big' else npos
    phi, status = _phi_case(npos, df, kind, 2500 + df)
    level = (0.95, 0.9, 0.999)[df % 3]
    got = rep_prior_host(phi, status, df, ci_level=level)
    p = _check_prior(got, phi, status, df, level)
    if kind == 'equal':
        assert p['evar'] < 0.0 and got['d0'] == math.inf
    if kind == 'spread':
        assert 0.0 < got['d0'] < 3.0
    if npos > 40:
        assert p['n_zero'] > 0 and 0 < p['n_used'] < npos - p['n_zero']
    # the bits: again, in device memory, and the same arrays at another address
    assert _rec_bits(rep_prior_host(phi, status, df, ci_level=level)) == _rec_bits(got)
    det = engine.DeviceDetector(0)
    d_phi, d_st = torch.from_numpy(phi).cuda(), torch.from_numpy(status).cuda()
    dev = det.rep_prior(d_phi, d_st, df, ci_level=level)
    pad_phi, pad_st = torch.empty(npos + 3, dtype=torch.float64, device='cuda'), torch.empty(npos + 3, dtype=torch.uint8, device='cuda')
    pad_phi[3:] = d_phi
    pad_st[3:] = d_st
    moved = det.rep_prior(pad_phi[3:], pad_st[3:], df, ci_level=level)
    torch.cuda.synchronize()
    assert _bits(dev.cpu().numpy()) == _rec_bits(got) and _bits(moved.cpu().numpy()) == _rec_bits(got)


def test_the_prior_recovers_a_planted_law():
    """20 000 sites of s0^2 F(4, 6) with s0^2 = 2: d0 and s0^2 come back within the sampling error of the moment fit"""
    rng = np.random.default_rng(2520)
    n = 20000
    phi = 2.0 * (rng.chisquare(4, n) / 4) / (rng.chisquare(6, n) / 6)
    got = rep_prior_host(phi, np.zeros(n, np.uint8), 4)
    _check_prior(got, phi, np.zeros(n, np.uint8), 4)
    assert abs(got['d0'] - 6.0) < 0.6 and abs(got['s0sq'] - 2.0) < 0.1 and got['n_used'] == n and got['n_zero'] == 0


# --------------------------------------------------------------------------------------------------------------- the moderated entry
def _drop(G):
    return engine._f1_quantile(0.95, G - 2)


def _no_prior(G):
    return np.array([0.0, np.nan, G - 2.0, _drop(G), 0.0, 0.0, np.nan, np.nan])


def _priors(G):
    """a finite fractional prior and d0 = inf, with the quantiles the restatement gives"""
    df = G - 2
    return (np.array([3.7, 1.3, df + 3.7, M.f1_quantile(0.95, df + 3.7), 50.0, 1.0, 0.1, 0.4]),
            np.array([np.inf, 0.8, np.inf, M.f1_quantile(0.95, np.inf), 50.0, 0.0, -0.2, -0.1]))


@pytest.mark.parametrize('key', R.CONFIGS, ids=lambda k: 'G%d_nc%d' % k)
def test_a_record_without_a_prior_gives_k24s_bytes(key):
    G, nc = key
    score, off = R.csr(R.length_batches()[key])
    plain = site_diff_rep_host(score, off, G, nc, min_valid=R.LENGTH_MIN_VALID)
    mod = site_diff_rep_host(score, off, G, nc, min_valid=R.LENGTH_MIN_VALID, prior=_no_prior(G), ci_level=0.5)    # (ci_level: ignored)
    assert set(mod) == set(plain) | {'phi_post'}
    for f in plain:
        assert _bits(mod[f]) == _bits(plain[f]), f
    assert _bits(mod['phi_post']) == _bits(plain['phi'])
    assert ((plain['status'] & L.REP_NO_ESTIMATE) == 0).sum() >= 3


def _check_mod(got, plain, exp, G, worst):
    """the unchanged members byte for byte against K24; status exactly; phi_post, p_rep and the interval within the gates"""
    for f in UNCHANGED:
        assert _bits(got[f]) == _bits(plain[f]), f
    est = 0
    for i, e in enumerate(exp):
        assert int(got['status'][i]) == e['status'], (i, got['status'][i], e['status'])
        if e['gates'] is None:
            assert all(np.isnan(got[f][i]) for f in ('phi_post', 'p_rep', 'delta_lo', 'delta_hi')), i
            continue
        est += 1
        g = e['gates']
        dev = abs(got['phi_post'][i] - e['phi_post'])
        assert dev <= g['phi_post'], (i, got['phi_post'][i], e['phi_post'], g['phi_post'])
        if g['phi_post'] > 0.0:
            worst['phi_post'] = max(worst.get('phi_post', 0.0), dev / g['phi_post'])
        lo, hi = g['p_rep']
        assert lo <= got['p_rep'][i] <= hi, (i, lo, got['p_rep'][i], hi)
        assert -1.0 <= got['delta_lo'][i] <= got['delta'][i] <= got['delta_hi'][i] <= 1.0, i
        assert (got['delta_lo'][i] == -1.0) == (e['delta_lo'] == -1.0) and (got['delta_hi'][i] == 1.0) == (e['delta_hi'] == 1.0), i
        for f in ('delta_lo', 'delta_hi'):
            dev = abs(got[f][i] - e[f])
            assert dev <= g[f], (i, f, got[f][i], e[f], g[f])
            if g[f] > 0.0:
                worst[f] = max(worst.get(f, 0.0), dev / g[f])
    return est


@pytest.mark.parametrize('key', R.CONFIGS, ids=lambda k: 'G%d_nc%d' % k)
def test_parity_over_the_lengths_under_a_prior(key):
    G, nc = key
    score, off = R.csr(R.length_batches()[key])
    plain = site_diff_rep_host(score, off, G, nc, min_valid=R.LENGTH_MIN_VALID)
    worst = {}
    for prior in _priors(G):
        exp = M.expected('length', key, tuple(prior.tolist()), 0.0, _drop(G))
        got = site_diff_rep_host(score, off, G, nc, min_valid=R.LENGTH_MIN_VALID, prior=prior)
        est = _check_mod(got, plain, exp, G, worst)
        assert 4 * est >= 3 * len(exp)
        assert not (got['status'] & M.BAD_PRIOR).any()
    print('worst deviation as a share of its gate: %s' % ', '.join('%s %.3g' % kv for kv in sorted(worst.items())))


@pytest.mark.parametrize('phi_floor', [0.0, 1.0])
def test_content_under_a_prior(phi_floor):
    sites = R.content_sites()
    score, off = R.csr(sites)
    plain = site_diff_rep_host(score, off, 4, 2, phi_floor=phi_floor)
    zero_s0 = np.array([np.inf, 0.0, np.inf, M.f1_quantile(0.95, np.inf), 9.0, 0.0, 0.0, -1.0])          # s0^2 = 0: PHI_ZERO at floor 0
    worst = {}
    for prior in _priors(4) + (zero_s0,):
        exp = M.expected('content', None, tuple(prior.tolist()), phi_floor, _drop(4))
        got = site_diff_rep_host(score, off, 4, 2, phi_floor=phi_floor, prior=prior)
        assert _check_mod(got, plain, exp, 4, worst) >= 20
        zero = (got['status'] & R.PHI_ZERO) != 0
        if prior[1] == 0.0 and phi_floor == 0.0:
            assert zero.sum() >= 15 and (got['p_rep'][zero] == R.DBL_MIN).all() and (got['phi_post'][zero] == 0.0).all()
            assert _bits(got['delta_lo'][zero]) == _bits(got['delta'][zero]) == _bits(got['delta_hi'][zero])
        else:
            assert not zero.any()                               # (K24's own PHI_ZERO site has a positive posterior dispersion, or the floor)
    i = next(i for i, rows in enumerate(sites) if all((np.abs(r) == 40.0).all() for r in rows))
    assert plain['phi'][i] == 0.0 and bool(plain['status'][i] & R.PHI_ZERO) == (phi_floor == 0.0)
    print('worst deviation as a share of its gate: %s' % ', '.join('%s %.3g' % kv for kv in sorted(worst.items())))


def test_a_record_that_cannot_be_used():
    sites = R.content_sites()
    score, off = R.csr(sites)
    plain = site_diff_rep_host(score, off, 4, 2)
    ok = _priors(4)[0]
    nan = np.nan
    for word, v in ((0, nan), (2, nan), (1, nan), (0, -1.0), (1, -0.5), (2, -2.0), (3, -3.84)):
        prior = ok.copy()
        prior[word] = v
        assert M.prior_bad(prior)
        got = site_diff_rep_host(score, off, 4, 2, prior=prior)
        exp = M.expected('content', None, tuple(prior.tolist()), 0.0, _drop(4))
        for f in UNCHANGED:
            assert _bits(got[f]) == _bits(plain[f]), (word, v, f)
        assert got['status'].tolist() == [e['status'] for e in exp] == ((plain['status'] & ~np.uint8(R.PHI_ZERO)) | M.BAD_PRIOR).tolist()
        assert all(np.isnan(got[f]).all() for f in ('p_rep', 'phi_post', 'delta_lo', 'delta_hi')), (word, v)
    # a NaN s0^2 that is not used (d0 = 0), and an infinite quantile, are no such record
    got = site_diff_rep_host(score, off, 4, 2, prior=_no_prior(4))
    assert not (got['status'] & M.BAD_PRIOR).any()
    wide = ok.copy()
    wide[3] = np.inf
    got = site_diff_rep_host(score, off, 4, 2, prior=wide)
    est = (got['status'] & L.REP_NO_ESTIMATE) == 0
    assert not (got['status'] & M.BAD_PRIOR).any() and (got['delta_lo'][est] == -1.0).all() and (got['delta_hi'][est] == 1.0).all()


def test_a_sites_bits_depend_on_its_rows_and_the_record_alone():
    """a shuffled batch, every site alone, device memory, fewer outputs; then about 40 000 sites, more than the persistent grids walk
    at once, every site equal to the same site computed alone"""
    import torch
    G, nc = 4, 2
    sites = R.length_batches()[(G, nc)]
    kw = dict(min_valid=R.LENGTH_MIN_VALID, prior=_priors(G)[0])
    full = site_diff_rep_host(*R.csr(sites), G, nc, **kw)
    n = len(sites)

    def same(res, idx, what):
        for f, v in res.items():
            w = G if f in ('pi_s', 'n_valid') else 1
            assert _bits(np.asarray(v).reshape(-1, w)) == _bits(full[f].reshape(-1, w)[idx]), (what, f)
    order = np.random.default_rng(2530).permutation(n).tolist()
    same(site_diff_rep_host(*R.csr([sites[i] for i in order]), G, nc, **kw), order, 'shuffled')
    for i in (0, n // 2, n - 1):
        same(site_diff_rep_host(*R.csr([sites[i]]), G, nc, **kw), [i], 'alone %d' % i)
    same(site_diff_rep_host(*R.csr(sites), G, nc, interval=False, **kw), list(range(n)), 'no interval')
    det = engine.DeviceDetector(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    score, off = R.csr(sites)
    dev = det.site_diff_rep(t(score), t(off), G, nc, min_valid=R.LENGTH_MIN_VALID, prior=t(kw['prior']))
    same({f: v.cpu().numpy() for f, v in dev.items()}, list(range(n)), 'device')
    # the large batch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nsites, kinds, G, nc = max(40000, cus * 8 * 16 + 37), 5, 3, 1
    rng = np.random.default_rng(2531)
    prior = _priors(G)[0]
    kind = [[SR.simulate_row(rng, 4, 3.0, p) for p in (0.3 + 0.1 * k, 0.5, 0.8 - 0.1 * k)] for k in range(kinds)]
    alone = [site_diff_rep_host(*R.csr([rows]), G, nc, prior=prior) for rows in kind]
    assert sum(a['status'][0] & L.REP_NO_ESTIMATE == 0 for a in alone) >= 4
    which = rng.integers(0, kinds, nsites)
    flat = np.stack([np.concatenate(rows) for rows in kind])[which].reshape(-1)
    got = site_diff_rep_host(flat, np.arange(0, 4 * G * nsites + 1, 4, dtype=np.int64), G, nc, prior=prior)
    for f in got:
        w = G if f in ('pi_s', 'n_valid') else 1
        ref = np.stack([a[f] for a in alone])[which].reshape(-1)
        assert ref.shape == (nsites * w,) and _bits(got[f]) == _bits(ref), f


def test_refusals_of_both_c_entries():
    lib = L.load()
    OK, INVALID = 0, -1                                         # NMOD_OK, NMOD_ERR_INVALID_ARG (include/nanomod_hip.h)
    prm = L.make_params(device=0, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    phi, status, rec = np.array([1.0, 2.0, 0.5]), np.zeros(3, np.uint8), np.full(8, -7.0)
    ptr = engine._np_ptr

    def rp(npos=3, df=2, phi=phi, status=status, level=0.95, rec=rec, prm=prm):
        return lib.nmod_rep_prior(C.byref(prm) if prm is not None else None, npos, df, ptr(phi) if phi is not None else None,
                                  ptr(status) if status is not None else None, level, ptr(rec) if rec is not None else None)
    assert rp() == OK and rec[4] == 3.0 and rec[0] != -7.0
    for bad in (dict(df=0), dict(df=15), dict(level=0.0), dict(level=1.0), dict(level=math.nan), dict(npos=-1), dict(phi=None), dict(status=None),
                dict(rec=None), dict(prm=None)):
        before = rec.copy()
        assert rp(**bad) == INVALID, bad
        assert _bits(before) == _bits(rec)
    short = L.make_params(device=0, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    short.struct_size -= 8
    assert rp(prm=short) == INVALID
    rec[:] = -7.0
    assert rp(npos=0, phi=None, status=None) == OK                                   # the n < 2 record
    assert rec[0] == 0.0 and math.isnan(rec[1]) and rec[2] == 2.0 and abs(rec[3] - M.f1_quantile(0.95, 2)) <= 1e-9 * rec[3]
    assert rec[4] == 0.0 and rec[5] == 0.0 and math.isnan(rec[6]) and math.isnan(rec[7])
    # the moderated entry: K24's refusals and a NULL prior
    score = np.array([1.0, -1.0, 2.0, 0.5, 1.0, -1.0, 2.0, 0.5, 3.0, 1.0, -2.0, 0.3])
    res = {f: np.full(1, np.nan) for f in ('p_rep',)}
    post = np.full(1, np.nan)
    prior = _no_prior(3)

    def rc(G, nc, off, opts=None, out=None, npos=1, prior=prior, post=post):
        off = np.asarray(off, np.int64)
        opts = L.make_rep_opts() if opts is None else opts
        out = L.make_out(L.NmodRepOut, **engine._np_ptrs(res)) if out is None else out
        return lib.nmod_site_diff_rep_mod(C.byref(prm), npos, G, nc, ptr(score), ptr(off), C.byref(opts), C.byref(out),
                                          ptr(prior) if prior is not None else None, ptr(post) if post is not None else None)
    off3 = [0, 4, 8, 12]
    assert rc(3, 1, off3) == OK and not np.isnan(res['p_rep'][0]) and not np.isnan(post[0])
    assert rc(3, 1, off3, post=None) == OK                                             # phi_post is optional
    assert rc(3, 1, off3, prior=None) == INVALID
    assert rc(2, 1, [0, 6, 12]) == INVALID and rc(17, 8, list(range(18))) == INVALID
    assert rc(3, 0, off3) == INVALID and rc(3, 3, off3) == INVALID and rc(3, 1, [0, 8, 4, 12]) == INVALID
    short = L.make_rep_opts(); short.struct_size -= 8
    assert rc(3, 1, off3, opts=short) == INVALID
    wrong = L.make_out(L.NmodRepOut, **engine._np_ptrs(res)); wrong.struct_size += 8
    assert rc(3, 1, off3, out=wrong) == INVALID
    for bad in (dict(phi_floor=-1.0), dict(phi_floor=np.nan), dict(ci_drop=0.0), dict(max_iter=0), dict(min_valid=0), dict(tol=-1.0)):
        assert rc(3, 1, off3, opts=L.make_rep_opts(**bad)) == INVALID, bad
    assert rc(3, 1, [0], npos=0) == OK
    # the Python layers
    for kw in (dict(df=0), dict(df=15), dict(df=2.5), dict(ci_level=0.0), dict(ci_level=1.0)):
        with pytest.raises(ValueError):
            rep_prior_host(phi, status, **dict(dict(df=2), **kw))
    with pytest.raises(ValueError):
        site_diff_rep_host(score, np.array(off3, np.int64), 3, 1, prior=np.zeros(7))


# ------------------------------------------------------------------------------------------------------------- the stream contract
def _chain_inputs():
    """length_batches()[(4, 2)] three times over in a seeded order; the decoy: the same sites in reverse order"""
    sites = R.length_batches()[(4, 2)]
    idx = np.random.default_rng(2540).permutation(np.tile(np.arange(len(sites)), 3))

    def one(ix):
        score, off = R.csr([sites[i] for i in ix])
        return dict(score=score, off=off)
    return one(idx), one(idx[::-1])


def test_the_three_call_chain_obeys_the_stream_contract():
    """tests/stream_cases.py's stall-and-decoy method, as the K24 test applies it: K24 without its interval, the prior and the moderated
    entry are enqueued behind a stall on a side stream, the record staying on the device; the calls return while the stream is still
    stalled — no host read in between — and the results have the bytes of the host path"""
    import torch
    import stream_cases as SC
    real, decoy = _chain_inputs()
    kw = dict(min_valid=R.LENGTH_MIN_VALID)
    first = site_diff_rep_host(real['score'], real['off'], 4, 2, interval=False, **kw)
    rec = rep_prior_host(first['phi'], first['status'], 2)
    host = site_diff_rep_host(real['score'], real['off'], 4, 2, prior=rec, **kw)
    assert rec['n_used'] >= 12 and rec['d0'] > 0.0                 # (a prior is in force: the chain is not K24 twice)
    det = engine.DeviceDetector(0)

    def call(t, out=None, record=None, first=None):
        a = det.site_diff_rep(t['score'], t['off'], 4, 2, interval=False, out=first, **kw)
        prior = det.rep_prior(a['phi'], a['status'], 2, out=record)
        return dict(det.site_diff_rep(t['score'], t['off'], 4, 2, prior=prior, out=out, **kw), rep_prior=prior)
    numpy = lambda res: {k: v.cpu().numpy() for k, v in res.items()}
    sw = SC.Swapped(real, decoy)
    sw.load_real()
    shape = call(sw.t)
    torch.cuda.synchronize()
    want = numpy(shape)
    assert _bits(want.pop('rep_prior')) == _rec_bits(rec)
    assert set(want) == set(host) and all(_bits(want[f]) == _bits(host[f]) for f in host)
    sw.load_decoy()
    torch.cuda.synchronize()
    other = numpy(call(sw.t))
    assert any(_bits(other[f]) != _bits(want[f]) for f in want), 'the decoy gives the same results: the test could not see a misplaced read'
    out = {k: torch.empty_like(v) for k, v in shape.items() if k != 'rep_prior'}
    record = torch.empty(L.REP_PRIOR_WORDS, dtype=torch.float64, device='cuda:0')
    first_out = {k: torch.empty_like(v) for k, v in out.items() if k not in ('phi_post', 'delta_lo', 'delta_hi')}     # all allocated before the stall
    for _ in range(2):
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            warm = [torch.empty(1 << 20, dtype=torch.uint8, device='cuda:0'), torch.empty(8 << 20, dtype=torch.uint8, device='cuda:0')]
        del warm
        stream.synchronize()
        with torch.cuda.stream(stream):
            SC.stall(stream, SC.T_MS)
            event = torch.cuda.Event()
            event.record(stream)
            sw.load_real()
            res = call(sw.t, SC.fill_sentinel(out), SC.fill_sentinel(dict(r=record))['r'], SC.fill_sentinel(first_out))
            sw.load_decoy()
            early = event.query()
        assert not early, 'the stall of %g ms had ended when the calls returned' % SC.T_MS
        stream.synchronize()
        got = numpy(res)
        assert _bits(got.pop('rep_prior')) == _rec_bits(rec)
        assert all(_bits(got[f]) == _bits(want[f]) for f in want), [f for f in want if _bits(got[f]) != _bits(want[f])]
        assert sw.holds('decoy'), 'the inputs were written after the trailing copy, or the copy did not run'


# ----------------------------------------------------------------------------------------------------------------------- the chain
def test_chain_and_command_line_find_the_planted_site(capsys, tmp_path):
    from nanomod_amd import cli, container, kmermodel
    from nanomod_amd import readllr as RL
    import test_site_diff_rep_gpu as K24
    c, m, model, alt, planted = K24._four_samples()
    lines = []
    plain = RL.compare_reads_llr_rep(c, m, model, alt, min_coverage=5, fdr='bh', log=lambda s: None)
    sites = RL.compare_reads_llr_rep(c, m, model, alt, min_coverage=5, fdr='bh', log=lines.append, moderate=True)
    assert len(lines) == 2 and lines[0].startswith('readdiff: 2 and 2 sample(s)') and lines[1].startswith('readdiff: the prior of the dispersions')
    rec = sites['rep_prior']
    assert list(rec) == list(L.REP_PRIOR_FIELDS) and sites['df_tot'] == rec['df_tot'] == 2.0 + rec['d0'] and rec['d0'] > 0.0
    for f in ('pi_s', 'n_valid', 'pi0', 'pi1', 'delta', 'stat_cond', 'p_cond', 'phi', 'pos'):
        assert _bits(sites[f]) == _bits(plain[f]), f
    est = (sites['rep_status'] & L.REP_NO_ESTIMATE) == 0
    assert est.sum() > 200 and rec['n_used'] + rec['n_zero'] <= est.sum() and rec['n_used'] > 100
    # the engine's own numbers for the same rows: the prior over the chain's phi, the posterior dispersion
    want = rep_prior_host(plain['phi'], plain['rep_status'], 2)
    assert _rec_bits(want) == _rec_bits(rec)
    prior = engine.rep_prior_record(rec)
    post = np.array([M.phi_post_of(p, prior, 2) for p in plain['phi'][est]])
    assert np.allclose(sites['phi_post'][est], post, rtol=1e-14, atol=0.0)
    for strand in '+-':
        sel = np.flatnonzero((sites['strand'] == strand) & est)
        at = sel[sites['pos'][sel] == planted]
        assert len(at) == 1
        i = at[0]
        assert 0.2 < sites['delta'][i] < 0.8 and sites['p_rep'][i] < 0.01 and sites['p_rep'][i] < np.median(sites['p_rep'][sel])
        assert sites['delta_lo'][i] > 0.0                       # (p_rep < 0.05 and the interval at the 0.95 quantile of the same law)
        print('planted site on %s: K24 p_rep %.3g, moderated %.3g (q %.3g) on %g degrees of freedom'
              % (strand, plain['p_rep'][i], sites['p_rep'][i], sites['q'][i], sites['df_tot']))
    # q is the device's Benjamini-Hochberg track of the moderated p_rep
    (want_q,), _ = engine.fdr_adjust_host([sites['p_rep']])
    assert _bits(sites['q']) == _bits(want_q) and _bits(sites['p_rep']) != _bits(plain['p_rep'])
    # the same chain through the command line
    paths = {}
    for n, r in (('c0', c[0]), ('c1', c[1]), ('m0', m[0]), ('m1', m[1])):
        paths[n] = str(tmp_path / (n + '.npz'))
        container.save_reads(paths[n], *[r[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
    zeros = np.zeros(64, np.int64)
    for n, t in (('model', model), ('alt', alt)):
        paths[n] = str(tmp_path / (n + '.npz'))
        kmermodel.save_kmer_model(paths[n], dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=t['mean'], sd=t['sd'],
                                                 n_positions=t['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
    base = ['readdiff', '--wrkBase1', paths['c0'] + ',' + paths['c1'], '--wrkBase2', paths['m0'] + ',' + paths['m1'], '--kmerModel', paths['model'],
            '--altModel', paths['alt'], '--FileID', 'run', '--minCoverage', '5', '--fdr', 'bh']
    out = str(tmp_path / 'out')
    capsys.readouterr()
    assert cli.main(base + ['--outFolder', out, '--moderate', '1']) == 0
    printed = capsys.readouterr().out
    assert 'run_site_diff_mod.txt' in printed and 'run_rep_prior.txt' in printed and 'the prior of the dispersions' in printed
    assert sorted(os.listdir(out)) == ['run_rep_prior.txt', 'run_site_diff_mod.txt']
    u = [ln.split() for ln in open(os.path.join(out, 'run_site_diff_mod.txt')).read().splitlines()]
    assert len(u) == len(sites['pos']) and all(len(r) == 5 + 8 + 12 + 2 + 2 for r in u)
    assert [int(r[2]) for r in u] == (sites['pos'] + 1).tolist() and [int(r[-1]) for r in u] == sites['rep_status'].tolist()
    assert [r[-5] for r in u] == ['%.3E' % v if v == v else 'nan' for v in sites['p_rep']]
    assert [r[-4] for r in u] == ['%.3f' % v if v == v else 'nan' for v in sites['phi_post']]
    assert all(r[-3] == '%g' % rec['df_tot'] for r in u)
    assert [r[-2] for r in u] == ['%.3E' % v if v == v else 'nan' for v in sites['q']]
    pr = [ln.split() for ln in open(os.path.join(out, 'run_rep_prior.txt')).read().splitlines()]
    assert [r[0] for r in pr] == list(L.REP_PRIOR_FIELDS) and [float(r[1]) for r in pr] == [rec[f] for f in L.REP_PRIOR_FIELDS]
    # without --moderate: K24's file, the bytes its own writer gives for K24's sites, and nothing else
    out2 = str(tmp_path / 'out2')
    assert cli.main(base + ['--outFolder', out2]) == 0
    assert 'prior' not in capsys.readouterr().out and os.listdir(out2) == ['run_site_diff_rep.txt']
    RL.write_site_diff_rep(str(tmp_path / 'k24.txt'), plain)
    assert open(os.path.join(out2, 'run_site_diff_rep.txt'), 'rb').read() == open(str(tmp_path / 'k24.txt'), 'rb').read()
    assert cli.main(base[:2] + [paths['c0'], '--wrkBase2', paths['m0']] + base[5:] + ['--outFolder', out2, '--moderate', '1']) == 1
    assert '--moderate' in capsys.readouterr().out
