"""nmod_site_diff_rep (K24) on the GPU against the numpy restatement of its definition (tests/diff_rep_ref.py, pinned against mpmath in
tests/test_site_diff_rep.py) and against the code it is built on: the condition level byte for byte against nmod_site_diff on the
concatenated rows, the saturated fit against nmod_site_stoich per sample; parity over G, ncontrol, the super-row lengths at which
the code takes another path and the sample lengths that break its lane alignment, over the content of the rows, the symmetries of
the definition, the independence of a site's bits from everything but the site, a batch larger than the persistent grids, the
iteration limits, the refusals of the C entry and the stream contract of the device entry.  The gates are diff_rep_ref's."""
import ctypes as C

import numpy as np
import pytest

import diff_rep_ref as R
import stoich_ref as SR
from nanomod_amd import _lib as L
from nanomod_amd import engine
from nanomod_amd.engine import site_diff_host, site_stoich_host
from nanomod_amd.engine import site_diff_rep_host          # K24's entry: without it nothing here can pass

pytestmark = pytest.mark.gpu

SITE_FIELDS = R.FIELDS + ('iters', 'status')
SAMPLE_FIELDS = ('pi_s', 'n_valid')
_worst = {}                                             # the worst ratio of a deviation to its gate over the session, printed per test


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _share(name, dev, gate, worst):
    if gate == 0.0:
        assert dev == 0.0, '%s differs where its gate is 0: %r' % (name, dev)
        return
    worst[name] = max(worst.get(name, 0.0), dev / gate)


def _report(worst):
    for k, v in worst.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    fmt = lambda w: ', '.join('%s %.3g' % kv for kv in sorted(w.items())) or 'none compared'
    print('worst deviation as a share of its gate: %s (over the session: %s)' % (fmt(worst), fmt(_worst)))
    assert all(v <= 1.0 for v in worst.values()), worst


def _check_sites(got, exp, G, converged=True, interval=True, worst=None):
    """status, the counts and the NaN pattern exactly; both ends of [0, 1] and of [-1, 1] exactly; everything else within the gates.
    Returns the number of sites with an estimate"""
    own = worst is None
    worst = {} if own else worst
    fields = [f for f in R.FIELDS if interval or f not in ('delta_lo', 'delta_hi')]
    pi_s, n_valid = got['pi_s'].reshape(-1, G), got['n_valid'].reshape(-1, G)
    est = 0
    for i, e in enumerate(exp):
        assert int(got['status'][i]) == e['status'] and n_valid[i].tolist() == e['n_valid'].tolist(), (i, got['status'][i], e['status'], n_valid[i], e['n_valid'])
        if e['gates'] is None:
            assert all(np.isnan(got[f][i]) for f in fields) and np.isnan(pi_s[i]).all() and got['iters'][i] == 0, i
            continue
        est += 1
        assert not any(np.isnan(got[f][i]) for f in fields) and not np.isnan(pi_s[i]).any(), i
        for f in ('pi0', 'pi1', 'pi_pool'):
            assert 0.0 <= got[f][i] <= 1.0 and (got[f][i] in (0.0, 1.0)) == (e[f] in (0.0, 1.0)), (i, f, got[f][i], e[f])
        assert ((pi_s[i] == 0.0) == (e['pi_s'] == 0.0)).all() and ((pi_s[i] == 1.0) == (e['pi_s'] == 1.0)).all(), (i, pi_s[i], e['pi_s'])
        g = e['gates']
        held = interval and g['delta_lo'] is not None
        if held:
            assert -1.0 <= got['delta_lo'][i] <= got['delta'][i] <= got['delta_hi'][i] <= 1.0, i
            assert (got['delta_lo'][i] == -1.0) == (e['delta_lo'] == -1.0) and (got['delta_hi'][i] == 1.0) == (e['delta_hi'] == 1.0), i
        if not converged:
            continue
        assert got['iters'][i] == e['iters'], (i, got['iters'][i], e['iters'])
        for k in range(G):
            _share('pi_s', abs(pi_s[i, k] - e['pi_s'][k]), g['pi_s'][k], worst)
        for f in fields:
            if f in ('p_cond', 'p_het', 'p_rep'):
                lo, hi = g[f]
                assert lo <= got[f][i] <= hi, (i, f, lo, got[f][i], hi)
            elif f in ('delta_lo', 'delta_hi'):
                if held:
                    _share(f, abs(got[f][i] - e[f]), g[f], worst)
            else:
                _share(f, abs(got[f][i] - e[f]), g[f], worst)
    if own:
        _report(worst)
    return est


def _exp(which, key=None, **kw):
    """diff_rep_ref.expected at the drop the Python layers pass for ci_level 0.95: engine._f1_quantile (pinned against scipy and mpmath
    in tests/test_site_diff_rep.py), so that both sides start from the same ci_drop to the bit"""
    return R.expected(which, key, ci_drop=engine._f1_quantile(0.95, (key[0] if key else 4) - 2), **kw)


def _cat_rows(sites, nc):
    """the two super-rows of every site as the CSR pairs nmod_site_diff takes"""
    s0, o0 = SR._csr([np.concatenate(rows[:nc]) for rows in sites])
    s1, o1 = SR._csr([np.concatenate(rows[nc:]) for rows in sites])
    return s0, o0, s1, o1


def _against_site_diff(got, sites, nc, exp, **kw):
    """the condition level byte for byte against nmod_site_diff on the concatenated rows, wherever both estimate"""
    k15 = site_diff_host(*_cat_rows(sites, nc), interval=False, **kw)
    both = np.array([e['gates'] is not None for e in exp]) & ((k15['status'] & L.DIFF_NO_ESTIMATE) == 0)
    for f, h in (('pi0', 'pi0'), ('pi1', 'pi1'), ('pi_pool', 'pi_pool'), ('delta', 'delta'), ('stat_cond', 'stat'), ('p_cond', 'p_diff'), ('iters', 'iters')):
        assert _bits(got[f][both]) == _bits(k15[h][both]), f
    return int(both.sum())


def _against_site_stoich(got, sites, G, exp, **kw):
    """pi_s and n_valid against nmod_site_stoich per sample: the counts exactly, the estimates within the two gates summed"""
    score, off = R.csr(sites)
    k14 = site_stoich_host(score, off, **kw)
    ref = SR.site_stoich(score, off, **dict(SR.DEFAULTS, **kw))
    assert np.array_equal(got['n_valid'], k14['n_valid'])
    seen = 0
    for i, e in enumerate(exp):
        if e['gates'] is None:
            continue
        for g in range(G):
            r = ref[i * G + g]
            assert r['gates'] is not None, (i, g)
            assert abs(got['pi_s'][i * G + g] - k14['pi'][i * G + g]) <= e['gates']['pi_s'][g] + r['gates']['pi'], (i, g)
            seen += 1
    return seen


@pytest.mark.parametrize('key', R.CONFIGS, ids=lambda k: 'G%d_nc%d' % k)
def test_parity_over_the_lengths(key):
    G, nc = key
    sites = R.length_batches()[key]
    score, off = R.csr(sites)
    exp = _exp('length', key)
    mv = R.LENGTH_MIN_VALID
    drop = R.f1_quantile(0.95, G - 2)
    got = site_diff_rep_host(score, off, G, nc, min_valid=mv)
    est = _check_sites(got, exp, G)
    assert 4 * est >= 3 * len(exp), (est, len(exp))
    assert _against_site_diff(got, sites, nc, exp, min_valid=mv) == est
    assert _against_site_stoich(got, sites, G, exp, min_valid=mv) == est * G
    # the interval against nmod_site_diff itself at the drop phi_used * ci_drop, a site at a time
    lib, opts_of = L.load(), engine._rep_opts(G, nc, mv, 0.95, 0.0, 60, 1e-12)[0]
    assert abs(opts_of.ci_drop - drop) <= 1e-9 * drop
    done = 0
    for i, e in enumerate(exp):
        if e['gates'] is None or not e['phi_used'] > 0.0:
            continue
        s0, o0, s1, o1 = _cat_rows([sites[i]], nc)
        phi_used = max(got['phi'][i], 0.0)
        res = {f: np.full(1, np.nan) for f in ('delta_lo', 'delta_hi')}
        out = L.make_out(L.NmodDiffOut, **engine._np_ptrs(res))
        o = L.make_diff_opts(60, mv, 1e-12, phi_used * opts_of.ci_drop)
        prm = L.make_params(device=0, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
        L.check(lib.nmod_site_diff(C.byref(prm), 1, engine._np_ptr(s0), engine._np_ptr(o0), engine._np_ptr(s1), engine._np_ptr(o1), C.byref(o), C.byref(out)))
        assert _bits(res['delta_lo']) == _bits(got['delta_lo'][i:i + 1]) and _bits(res['delta_hi']) == _bits(got['delta_hi'][i:i + 1]), i
        done += 1
    assert done >= 2


def test_the_length_batches_hold_every_step():
    """the super-row lengths at K15's steps, the stage limit and the sample lengths of the issue all occur (no device work)"""
    longer, staged, samples = set(), set(), set()
    for (G, nc), sites in R.length_batches().items():
        for rows in sites:
            a, b = sum(len(r) for r in rows[:nc]), sum(len(r) for r in rows[nc:])
            longer.add(max(a, b)); staged.add(a + b); samples.update(len(r) for r in rows)
    assert {127, 128, 129, 511, 512, 513} <= longer and {R.STAGE, R.STAGE + 1} <= staged
    assert {0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65} <= samples
    assert {G for G, _ in R.CONFIGS} == {3, 4, 7, 16} and all({1, G - 1} <= {nc for g, nc in R.CONFIGS if g == G} for G in (3, 4, 7, 16))


@pytest.mark.parametrize('phi_floor', [0.0, 1.0])
def test_content(phi_floor):
    sites = R.content_sites()
    score, off = R.csr(sites)
    exp = _exp('content', phi_floor=phi_floor)
    got = site_diff_rep_host(score, off, 4, 2, phi_floor=phi_floor)
    est = _check_sites(got, exp, 4)
    assert 4 * est >= 3 * len(exp)
    st = np.array([e['status'] for e in exp])
    assert (st & R.TOO_FEW).any() and (st & R.FLAT).any() and (st == 0).any() and (st & R.POOL_AT_END).any()
    assert _against_site_diff(got, sites, 2, exp) == est
    assert _against_site_stoich(got, sites, 4, exp) == est * 4
    # the constructed site: every g is exactly 0
    i = next(i for i, rows in enumerate(sites) if all((np.abs(r) == 40.0).all() for r in rows))
    assert got['phi'][i] == 0.0 and got['stat_het'][i] == 0.0 and got['stat_cond'][i] > 0.0 and got['pi_s'].reshape(-1, 4)[i].tolist() == [0.0, 0.0, 1.0, 1.0]
    if phi_floor == 0.0:
        assert got['status'][i] & R.PHI_ZERO and got['p_rep'][i] == R.DBL_MIN and ((st & R.PHI_ZERO) != 0).sum() == 1
    else:                                                       # the plain F on (1, 2)
        lo, hi = exp[i]['gates']['p_rep']
        assert not got['status'][i] & R.PHI_ZERO and lo <= got['p_rep'][i] <= hi and exp[i]['p_rep'] == R.t_two_sided(exp[i]['stat_cond'], 2)
        assert not (st & R.PHI_ZERO).any()


def test_one_evaluation_and_no_tolerance():
    sites = R.content_sites()
    score, off = R.csr(sites)
    for kw in (dict(max_iter=1), dict(tol=0.0, max_iter=30)):
        exp = _exp('content', **kw)
        got = site_diff_rep_host(score, off, 4, 2, **kw)
        assert _check_sites(got, exp, 4, converged=False) >= 20
        interior = [i for i, e in enumerate(exp) if e['gates'] is not None and 0.0 < e['pi_pool'] < 1.0]
        assert interior and all(got['iters'][i] == kw['max_iter'] for i in interior)
        # (the constructed site is symmetric: S is exactly 0 at the first point, 0.5, the step is 0 and the stop test holds at once)
        still = [i for i in interior if exp[i]['status'] & R.NOT_CONVERGED]
        assert len(still) >= len(interior) - 1 and all(got['status'][i] & R.NOT_CONVERGED for i in still)
        assert all(not np.isnan(got[f][i]) for f in R.FIELDS for i in interior)


def _gates_of(exp, f):
    return np.array([e['gates'][f] if e['gates'] is not None and e['gates'][f] is not None else 0.0 for e in exp])


def test_permuting_the_samples_inside_a_condition():
    """G = 7, ncontrol = 3: pi_s and n_valid move with their samples bit for bit — a sample's sums run in the sample's own order,
    whatever its offset in the super-row — and the rest moves within its gates"""
    key, perm = (7, 3), [2, 0, 1, 6, 3, 5, 4]
    sites = R.length_batches()[key]
    exp = _exp('length', key)
    a = site_diff_rep_host(*R.csr(sites), 7, 3, min_valid=R.LENGTH_MIN_VALID)
    b = site_diff_rep_host(*R.csr([[rows[p] for p in perm] for rows in sites]), 7, 3, min_valid=R.LENGTH_MIN_VALID)
    est = np.array([e['gates'] is not None for e in exp])
    assert est.sum() >= 4 and np.array_equal(a['status'], b['status'])
    pa, pb = a['pi_s'].reshape(-1, 7)[:, perm], b['pi_s'].reshape(-1, 7)
    differ = (pa != pb) & ~(np.isnan(pa) & np.isnan(pb))
    print('pi_s after the permutation: %d of %d estimates differ in their bits' % (differ.sum(), est.sum() * 7))
    for f in SAMPLE_FIELDS:
        assert _bits(a[f].reshape(-1, 7)[:, perm]) == _bits(b[f].reshape(-1, 7)), f
    worst = {}
    for f in ('pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat_cond', 'stat_het', 'phi'):
        gate = 2.0 * _gates_of(exp, f)
        for i in np.flatnonzero(est):
            _share(f, abs(a[f][i] - b[f][i]), gate[i], worst)
    for f in ('p_cond', 'p_het', 'p_rep'):
        for i in np.flatnonzero(est):
            lo, hi = exp[i]['gates'][f]
            assert lo <= b[f][i] <= hi, (f, i)
    _report(worst)
    # the offset alone: the same samples behind a longer first sample of their condition, in the 16-lane, wave and workgroup forms
    rng = np.random.default_rng(2408)
    for first in (5, 130, 600):
        rows = [SR.simulate_row(rng, n, 3.0, 0.4) for n in (17, 64, 9, 33, 65)]
        lead = [SR.simulate_row(rng, n, 3.0, 0.4) for n in (3, first)]
        x = site_diff_rep_host(*R.csr([[lead[0], rows[0], rows[1], rows[2], rows[3], rows[4]]]), 6, 3)
        y = site_diff_rep_host(*R.csr([[lead[1], rows[1], rows[0], rows[2], rows[4], rows[3]]]), 6, 3)
        assert x['status'][0] == y['status'][0] == 0
        assert _bits(x['pi_s'][[1, 2, 3, 4, 5]]) == _bits(y['pi_s'][[2, 1, 3, 5, 4]]), first


def test_swapping_the_conditions():
    """G = 4, ncontrol = 2 and G = 7, 3 against 4: delta flips, its interval ends swap, pi_s moves with its samples bit for bit"""
    for (G, nc), sites, kw in (((4, 2), R.content_sites(), {}), ((7, 3), R.length_batches()[(7, 3)], dict(min_valid=R.LENGTH_MIN_VALID))):
        exp = _exp('content') if G == 4 else _exp('length', (G, nc))
        a = site_diff_rep_host(*R.csr(sites), G, nc, **kw)
        order = list(range(nc, G)) + list(range(nc))
        b = site_diff_rep_host(*R.csr([[rows[p] for p in order] for rows in sites]), G, G - nc, **kw)
        est = np.array([e['gates'] is not None for e in exp])
        assert np.array_equal(a['status'], b['status'])
        for f in SAMPLE_FIELDS:
            assert _bits(a[f].reshape(-1, G)[:, order]) == _bits(b[f].reshape(-1, G)), f
        assert _bits(a['pi0']) == _bits(b['pi1']) and _bits(a['pi1']) == _bits(b['pi0']) and _bits(a['pi_pool']) == _bits(b['pi_pool'])
        assert np.array_equal(a['delta'][est], -b['delta'][est])
        for f, g in (('delta_lo', 'delta_hi'), ('delta_hi', 'delta_lo')):
            assert (np.abs(a[f][est] + b[g][est]) <= (_gates_of(exp, f) * 2.0 + _gates_of(exp, g) * 2.0)[est]).all(), f
        for f in ('stat_cond', 'stat_het', 'phi'):
            assert (np.abs(a[f][est] - b[f][est]) <= (_gates_of(exp, f) * 2.0)[est]).all(), f


def test_a_sites_bits_depend_on_the_site_alone():
    import torch
    G, nc = 4, 2
    sites = R.length_batches()[(G, nc)]
    score, off = R.csr(sites)
    kw = dict(min_valid=R.LENGTH_MIN_VALID)
    full = site_diff_rep_host(score, off, G, nc, **kw)
    n = len(sites)

    def same(res, idx, what):
        for f in SITE_FIELDS:
            if f in res:
                assert _bits(res[f]) == _bits(full[f][idx]), (what, f)
        for f in SAMPLE_FIELDS:
            if f in res:
                assert _bits(res[f].reshape(-1, G)) == _bits(full[f].reshape(-1, G)[idx]), (what, f)
    # reversed, and every site alone (one of each form, both sides of the stage limit among them)
    rev = list(range(n))[::-1]
    same(site_diff_rep_host(*R.csr([sites[i] for i in rev]), G, nc, **kw), rev, 'reversed')
    for i in range(n):
        same(site_diff_rep_host(*R.csr([sites[i]]), G, nc, **kw), [i], 'alone %d' % i)
    # device memory
    det = engine.DeviceDetector(device=0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dev = det.site_diff_rep(t(score), t(off), G, nc, **kw)
    same({f: v.cpu().numpy() for f, v in dev.items()}, list(range(n)), 'device')
    # without the interval, and a subset of the outputs through the C entry
    no = site_diff_rep_host(score, off, G, nc, interval=False, **kw)
    assert 'delta_lo' not in no and 'delta_hi' not in no
    same(no, list(range(n)), 'no interval')
    few = {f: torch.empty(n, dtype=torch.float64, device='cuda') for f in ('p_rep', 'delta_hi', 'phi')}
    few['pi_s'] = torch.empty(n * G, dtype=torch.float64, device='cuda')
    opts = engine._rep_opts(G, nc, R.LENGTH_MIN_VALID, 0.95, 0.0, 60, 1e-12)[0]
    out = L.make_out(L.NmodRepOut, **{f: v.data_ptr() for f, v in few.items()})
    prm = det._params(L.DTYPE_F64, 0, 0, 0, 0)
    d_score, d_off = t(score), t(off)
    L.check(L.load().nmod_site_diff_rep(C.byref(prm), n, G, nc, d_score.data_ptr(), d_off.data_ptr(), C.byref(opts), C.byref(out)))
    torch.cuda.synchronize()
    same({f: v.cpu().numpy() for f, v in few.items()}, list(range(n)), 'subset')


def test_a_batch_larger_than_the_persistent_grids():
    """about 40 000 sites of 3 x 4 reads, more than the 16-lane form walks at once (8 workgroups per CU of 16 sites each): every site
    equal to the same site computed alone"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nsites, kinds, G, nc = max(40000, cus * 8 * 16 + 37), 5, 3, 1
    rng = np.random.default_rng(2406)
    kind = [[SR.simulate_row(rng, 4, 3.0, p) for p in (0.3 + 0.1 * k, 0.5, 0.8 - 0.1 * k)] for k in range(kinds)]
    alone = [site_diff_rep_host(*R.csr([rows]), G, nc) for rows in kind]
    assert sum(a['status'][0] & R.NO_ESTIMATE == 0 for a in alone) >= 4
    which = rng.integers(0, kinds, nsites)
    flat = np.stack([np.concatenate(rows) for rows in kind])[which].reshape(-1)
    got = site_diff_rep_host(flat, np.arange(0, 4 * G * nsites + 1, 4, dtype=np.int64), G, nc)
    for f in SITE_FIELDS + SAMPLE_FIELDS:
        w = G if f in SAMPLE_FIELDS else 1
        ref = np.stack([a[f] for a in alone])[which].reshape(-1)
        assert ref.shape == (nsites * w,) and _bits(got[f]) == _bits(ref), f


def test_refusals_of_the_c_entry():
    lib = L.load()
    OK, INVALID = 0, -1                                         # NMOD_OK, NMOD_ERR_INVALID_ARG (include/nanomod_hip.h)
    score = np.array([1.0, -1.0, 2.0, 0.5, 1.0, -1.0, 2.0, 0.5, 3.0, 1.0, -2.0, 0.3])
    res = {f: np.full(1, np.nan) for f in ('p_rep',)}
    prm = L.make_params(device=0, memspace=L.MEM_HOST, dtype=L.DTYPE_F64)

    def rc(G, nc, off, opts=None, out=None, npos=1):
        off = np.asarray(off, np.int64)
        opts = L.make_rep_opts() if opts is None else opts
        out = L.make_out(L.NmodRepOut, **engine._np_ptrs(res)) if out is None else out
        return lib.nmod_site_diff_rep(C.byref(prm), npos, G, nc, engine._np_ptr(score), engine._np_ptr(off), C.byref(opts), C.byref(out))
    off3 = [0, 4, 8, 12]
    assert rc(3, 1, off3) == OK and not np.isnan(res['p_rep'][0])
    assert rc(2, 1, [0, 6, 12]) == INVALID                           # two samples: nmod_site_diff
    assert rc(17, 8, list(range(18))) == INVALID
    assert rc(3, 0, off3) == INVALID and rc(3, 3, off3) == INVALID
    assert rc(3, 1, [0, 8, 4, 12]) == INVALID                        # a decreasing host off
    short = L.make_rep_opts(); short.struct_size -= 8
    assert rc(3, 1, off3, opts=short) == INVALID
    wrong = L.make_out(L.NmodRepOut, **engine._np_ptrs(res)); wrong.struct_size += 8
    assert rc(3, 1, off3, out=wrong) == INVALID
    for bad in (dict(phi_floor=-1.0), dict(phi_floor=np.inf), dict(phi_floor=np.nan), dict(ci_drop=0.0), dict(max_iter=0), dict(min_valid=0), dict(tol=-1.0)):
        assert rc(3, 1, off3, opts=L.make_rep_opts(**bad)) == INVALID, bad
    assert lib.nmod_site_diff_rep(C.byref(prm), 1, 3, 1, engine._np_ptr(score), None, C.byref(L.make_rep_opts()),
                                  C.byref(L.make_out(L.NmodRepOut, **engine._np_ptrs(res)))) == INVALID      # CSR only
    assert rc(3, 1, [0], npos=0) == OK


def test_p_rep_goes_straight_into_the_device_fdr():
    import torch
    score, off = R.csr(R.content_sites())
    det = engine.DeviceDetector(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    res = det.site_diff_rep(t(score), t(off), 4, 2)
    (q,), summary = det.fdr(res, tracks=('p_rep',), method='bh', alpha=0.05)
    torch.cuda.synchronize()
    p, q = res['p_rep'].cpu().numpy(), q.cpu().numpy()
    (want,), (summ,) = engine.fdr_adjust_host([p])
    assert _bits(q) == _bits(want) and engine.fdr_summary_dicts(summary)[0] == summ
    assert summ['tested'] == int((~np.isnan(p)).sum()) and summ['excluded'] == int(np.isnan(p).sum()) and summ['rejected'] >= 1


def test_match_score_rows_multi_gathers_site_major():
    import torch
    t = lambda x, d: torch.tensor(x, dtype=d, device='cuda')
    piv = lambda key, off, sig, base: dict(key=t(key, torch.int64), off=t(off, torch.int64), sig=t(sig, torch.float64), base=t(base, torch.uint8), names=['chrT'])
    g = [piv([5, 6, 9], [0, 2, 3, 6], [1.5, -2.25, 0.125, 3.0, -1.0, 2.0], [65, 67, 71]),
         piv([5, 9, 11], [0, 3, 5, 6], [0.001, 1e-7, -4.5, 7.0, 1e300, 2.0], [65, 71, 84]),
         piv([4, 5, 9], [0, 1, 3, 5], [9.0, 0.5, -0.5, 8.0, -8.0], [84, 65, 71])]
    m = engine.match_score_rows_multi(g, 1, 2)
    assert m['sig'].dtype == torch.float64 and (m['n_samples'], m['n_control']) == (3, 1)
    assert m['key'].tolist() == [5, 9] and m['base'].tolist() == [65, 71] and m['off'].tolist() == [0, 2, 5, 7, 10, 12, 14]
    assert _bits(m['sig'].cpu().numpy()) == _bits(np.array([1.5, -2.25, 0.001, 1e-7, -4.5, 0.5, -0.5, 3.0, -1.0, 2.0, 7.0, 1e300, 8.0, -8.0]))
    assert engine.match_score_rows_multi(g, 2, 3)['key'].tolist() == [] and engine.match_score_rows_multi(g, 2, 3)['off'].tolist() == [0]


# ------------------------------------------------------------------------------------------------------------- the stream contract
def _rep_inputs():
    """length_batches()[(4, 2)] three times over in a seeded order (every class of K15, both sides of the stage limit); the decoy: the
    same sites in reverse order"""
    sites = R.length_batches()[(4, 2)]
    idx = np.random.default_rng(2407).permutation(np.tile(np.arange(len(sites)), 3))

    def one(ix):
        score, off = R.csr([sites[i] for i in ix])
        return dict(score=score, off=off)
    return one(idx), one(idx[::-1])


def test_the_device_entry_obeys_the_stream_contract():
    """tests/stream_cases.py's stall-and-decoy method, as tests/test_stream_contract_gpu.py applies it to the other entries: the call
    returns while the stream is still stalled, and its results are those of the inputs in place at its position in the stream"""
    import torch
    import stream_cases as SC
    real, decoy = _rep_inputs()
    assert {k: v.shape for k, v in real.items()} == {k: v.shape for k, v in decoy.items()} and not np.array_equal(real['off'], decoy['off'])
    kw = dict(min_valid=R.LENGTH_MIN_VALID)
    host = site_diff_rep_host(real['score'], real['off'], 4, 2, **kw)
    det = engine.DeviceDetector(0)
    call = lambda t, out=None: det.site_diff_rep(t['score'], t['off'], 4, 2, out=out, **kw)
    numpy = lambda res: {k: v.cpu().numpy() for k, v in res.items()}
    # serially first: the shapes of the outputs, every kernel loaded, the results the stalled calls must give
    sw = SC.Swapped(real, decoy)
    sw.load_real()
    first = call(sw.t)
    torch.cuda.synchronize()
    want = numpy(call(sw.t, SC.fill_sentinel({k: torch.empty_like(v) for k, v in first.items()})))
    sw.load_decoy()
    torch.cuda.synchronize()
    assert set(want) == set(host) and all(_bits(want[f]) == _bits(host[f]) for f in host)
    other = numpy(call(sw.t))
    assert any(_bits(other[f]) != _bits(want[f]) for f in want), 'the decoy gives the same results: the test could not see a misplaced read'
    out = {k: torch.empty_like(v) for k, v in first.items()}     # allocated before the stall, filled behind it
    for _ in range(2):                                          # two streams made one after the other: stream_cases' docstring
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
            res = call(sw.t, SC.fill_sentinel(out))
            sw.load_decoy()
            early = event.query()
        assert not early, 'the stall of %g ms had ended when the call returned' % SC.T_MS
        stream.synchronize()
        got = numpy(res)
        assert all(_bits(got[f]) == _bits(want[f]) for f in want), [f for f in want if _bits(got[f]) != _bits(want[f])]
        assert sw.holds('decoy'), 'the inputs were written after the trailing copy, or the copy did not run'


# ----------------------------------------------------------------------------------------------------------------------- the chain
def _take_reads(reads, lo, hi):
    off = np.asarray(reads['off'], np.int64)
    return dict(chrom=reads['chrom'][lo:hi], strand=reads['strand'][lo:hi], start=reads['start'][lo:hi], off=off[lo:hi + 1] - off[lo],
                norm_mean=reads['norm_mean'][off[lo]:off[hi]], base=reads['base'][off[lo]:off[hi]])


def _four_samples():
    """readllr_ref.chain_inputs, the builder of K15's chain test: two control replicates of 60 canonical reads, two replicates of 60
    reads half of which are modified at the planted base (the modified table 2 sd higher there), all over one reference"""
    import readllr_ref as RF
    mod, model, alt, planted = RF.chain_inputs(n_reads=120, shift_sd=2.0)
    canon, _, _, planted0 = RF.chain_inputs(n_reads=240, shift_sd=0.0)
    assert planted0 == planted
    return [_take_reads(canon, 120, 180), _take_reads(canon, 180, 240)], [_take_reads(mod, 0, 60), _take_reads(mod, 60, 120)], model, alt, planted


def test_chain_and_command_line_find_the_planted_site(capsys, tmp_path):
    import os
    from nanomod_amd import cli, container, kmermodel
    from nanomod_amd import readllr as RL
    c, m, model, alt, planted = _four_samples()
    lines = []
    sites = RL.compare_reads_llr_rep(c, m, model, alt, min_coverage=5, fdr='bh', log=lines.append)
    assert len(lines) == 1 and lines[0].startswith('readdiff: 2 and 2 sample(s) of 60, 60, 60, 60 read(s)')
    assert list(sites)[-2:] == ['q', 'rep_status'] and len(sites['pos']) > 400 and sites['pi_s'].shape == (len(sites['pos']), 4)
    est = (sites['rep_status'] & L.REP_NO_ESTIMATE) == 0
    assert est.sum() > 200 and (sites['n_valid'][est] >= 3).all()
    for strand in '+-':
        sel = np.flatnonzero((sites['strand'] == strand) & est)
        at = sel[sites['pos'][sel] == planted]
        assert len(at) == 1
        i = at[0]
        assert 0.2 < sites['delta'][i] < 0.8 and sites['pi0'][i] < 0.15 and sites['pi_s'][i, :2].mean() < sites['pi_s'][i, 2:].mean()
        assert sites['p_cond'][i] < 0.01 and sites['p_rep'][i] < np.median(sites['p_rep'][sel])
    # the same chain through the command line, comma-separated replicates
    paths = {}
    for n, r in (('c0', c[0]), ('c1', c[1]), ('m0', m[0]), ('m1', m[1])):
        paths[n] = str(tmp_path / (n + '.npz'))
        container.save_reads(paths[n], *[r[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
    zeros = np.zeros(64, np.int64)
    for n, t in (('model', model), ('alt', alt)):
        paths[n] = str(tmp_path / (n + '.npz'))
        kmermodel.save_kmer_model(paths[n], dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=t['mean'], sd=t['sd'],
                                                 n_positions=t['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
    out = str(tmp_path / 'out')
    capsys.readouterr()
    assert cli.main(['readdiff', '--wrkBase1', paths['c0'] + ',' + paths['c1'], '--wrkBase2', paths['m0'] + ',' + paths['m1'], '--kmerModel', paths['model'],
                     '--altModel', paths['alt'], '--FileID', 'run', '--outFolder', out, '--minCoverage', '5', '--fdr', 'bh']) == 0
    printed = capsys.readouterr().out
    assert 'readdiff: 2 and 2 sample(s)' in printed and 'run_site_diff_rep.txt' in printed
    assert os.listdir(out) == ['run_site_diff_rep.txt']
    u = [ln.split() for ln in open(os.path.join(out, 'run_site_diff_rep.txt')).read().splitlines()]
    assert len(u) == len(sites['pos']) and all(len(r) == 5 + 8 + 12 + 2 for r in u)
    assert [int(r[2]) for r in u] == (sites['pos'] + 1).tolist() and [int(r[-1]) for r in u] == sites['rep_status'].tolist()
    assert [r[-3] for r in u] == ['%.3E' % v if v == v else 'nan' for v in sites['p_rep']]
    assert [r[-2] for r in u] == ['%.3E' % v if v == v else 'nan' for v in sites['q']]
    assert [r[6] for r in u] == ['%.6f' % v if v == v else 'nan' for v in sites['pi_s'][:, 0]]
