"""CPU: the restatement of nmod_read_classes_step (tests/classes_ref.py) against itself — the device's order against mpmath within
the derived gates and against a dense brute force —, the EM loop's monotonicity, the one-class case against K19's ll_indep and K14's
estimate, readllr.fit_classes and the seeded starts, the writers' bytes, the refusals of the Python layer, and the planted classes."""
import math
import os
import re

import numpy as np
import pytest

import classes_ref as K
import hmm_ref as H
import stoich_ref as ST
from nanomod_amd import _lib as L
from nanomod_amd import engine, readllr

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'nanomod_hip.h')


def test_the_constants_are_the_headers():
    text = open(HEADER).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define NMOD_CLASSES_(\w+) (\d+)', text)}
    assert got == dict(MAX=K.CLASSES_MAX, SMALL=K.SMALL, WAVE=K.WAVE) == dict(MAX=L.CLASSES_MAX, SMALL=L.CLASSES_SMALL, WAVE=L.CLASSES_WAVE)
    assert K.WAVE_MAX == L.HMM_WAVE_MAX and K.NO_SITE == L.HMM_NO_SITE
    assert 'nmod_read_class_rows' in L._SIGNATURES and 'nmod_read_classes_step' in L._SIGNATURES
    assert engine.CLASSES_OUTPUTS == ('gamma', 'll', 'cls', 'status', 'theta_out', 'n_site', 'w_out', 'sums')
    assert len(L.CLASSES_SUMS) == K.SUMS


# ------------------------------------------------------------------------------------------------------------ (a), (b) and the dense form
EXTREME = np.array([0.0, 0.5, -0.5, 40.0, -40.0, 745.0, -745.0, 3.0, -2.0])


def _extreme_rows(rng, n_reads=40, n_sites=9):
    """reads of 0 .. n_sites entries with scores at 0, +-0.5, +-40 and +-745, every site covered, one read without an entry"""
    cover = rng.random((n_reads, n_sites)) < 0.5
    cover[0] = False
    cover[1] = True
    hoff = np.zeros(n_reads + 1, np.int64)
    hoff[1:] = np.cumsum(cover.sum(1))
    rr, ss = np.nonzero(cover)
    return K.rows_from_entries(hoff, ss, EXTREME[rng.integers(0, len(EXTREME), len(rr))], n_sites)


def _theta_with_clamps(rng, n_sites, nc):
    theta = rng.uniform(0.02, 0.98, (n_sites, nc))
    theta[0], theta[1] = K.LO, K.HI
    theta[2, ::2], theta[2, 1::2] = K.LO, K.HI
    return theta


@pytest.mark.parametrize('nc', [1, 2, 3, 8])
def test_the_devices_order_against_mpmath_and_the_dense_form(nc):
    rng = np.random.default_rng(2200 + nc)
    rows = _extreme_rows(rng)
    theta = _theta_with_clamps(rng, 9, nc)
    w = rng.dirichlet(np.full(nc, 3.0)) if nc > 1 else np.ones(1)
    a, exact = K.step_ref(rows, theta, w), K.step_mp(rows, theta, w)
    worst = {f: float(e.max()) for f, e in K.errors_against_mp(a, exact).items()}
    print('C = %d: the largest errors of the device-order restatement against mpmath, in gates: %s' % (nc, worst))
    assert all(v <= 1.0 for v in worst.values()), worst
    assert np.array_equal(a['status'], exact['status']) and a['status'][0] == K.NO_SITE and a['cls'][0] == -1 and not a['gamma'][0].any() and a['ll'][0] == 0.0
    ok = K.decided(exact)
    assert ok.sum() >= 0.9 * (exact['status'] == 0).sum()
    assert np.array_equal(a['cls'][ok], np.array([int(np.argmax([float(v) for v in g])) for g in exact['gamma']])[ok])
    for other, name in ((K.step_vec(rows, theta, w), 'vectorised'), (K.step_dense(rows, theta, w), 'dense')):
        worst = {f: float(e.max()) for f, e in K.errors_against_mp(other, exact).items()}
        assert all(v <= 1.0 for v in worst.values()), (name, worst)
        assert np.array_equal(np.asarray(other['cls'])[ok], a['cls'][ok]), name
    v = K.step_vec(rows, theta, w)
    assert np.allclose(v['sums'], a['sums'], rtol=1e-12, atol=1e-12) and np.allclose(v['w_out'], a['w_out'], rtol=1e-12)
    assert a['sums'][1] == (np.diff(rows['hoff']) > 0).sum() and a['sums'][2] == len(rows['s']) and abs(a['w_out'].sum() - 1.0) < 1e-12


def test_a_class_that_no_read_prefers_keeps_its_theta():
    """class 1 has theta 1e-9 where every score is +745, at 40 sites of every read: each costs it log(1e-9 / 0.9), 40 of them more than
    exp can hold: its weight in every read underflows, N is 0 and theta_out stays theta_in"""
    n, ns = 6, 40
    hoff = np.arange(0, (n + 1) * ns, ns, dtype=np.int64)
    rows = K.rows_from_entries(hoff, np.tile(np.arange(ns), n), np.full(n * ns, 745.0), ns)
    theta = np.stack((np.full(ns, 0.9), np.full(ns, K.LO)), 1)
    a = K.step_ref(rows, theta, np.array([0.5, 0.5]))
    assert np.all(a['gamma'][:, 1] == 0.0) and np.all(a['n_site'][:, 1] == 0.0) and np.array_equal(a['theta_out'][:, 1], theta[:, 1])
    assert np.all(a['theta_out'][:, 0] == K.HI) and a['sums'][4:].tolist() == [float(n), 0.0] and a['w_out'].tolist() == [1.0, 0.0]
    exact = K.step_mp(rows, theta, np.array([0.5, 0.5]))
    assert all(float(e.max()) <= 1.0 for e in K.errors_against_mp(a, exact).values())


# ------------------------------------------------------------------------------------------------------------ EM
@pytest.mark.parametrize('seed', [221, 222, 223])
def test_em_never_lowers_the_log_likelihood(seed):
    """60 steps from a seeded start.  SUM ll may fall by rounding alone: by no more than the sum of the reads' gates of ll, taken at the
    first and at the last step (the larger)"""
    rows, _, _ = K.planted_rows(seed, n_reads=150, n_sites=20)
    theta0 = readllr.class_starts(np.full(20, 0.45), 2, 1, seed)[0]
    fit = K.em_ref(rows, theta0, np.array([0.5, 0.5]), tol=-1.0, max_iter=60)
    assert fit['n_iter'] == 60 and not fit['converged']
    gate = max(float(K.step_mp(rows, th, w)['g_ll'].sum()) for th, w in ((theta0, np.array([0.5, 0.5])), (fit['theta'], fit['w'])))
    rise = np.diff(fit['trace'])
    print('seed %d: the smallest rise of SUM ll over 60 steps %.3g (the gate of a fall %.3g)' % (seed, rise.min(), gate))
    assert rise.min() >= -gate and fit['trace'][-1] > fit['trace'][0] + 1.0


def test_one_class_is_independence_with_a_pi_per_site():
    rows, _, _ = K.planted_rows(224, n_reads=120, n_sites=10)
    rng = np.random.default_rng(224)
    theta = rng.uniform(0.1, 0.9, (10, 1))
    a = K.step_ref(rows, theta, np.ones(1))
    exact = K.step_mp(rows, theta, np.ones(1))
    has = np.diff(rows['hoff']) > 0
    assert np.all(a['gamma'][has] == 1.0) and np.all(a['cls'][has] == 0) and a['w_out'].tolist() == [1.0]
    # ll is K19's ll_indep with the site's theta as pi
    for r in np.flatnonzero(has):
        ind = 0.0
        for row in range(rows['hoff'][r], rows['hoff'][r + 1]):
            pi = float(theta[rows['site'][row], 0])
            e0, e1 = H.emission(float(rows['s'][row]))
            ind += math.log((1.0 - pi) * e0 + pi * e1) + max(float(rows['s'][row]), 0.0)
        assert abs(a['ll'][r] - ind) <= 2.0 * exact['g_ll'][r], r
    # the fixed point is K14's estimate, site by site
    fit = K.em_ref(rows, np.full((10, 1), 0.5), np.ones(1), tol=0.0, max_iter=5000)
    for j in range(10):
        lst = rows['srow'][rows['soff'][j]:rows['soff'][j + 1]]
        pi = ST.row(rows['s'][lst], estimate_only=True)['pi']
        assert 0.0 < pi < 1.0 and abs(fit['theta'][j, 0] - pi) <= 1e-6, (j, pi, fit['theta'][j, 0])


# ------------------------------------------------------------------------------------------------------------ fit_classes and the starts
def test_fit_classes_is_the_loop_of_the_restatement():
    rows, _, _ = K.planted_rows(225, n_reads=150, n_sites=16)
    theta0 = readllr.class_starts(np.full(16, 0.4), 2, 1, 3)[0]
    w0 = np.array([0.5, 0.5])
    calls = []

    def step(theta, w):
        res = K.step_vec(rows, theta, w)
        calls.append(float(res['sums'][0]))
        return res['theta_out'], res['w_out'], res['sums'].tolist()
    fit = readllr.fit_classes(step, theta0, w0)
    ref = K.em_ref(rows, theta0, w0)
    assert fit['converged'] and fit['n_iter'] == ref['n_iter'] == len(calls) and fit['trace'] == ref['trace'] == calls and fit['ll'] == ref['ll']
    assert np.array_equal(fit['theta'], ref['theta']) and np.array_equal(fit['w'], ref['w'])
    # the stopping rule: the last rise is at most tol (|ll| + 1), the one before is not
    tr = fit['trace']
    assert tr[-1] - tr[-2] <= 1e-9 * (abs(tr[-1]) + 1.0) < tr[-2] - tr[-3]
    # ll is SUM ll at the parameters returned
    assert K.step_vec(rows, fit['theta'], fit['w'])['sums'][0] == fit['ll']
    # max_iter
    del calls[:]
    short = readllr.fit_classes(step, theta0, w0, max_iter=5)
    assert not short['converged'] and short['n_iter'] == 5 == len(calls) and short['trace'] == tr[:5]
    assert K.step_vec(rows, short['theta'], short['w'])['sums'][0] == short['ll']
    for bad in (dict(tol=-1.0), dict(tol=float('nan')), dict(max_iter=0), dict(max_iter=2.5)):
        with pytest.raises(ValueError):
            readllr.fit_classes(step, theta0, w0, **bad)


def test_the_starts_are_seeded_and_the_labels_go_by_weight():
    pihat = np.array([0.2, np.nan, 0.99, 0.0, 0.5])
    a, b = readllr.class_starts(pihat, 3, 4, 7), readllr.class_starts(pihat, 3, 4, 7)
    assert len(a) == 4 and all(x.shape == (5, 3) and np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], readllr.class_starts(pihat, 3, 1, 8)[0])
    assert not np.array_equal(a[0][:, :2], readllr.class_starts(pihat, 2, 1, 7)[0])               # the count of classes is part of the seed
    z = np.random.default_rng([7, 3, 2]).standard_normal((5, 3))
    p = np.array([0.2, 0.5, 0.95, 0.05, 0.5])
    assert np.allclose(a[2], 1.0 / (1.0 + np.exp(-(np.log(p / (1.0 - p))[:, None] + z))), rtol=1e-14)
    for bad in ((pihat, 0, 1, 0), (pihat, 9, 1, 0), (pihat, 2, 0, 0), (pihat, 2, 1, -1), (pihat, 2.5, 1, 0)):
        with pytest.raises(ValueError):
            readllr.class_starts(*bad)
    assert readllr.class_order([0.2, 0.5, 0.3]).tolist() == [1, 2, 0] and readllr.class_order([0.25, 0.5, 0.25]).tolist() == [1, 0, 2]
    assert readllr.class_order([1.0]).tolist() == [0]
    # BIC and the choice
    assert readllr.class_bic(-100.0, 2, 40, 600) == 200.0 + (1 + 80) * math.log(600.0)
    assert readllr.class_bic(-100.0, 1, 40, 600) == 200.0 + 40 * math.log(600.0) and readllr.class_bic(-1.0, 2, 3, 0) == math.inf
    fits = [dict(C=1, start=0, ll=-50.0, bic=130.0), dict(C=2, start=0, ll=-40.0, bic=120.0), dict(C=2, start=1, ll=-40.0, bic=120.0),
            dict(C=2, start=2, ll=-39.0, bic=118.0), dict(C=3, start=0, ll=-38.5, bic=118.0)]
    best, profile, chosen = readllr.choose_classes(fits)
    assert best[2] is fits[3] and profile == [(1, -50.0, 130.0), (2, -39.0, 118.0), (3, -38.5, 118.0)] and chosen is fits[3]
    assert readllr.choose_classes(fits[:3])[0][2] is fits[1]                                        # the first of equals
    for bad in ([], [0], [9], [2.5], 0):
        with pytest.raises(ValueError):
            readllr._classes_list(bad)
    assert readllr._classes_list(3) == [3] and readllr._classes_list((1, 2)) == [1, 2]


# ------------------------------------------------------------------------------------------------------------ the writers
def test_the_writers_bytes(tmp_path):
    res = dict(C=2,
               reads=dict(index=np.arange(3), chrom=np.array(['chrA', 'chrA', 'chrB']), strand=np.array(['+', '-', '+']), n_sites=np.array([4, 0, 2], np.int32),
                          cls=np.array([1, -1, 0], np.int32), gamma=np.array([0.75, 0.0, 0.999999949]), ll=np.array([-1.5, 0.0, 12.3456789])),
               sites=dict(chrom=np.array(['chrA', 'chrB']), strand=np.array(['+', '-']), pos=np.array([9, 99]),
                          theta=np.array([[0.8, 0.1], [1e-9, 0.25]]), n=np.array([[1.5, 0.5], [0.0, 2.0]])),
               fit=[dict(C=1, start=0, w=(1.0,), ll=-10.0, bic=25.5, n_iter=3, converged=True, kept=True),
                    dict(C=2, start=1, w=(0.65, 0.35), ll=-8.25, bic=27.125, n_iter=500, converged=False, kept=False)])
    paths = [str(tmp_path / n) for n in ('r.txt', 's.txt', 'f.txt')]
    readllr.write_read_classes(paths[0], res)
    readllr.write_class_sites(paths[1], res)
    readllr.write_classes_fit(paths[2], res)
    assert open(paths[0]).read() == ('read\tchrom\tstrand\tn_sites\tclass\tgamma\tll\n0\tchrA\t+\t4\t1\t0.750000\t-1.500000\n'
                                     '1\tchrA\t-\t0\t-1\t0.000000\t0.000000\n2\tchrB\t+\t2\t0\t1.000000\t12.345679\n')
    assert open(paths[1]).read() == ('chrom\tstrand\tpos\ttheta_0\tN_0\ttheta_1\tN_1\nchrA\t+\t10\t0.800000\t1.500\t0.100000\t0.500\n'
                                     'chrB\t-\t100\t0.000000\t0.000\t0.250000\t2.000\n')
    assert open(paths[2]).read() == ('C\tstart\tweights\tll\tBIC\titerations\tconverged\tkept\n1\t0\t1.000000\t-10.000000\t25.500000\t3\t1\t1\n'
                                     '2\t1\t0.650000,0.350000\t-8.250000\t27.125000\t500\t0\t0\n')


# ------------------------------------------------------------------------------------------------------------ refusals
def test_the_python_layer_refuses_before_the_library_is_loaded(monkeypatch):
    def no_load():
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(L, 'load', no_load)
    rows, _, _ = K.planted_rows(226, n_reads=8, n_sites=5)
    theta, w = np.full((5, 2), 0.5), np.array([0.5, 0.5])
    step = engine.read_classes_step_host
    bad_rows = lambda **kw: dict(rows, **kw)
    cases = [
        (rows, theta, np.full(9, 1.0 / 9)), (rows, theta, np.zeros(0)), (rows, theta, np.array([0.5, 0.4])), (rows, theta, np.array([1.0, 0.0])),
        (rows, theta, np.array([0.5, np.nan])), (rows, theta, np.array([1.0 + 1e-8, -1e-8])), (rows, np.full((5, 1), 0.5), np.array([0.9])),
        (rows, np.full((5, 3), 0.5), w), (rows, np.full((4, 2), 0.5), w), (rows, np.full((5, 2), 0.0), w), (rows, np.full((5, 2), 1.0), w),
        (rows, np.full((5, 2), np.nan), w), (rows, np.full((5, 2), 1e-10), w),
        (bad_rows(hoff=rows['hoff'] + 1), theta, w), (bad_rows(hoff=rows['hoff'][::-1].copy()), theta, w), (bad_rows(hoff=rows['hoff'][:-1]), theta, w),
        (bad_rows(soff=rows['soff'] + 1), theta, w), (bad_rows(soff=rows['soff'][::-1].copy()), theta, w),
        (bad_rows(soff=np.concatenate((rows['soff'][:-1], [rows['soff'][-1] - 1]))), theta, w),
        (bad_rows(site=rows['site'][:-1]), theta, w), (bad_rows(s=rows['s'][:-1]), theta, w), (bad_rows(rread=rows['rread'][:-1]), theta, w),
        (bad_rows(srow=rows['srow'][:-1]), theta, w),
    ]
    for i, (r, th, ww) in enumerate(cases):
        with pytest.raises(ValueError):
            step(r, th, ww)
            pytest.fail('case %d was not refused' % i)
    with pytest.raises(ValueError):
        step(rows, theta, w, want=('gamma', 'post'))
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError):
            engine._classes_opts(bad, ())
    # one class: the weight 1 is the only one there is
    assert engine._check_class_params(np.full((5, 1), 0.5), np.ones(1), 5)[2] == 1
    # the rows
    key = np.array([5, 9, 12], np.int64)
    reads = (np.zeros(2, np.int32), np.array([0, 3], np.int64), np.array([0, 10, 20], np.int64), np.zeros(20))
    for args, kw in (((reads[0], reads[1], reads[2][::-1].copy(), reads[3], key), {}), ((reads[0][:1],) + reads[1:] + (key,), {}),
                     (reads + (key[::-1].copy(),), {}), (reads + (key,), dict(hoff=np.array([0, 2]))), (reads + (key,), dict(hoff=np.array([1, 2, 3]))),
                     (reads + (key,), dict(hoff=np.array([0, 2, 1]))), (reads + (key,), dict(hoff=np.array([0, 1, 2]), want=('site', 'x'))),
                     (reads + (np.zeros(0, np.int64),), dict(hoff=np.array([0, 1, 2])))):
        with pytest.raises(ValueError):
            engine.read_class_rows_host(*args, **kw)
    with pytest.raises(ValueError):
        readllr.cluster_reads_llr(None, None, None, classes=[2, 9])
    with pytest.raises(ValueError):
        readllr.cluster_reads_llr(None, None, None, n_init=0)
    with pytest.raises(ValueError):
        readllr.cluster_reads_llr(None, None, None, max_iter=0)


def test_the_command_line_checks_its_flags(tmp_path, capsys):
    from nanomod_amd import cli
    assert cli.parse_classes('2') == [2] and cli.parse_classes('1,2,3') == [1, 2, 3] and cli.parse_classes('2,x') is None and cli.parse_classes('') is None
    base = ['readclasses', '--wrkBase1', str(tmp_path / 'none.npz'), '--model', str(tmp_path / 'm.npz'), '--altModel', str(tmp_path / 'a.npz')]
    assert cli.main(base + ['--classes', '0,2', '--nInit', '0', '--seed', '-1', '--maxIter', '0', '--tol', '-1']) == 1
    out = capsys.readouterr().out
    for flag in ('--classes', '--nInit', '--seed', '--maxIter', '--tol', 'does not exist'):
        assert flag in out, flag
    a = cli.build_parser().parse_args(base)
    assert (a.classes, a.nInit, a.seed, a.maxIter, a.tol, a.sites) == ('2', 4, 0, 500, 1e-9, 'stoich')


# ------------------------------------------------------------------------------------------------------------ planted classes
def test_the_planted_classes_are_found():
    """600 reads, 40 sites, coverage 0.6, shares 0.35 and 0.65, theta 0.8 / 0.1 on the two halves of the sites and the reverse, scores
    d (x - d / 2) with d = 2: the hard classes of the best of 4 starts agree with the planted ones on at least 98 % of the reads with
    an entry, up to relabelling"""
    rows, z, theta = K.planted_rows()
    assert len(z) == 600 and theta.shape == (40, 2) and abs(len(rows['s']) / (600 * 40) - 0.6) < 0.02 and abs((z == 0).mean() - 0.35) < 0.05
    pihat = np.array([ST.row(rows['s'][rows['srow'][rows['soff'][j]:rows['soff'][j + 1]]], estimate_only=True)['pi'] for j in range(40)])
    fits = [K.em_ref(rows, th0, np.array([0.5, 0.5])) for th0 in readllr.class_starts(pihat, 2, 4, 0)]
    best = max(fits, key=lambda f: f['ll'])
    share = K.agreement(best['last']['cls'], z)
    order = readllr.class_order(best['w'])
    print('planted classes: agreement %.4f, weights %s, %s steps' % (share, best['w'][order], [f['n_iter'] for f in fits]))
    assert all(f['converged'] for f in fits) and share >= 0.98
    assert np.allclose(best['w'][order], [0.65, 0.35], atol=0.05) and np.abs(best['theta'][:, order] - theta[:, ::-1]).max() < 0.15
    # BIC prefers two classes to one and to three
    bic = {}
    for nc in (1, 2, 3):
        f = max((K.em_ref(rows, th0, np.full(nc, 1.0 / nc)) for th0 in readllr.class_starts(pihat, nc, 4, 0)), key=lambda f: f['ll'])
        bic[nc] = readllr.class_bic(f['ll'], nc, 40, int(f['last']['sums'][1]))
    assert bic[2] < bic[1] and bic[2] < bic[3], bic
