"""nmod_site_diff (K15) on the GPU against the numpy restatement of its definition (tests/diff_ref.py, pinned against mpmath in
tests/test_site_diff.py): parity over every pair of row lengths at which the code takes another path and over the content of the
rows, the symmetries of the definition, the agreement of the test with the interval and with three calls of nmod_site_stoich, the
independence of a site's bits from everything but the site, and batches larger than the persistent grids.  The gates are diff_ref's."""
import numpy as np
import pytest

import diff_ref as F
import stoich_ref as SR
from nanomod_amd import _lib as L
from nanomod_amd.engine import site_diff_host, site_stoich_host          # K15's entry: without it nothing here can pass

pytestmark = pytest.mark.gpu

INT_FIELDS = ('n_valid0', 'n_valid1', 'iters', 'status')
_worst = {}                                             # the worst ratio of a deviation to its gate over the session, printed per test


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _share(name, dev, gate, worst):
    if gate == 0.0:
        assert dev == 0.0, '%s differs where its gate is 0: %r' % (name, dev)
        return
    worst[name] = max(worst.get(name, 0.0), dev / gate)


def _check_sites(got, exp, rows=None, converged=True, interval=True):
    """status, the counts and the NaN pattern exactly; both ends of [0, 1] and of [-1, 1] exactly; everything else within the gates"""
    worst = {}
    fields = [f for f in F.FIELDS if interval or f not in ('delta_lo', 'delta_hi')]
    for i in (range(len(exp)) if rows is None else rows):
        e = exp[i]
        assert (int(got['status'][i]), int(got['n_valid0'][i]), int(got['n_valid1'][i])) == (e['status'], e['n_valid0'], e['n_valid1']), \
            (i, got['status'][i], e['status'], got['n_valid0'][i], got['n_valid1'][i])
        if e['gates'] is None:
            assert all(np.isnan(got[f][i]) for f in fields) and got['iters'][i] == 0, i
            continue
        assert not any(np.isnan(got[f][i]) for f in fields), i
        for f in ('pi0', 'pi1', 'pi_pool'):
            assert 0.0 <= got[f][i] <= 1.0 and (got[f][i] in (0.0, 1.0)) == (e[f] in (0.0, 1.0)), (i, f, got[f][i], e[f])
        if interval:
            assert -1.0 <= got['delta_lo'][i] <= got['delta'][i] <= got['delta_hi'][i] <= 1.0, i
            assert (got['delta_lo'][i] == -1.0) == (e['delta_lo'] == -1.0) and (got['delta_hi'][i] == 1.0) == (e['delta_hi'] == 1.0), i
        if not converged:
            continue
        g = e['gates']
        for f in fields:
            if f != 'p_diff':
                _share(f, abs(got[f][i] - e[f]), g[f], worst)
        lo, hi = g['p_diff']
        assert lo <= got['p_diff'][i] <= hi, (i, lo, got['p_diff'][i], hi)
    for k, v in worst.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    fmt = lambda w: ', '.join('%s %.3g' % kv for kv in sorted(w.items())) or 'none compared'
    print('worst deviation as a share of its gate: %s (over the session: %s)' % (fmt(worst), fmt(_worst)))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_parity_over_the_row_lengths():
    s0, o0, s1, o1 = F.length_batch()
    n0, n1 = np.diff(o0), np.diff(o1)
    assert set(F.LENGTHS) <= set(n0[n0 == n1].tolist()) and (n0 + n1 == F.STAGE).any() and (n0 + n1 == F.STAGE + 1).any()
    for mv in (3, 1):
        exp = F.expected('length', min_valid=mv)
        _check_sites(site_diff_host(s0, o0, s1, o1, min_valid=mv), exp)
    assert sum(e['gates'] is not None for e in exp) >= len(exp) - 1


@pytest.mark.parametrize('min_valid', [1, 3, 6])
def test_content(min_valid):
    s0, o0, s1, o1 = F.content_batch()
    exp = F.expected('content', min_valid=min_valid)
    _check_sites(site_diff_host(s0, o0, s1, o1, min_valid=min_valid), exp)
    st = np.array([e['status'] for e in exp])
    assert (st & F.TOO_FEW).any() and (st == 0).any() and (st & F.POOL_AT_END).any()
    if min_valid == 1:
        assert (st & F.FLAT).any()


def test_one_evaluation_and_no_tolerance():
    s0, o0, s1, o1 = F.content_batch()
    for kw in (dict(max_iter=1), dict(tol=0.0, max_iter=30)):
        exp = F.expected('content', **kw)
        got = site_diff_host(s0, o0, s1, o1, **kw)
        _check_sites(got, exp, converged=False)
        interior = [i for i, e in enumerate(exp) if e['gates'] is not None and 0.0 < e['pi_pool'] < 1.0]
        assert interior and all(got['iters'][i] == kw['max_iter'] and got['status'][i] & F.NOT_CONVERGED for i in interior)


def _gates_of(exp, f):
    return np.array([e['gates'][f] if e['gates'] is not None else 0.0 for e in exp])


def test_swapping_the_samples():
    s0, o0, s1, o1 = F.content_batch()
    exp = F.expected('content')
    a, b = site_diff_host(s0, o0, s1, o1), site_diff_host(s1, o1, s0, o0)
    est = np.array([e['gates'] is not None for e in exp])
    assert np.array_equal(a['status'], b['status']) and np.array_equal(a['n_valid0'], b['n_valid1'])
    assert _bits(a['pi0']) == _bits(b['pi1']) and _bits(a['pi1']) == _bits(b['pi0']) and _bits(a['pi_pool']) == _bits(b['pi_pool'])
    assert np.array_equal(a['delta'][est], -b['delta'][est])
    for f, g in (('delta_lo', 'delta_hi'), ('delta_hi', 'delta_lo')):
        assert (np.abs(a[f][est] + b[g][est]) <= (_gates_of(exp, f) * 2.0)[est]).all()
    assert (np.abs(a['stat'][est] - b['stat'][est]) <= (_gates_of(exp, 'stat') * 2.0)[est]).all()


def test_the_same_row_in_both_samples():
    s0, o0, _, _ = F.content_batch()
    got = site_diff_host(s0, o0, s0, o0)
    exp = F.site_diff(s0, o0, s0, o0)
    est = np.array([e['gates'] is not None for e in exp])
    assert est.sum() >= 30 and _bits(got['pi0']) == _bits(got['pi1'])
    assert (got['delta'][est] == 0.0).all() and (got['stat'][est] <= _gates_of(exp, 'stat')[est]).all()
    assert (got['delta_lo'][est] <= 0.0).all() and (got['delta_hi'][est] >= 0.0).all()


def test_the_test_and_the_interval_are_one_statement():
    s0, o0, s1, o1 = F.content_batch()
    exp = F.expected('content')
    got = site_diff_host(s0, o0, s1, o1, ci_level=0.95)
    drop, seen = SR.DEFAULTS['ci_drop'], [0, 0]
    for i, e in enumerate(exp):
        if e['gates'] is None:
            continue
        inside = got['delta_lo'][i] <= 0.0 <= got['delta_hi'][i]
        if got['stat'][i] > drop + e['gates']['stat']:
            seen[0] += 1
            assert not inside, i
        elif got['stat'][i] < drop - e['gates']['stat']:
            seen[1] += 1
            assert inside, i
    assert min(seen) >= 5, seen


def test_against_three_calls_of_site_stoich():
    s0, o0, s1, o1 = F.content_batch()
    exp = F.expected('content')
    rows = [np.concatenate([s0[o0[i]:o0[i + 1]], s1[o1[i]:o1[i + 1]]]) for i in range(len(o0) - 1)]
    cat, oc = SR._csr(rows)
    got = site_diff_host(s0, o0, s1, o1)
    k0, k1, kc = site_stoich_host(s0, o0), site_stoich_host(s1, o1), site_stoich_host(cat, oc)
    r0, r1, rc = SR.site_stoich(s0, o0), SR.site_stoich(s1, o1), SR.site_stoich(cat, oc)
    seen = 0
    for i, e in enumerate(exp):
        if e['gates'] is None or any(r[i]['gates'] is None for r in (r0, r1, rc)):
            continue
        seen += 1
        assert abs(got['pi0'][i] - k0['pi'][i]) <= e['gates']['pi0'] + r0[i]['gates']['pi']
        assert abs(got['pi1'][i] - k1['pi'][i]) <= e['gates']['pi1'] + r1[i]['gates']['pi']
        assert abs(got['pi_pool'][i] - kc['pi'][i]) <= e['gates']['pi_pool'] + rc[i]['gates']['pi']
        three = k0['stat'][i] + k1['stat'][i] - kc['stat'][i]
        if np.isfinite(three):
            gate = e['gates']['stat'] + r0[i]['gates']['stat'] + r1[i]['gates']['stat'] + rc[i]['gates']['stat'] + 8.0 * SR.EPS * kc['stat'][i]
            assert abs(max(three, 0.0) - got['stat'][i]) <= gate, (i, three, got['stat'][i], gate)
    assert seen >= 30


def _take(s, o, idx):
    rows = [s[o[i]:o[i + 1]] for i in idx]
    return SR._csr(rows)


def test_a_sites_bits_depend_on_the_site_alone():
    import torch
    from nanomod_amd import engine
    s0, o0, s1, o1 = F.length_batch()
    full = site_diff_host(s0, o0, s1, o1)
    n = len(o0) - 1
    names = list(F.FIELDS) + list(INT_FIELDS)
    # shuffled
    perm = np.random.default_rng(1505).permutation(n)
    a0, p0 = _take(s0, o0, perm)
    a1, p1 = _take(s1, o1, perm)
    sh = site_diff_host(a0, p0, a1, p1)
    for f in names:
        assert _bits(sh[f]) == _bits(full[f][perm]), f
    # alone: one site of each form
    lens = np.maximum(np.diff(o0), np.diff(o1))
    for i in (int(np.argmax(lens == 9)), int(np.argmax(lens == F.SMALL + 1)), int(np.argmax(lens == F.WAVE + 1)), n - 1):
        b0, q0 = _take(s0, o0, [i])
        b1, q1 = _take(s1, o1, [i])
        one = site_diff_host(b0, q0, b1, q1)
        for f in names:
            assert _bits(one[f]) == _bits(full[f][i:i + 1]), (i, f)
    # stride against CSR, one sample each way
    eq = [i for i in range(n) if o0[i + 1] - o0[i] == 9]
    b0, q0 = _take(s0, o0, eq * 3)
    b1, q1 = _take(s1, o1, eq * 3)
    csr = site_diff_host(b0, q0, b1, q1)
    for kw, args in ((dict(stride0=9), (b0, None, b1, q1)), (dict(stride1=9), (b0, q0, b1, None)), (dict(stride0=9, stride1=9), (b0, None, b1, None))):
        st = site_diff_host(*args, **kw)
        for f in names:
            assert _bits(st[f]) == _bits(csr[f]), (kw, f)
    # device memory, without the interval, with fewer outputs
    det = engine.DeviceDetector(device=0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dev = det.site_diff(t(s0), t(s1), off0=t(o0), off1=t(o1))
    for f in names:
        assert _bits(dev[f].cpu().numpy()) == _bits(full[f]), f
    no = site_diff_host(s0, o0, s1, o1, interval=False)
    assert 'delta_lo' not in no and 'delta_hi' not in no
    for f in no:
        assert _bits(no[f]) == _bits(full[f]), f
    few = {f: torch.empty(n, dtype=torch.float64, device='cuda') for f in ('stat', 'delta_hi')}
    lib, opts = L.load(), engine._diff_opts(3, 0.95, 60, 1e-12)
    import ctypes as C
    out = L.make_out(L.NmodDiffOut, **{f: v.data_ptr() for f, v in few.items()})
    prm = det._params(L.DTYPE_F64, 0, 0, 0, 0)
    d0, d1, e0, e1 = t(s0), t(s1), t(o0), t(o1)
    L.check(lib.nmod_site_diff(C.byref(prm), n, d0.data_ptr(), e0.data_ptr(), d1.data_ptr(), e1.data_ptr(), C.byref(opts), C.byref(out)))
    torch.cuda.synchronize()
    for f, v in few.items():
        assert _bits(v.cpu().numpy()) == _bits(full[f]), f


@pytest.mark.parametrize('form', ['lanes16', 'wave', 'workgroup'])
def test_a_batch_larger_than_the_persistent_grid(form):
    """more sites than the grid of the form walks at once (8 workgroups per CU of 16 or 4 sites each; 2 workgroups per CU of one site):
    every site equal to the same site computed alone"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    length, per_cu = dict(lanes16=(3, 8 * 16), wave=(F.SMALL + 1, 8 * 4), workgroup=(F.WAVE + 1, 2))[form]
    nsites, kinds = cus * per_cu + 37, 5
    rng = np.random.default_rng(1506)
    k0 = [SR.simulate_row(rng, length, 3.0, 0.3 + 0.1 * k) for k in range(kinds)]
    k1 = [SR.simulate_row(rng, length, 3.0, 0.8 - 0.1 * k) for k in range(kinds)]
    alone = [site_diff_host(k0[k], None, k1[k], None, stride0=length, stride1=length) for k in range(kinds)]
    assert all(a['status'][0] == 0 for a in alone)
    which = rng.integers(0, kinds, nsites)
    s0 = np.concatenate([k0[k] for k in which])
    s1 = np.concatenate([k1[k] for k in which])
    got = site_diff_host(s0, None, s1, None, stride0=length, stride1=length)
    for f in list(F.FIELDS) + list(INT_FIELDS):
        ref = np.concatenate([alone[k][f] for k in range(kinds)])[which]
        assert _bits(got[f]) == _bits(ref), f


def test_a_row_beyond_max_deep_by_offsets_only():
    """2^24 scores in row 1 of the middle site: NaN outputs and its status; its neighbours are computed"""
    n = 2 ** 24
    rng = np.random.default_rng(1507)
    a, b, c = SR.simulate_row(rng, 50, 3.0, 0.5), SR.simulate_row(rng, 40, 3.0, 0.2), SR.simulate_row(rng, 600, 1.0, 0.3)
    s0 = np.concatenate([a, b, c])
    o0 = np.array([0, 50, 90, 690], np.int64)
    s1 = np.concatenate([b, np.tile(np.array([1.0, -1.0, 0.5, -2.0]), n // 4), a])
    o1 = np.array([0, 40, 40 + n, 40 + n + 50], np.int64)
    got = site_diff_host(s0, o0, s1, o1)
    assert got['status'].tolist() == [0, F.TOO_LARGE, 0] and got['n_valid0'].tolist() == [50, 0, 600] and got['n_valid1'].tolist() == [40, 0, 50]
    assert all(np.isnan(got[f][1]) for f in F.FIELDS) and got['iters'][1] == 0
    _check_sites(got, {0: F.site(a, b), 2: F.site(c, a)}, rows=[0, 2])


def test_status_at_a_few_evaluations_is_the_sites_own():
    """max_iter = 6: some roots converge and some do not, so NOT_CONVERGED tells the sites apart.  A site whose interval end is fixed
    computes along with the other sites of its wave and must not take the bit from roots it never wanted: the status of every site
    in the batch is the status of the site alone, and the restatement's"""
    s0, o0, s1, o1 = F.content_batch()
    exp = F.expected('content', max_iter=6)
    got = site_diff_host(s0, o0, s1, o1, max_iter=6)
    _check_sites(got, exp, converged=False)
    st = np.array([e['status'] for e in exp])
    est = np.array([e['gates'] is not None for e in exp])
    assert (st[est] & F.NOT_CONVERGED).any() and not (st[est] & F.NOT_CONVERGED).all()
    fixed = [i for i, e in enumerate(exp) if e['gates'] is not None and (e['delta_lo'] == -1.0 or e['delta_hi'] == 1.0)]
    assert len(fixed) >= 4
    for i in range(len(exp)):
        a0, p0 = _take(s0, o0, [i])
        a1, p1 = _take(s1, o1, [i])
        if len(a0) == 0 or len(a1) == 0:
            continue
        one = site_diff_host(a0, p0, a1, p1, max_iter=6)
        for f in list(F.FIELDS) + list(INT_FIELDS):
            assert _bits(one[f]) == _bits(got[f][i:i + 1]), (i, f)


# ----------------------------------------------------------------------------------------------- the chain
def _take_reads(reads, lo, hi):
    off = np.asarray(reads['off'], np.int64)
    return dict(chrom=reads['chrom'][lo:hi], strand=reads['strand'][lo:hi], start=reads['start'][lo:hi], off=off[lo:hi + 1] - off[lo],
                norm_mean=reads['norm_mean'][off[lo]:off[hi]], base=reads['base'][off[lo]:off[hi]])


def _two_samples():
    """readllr_ref.chain_inputs, the builder of K14's chain test: sample 1: 60 reads, half of each strand modified at the planted base
    (the modified table 2 sd higher there); sample 0, the control: 60 canonical reads over the same reference with noise of their own
    (reads 60 .. 119 of a canonical set of 120 from the same seed)"""
    import readllr_ref as RF
    reads1, model, alt, planted = RF.chain_inputs(n_reads=60, shift_sd=2.0)
    canon, _, _, planted0 = RF.chain_inputs(n_reads=120, shift_sd=0.0)
    assert planted0 == planted
    return _take_reads(canon, 60, 120), reads1, model, alt, planted


def test_chain_finds_the_site_planted_in_sample_1_only():
    from nanomod_amd import readllr as RL
    reads0, reads1, model, alt, planted = _two_samples()
    lines = []
    sites = RL.compare_reads_llr(reads0, reads1, model, alt, fdr='bh', log=lines.append)
    assert len(lines) == 1 and lines[0].startswith('readdiff: 60 and 60 read(s)')
    assert list(sites)[-2:] == ['q', 'diff_status'] and len(sites['pos']) > 400
    k = model['k']
    est = (sites['diff_status'] & L.DIFF_NO_ESTIMATE) == 0
    far_out = []
    for strand in '+-':
        m = np.flatnonzero((sites['strand'] == strand) & est)
        at = m[sites['pos'][m] == planted]
        assert len(at) == 1 and sites['delta_lo'][at[0]] > 0.0 and 0.2 < sites['delta'][at[0]] < 0.8 and sites['pi0'][at[0]] < 0.15
        assert sites['n_valid0'][at[0]] >= 20 and sites['n_valid1'][at[0]] >= 20
        far = m[np.abs(sites['pos'][m] - planted) >= k]
        # the smallest p_diff and q of its strand but for the bases within k - 1, whose window sums share its events
        assert sites['p_diff'][at[0]] < sites['p_diff'][far].min() and sites['q'][at[0]] < sites['q'][far].min() and sites['q'][at[0]] <= 0.05
        assert abs(int(sites['pos'][m][np.argmin(sites['p_diff'][m])]) - planted) < k
        far_out.append((sites['delta_lo'][far] > 0.0) | (sites['delta_hi'][far] < 0.0))
    # elsewhere both samples are canonical (a site none of whose k-mers differs between the tables is flat and has no estimate): the
    # 95 % interval of delta holds 0 at about the nominal rate.  The bound: the largest null rejection share the CPU file measures,
    # 0.064, plus five binomial sd at the effective number of sites — the window sums of k neighbouring bases share events, so a k-th
    out = np.concatenate(far_out)
    bound = 0.064 + 5.0 * np.sqrt(0.064 * 0.936 / (len(out) / k))
    print('null sites with an estimate: %d, interval excludes 0 at %.4f (bound %.4f)' % (len(out), out.mean(), bound))
    assert len(out) >= 60 and out.mean() <= bound
    # the test and the interval agree on the chain's rows too
    drop = SR.DEFAULTS['ci_drop']
    sure = est & (np.abs(sites['stat'] - drop) > 1e-6)
    inside = (sites['delta_lo'] <= 0.0) & (sites['delta_hi'] >= 0.0)
    assert np.array_equal(inside[sure], (sites['stat'] < drop)[sure])


def test_end_to_end_through_the_command_line(capsys, tmp_path):
    from nanomod_amd import cli, container, kmermodel
    from nanomod_amd import readllr as RL
    reads0, reads1, model, alt, planted = _two_samples()
    paths = {n: str(tmp_path / (n + '.npz')) for n in ('r0', 'r1', 'model', 'alt')}
    for n, r in (('r0', reads0), ('r1', reads1)):
        container.save_reads(paths[n], *[r[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
    zeros = np.zeros(64, np.int64)
    for n, m in (('model', model), ('alt', alt)):
        kmermodel.save_kmer_model(paths[n], dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                                 n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
    out = str(tmp_path / 'out')
    capsys.readouterr()
    assert cli.main(['readdiff', '--wrkBase1', paths['r0'], '--wrkBase2', paths['r1'], '--kmerModel', paths['model'], '--altModel', paths['alt'],
                     '--FileID', 'run', '--outFolder', out, '--minCoverage', '5', '--minValid', '6', '--ciLevel', '0.9', '--fdr', 'by']) == 0
    printed = capsys.readouterr().out
    assert 'readdiff: 60 and 60 read(s)' in printed and 'run_site_diff.txt' in printed
    import os
    assert os.listdir(out) == ['run_site_diff.txt']
    want = RL.compare_reads_llr(container.load_reads(paths['r0']), container.load_reads(paths['r1']), kmermodel.load_kmer_model(paths['model']),
                                kmermodel.load_kmer_model(paths['alt']), min_coverage=5, diff=dict(min_valid=6, ci_level=0.9), fdr='by',
                                log=lambda *a: None)
    u = [ln.split() for ln in open(os.path.join(out, 'run_site_diff.txt')).read().splitlines()]
    assert len(u) == len(want['pos']) > 400 and all(len(r) == 18 for r in u)
    assert (want['n_reads0'] >= 5).all() and (want['n_reads1'] >= 5).all()
    assert [r[0] for r in u] == want['chrom'].tolist() and [r[1] for r in u] == want['strand'].tolist() and {r[3] for r in u} <= set('ACGT')
    for col, f in ((2, want['pos'] + 1), (4, want['n_reads0']), (5, want['n_reads1']), (6, want['n_valid0']), (7, want['n_valid1']), (17, want['diff_status'])):
        assert [int(r[col]) for r in u] == np.asarray(f).tolist(), col
    for col, f in enumerate(('pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi'), 8):
        assert [r[col] for r in u] == ['%.6f' % v for v in want[f]], f
    assert [r[14] for r in u] == ['%.3f' % v for v in want['stat']]
    for col, f in ((15, 'p_diff'), (16, 'q')):
        assert [r[col] for r in u] == ['%.3E' % v if v == v else 'nan' for v in want[f]], f
    row = [r for r in u if int(r[2]) == planted + 1 and r[1] == '+']
    assert len(row) == 1 and float(row[0][12]) > 0.0                      # the planted site's interval lies above 0 at 0.9 too


def test_p_diff_goes_straight_into_the_device_fdr():
    import torch
    from nanomod_amd import engine
    s0, o0, s1, o1 = F.content_batch()
    det = engine.DeviceDetector(0)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    res = det.site_diff(t(s0), t(s1), off0=t(o0), off1=t(o1))
    (q,), summary = det.fdr(res, tracks=('p_diff',), method='bh', alpha=0.05)
    torch.cuda.synchronize()
    p, q = res['p_diff'].cpu().numpy(), q.cpu().numpy()
    (want,), (summ,) = engine.fdr_adjust_host([p])
    assert _bits(q) == _bits(want) and engine.fdr_summary_dicts(summary)[0] == summ
    assert summ['tested'] == int((~np.isnan(p)).sum()) and summ['excluded'] == int(np.isnan(p).sum()) and summ['rejected'] >= 2


def test_match_score_rows_keeps_float64_whatever_the_values():
    """scores on the 0.001 grid, which nmod_select_tested's dtype word would narrow to int16 milli-units: the gathered rows are the
    float64 rows of the sites both samples hold with the coverage asked for"""
    import torch
    from nanomod_amd import engine
    t = lambda x, d: torch.tensor(x, dtype=d, device='cuda')
    g0 = dict(key=t([5, 6, 9], torch.int64), off=t([0, 2, 3, 6], torch.int64), sig=t([1.5, -2.25, 0.125, 3.0, -1.0, 2.0], torch.float64),
              base=t([65, 67, 71], torch.uint8), names=['chrT'])
    g1 = dict(key=t([5, 9, 11], torch.int64), off=t([0, 3, 5, 6], torch.int64), sig=t([0.001, 1e-7, -4.5, 7.0, 1e300, 2.0], torch.float64),
              base=t([65, 71, 84], torch.uint8), names=['chrT'])
    m = engine.match_score_rows(g0, g1, 2)
    assert m['sig0'].dtype == m['sig1'].dtype == torch.float64
    assert m['key'].tolist() == [5, 9] and m['off0'].tolist() == [0, 2, 5] and m['off1'].tolist() == [0, 3, 5] and m['base'].tolist() == [65, 71]
    assert _bits(m['sig0'].cpu().numpy()) == _bits(np.array([1.5, -2.25, 3.0, -1.0, 2.0]))
    assert _bits(m['sig1'].cpu().numpy()) == _bits(np.array([0.001, 1e-7, -4.5, 7.0, 1e300]))
    assert engine.match_score_rows(g0, g1, 3)['key'].tolist() == []
