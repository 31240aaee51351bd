"""nmod_site_stoich (K14) on the GPU against the numpy restatement of its definition (tests/stoich_ref.py, pinned against mpmath in
tests/test_site_stoich.py): parity over every row length at which the code takes another path, the content of the rows, the
independence of a row's bits from everything but the row, batches larger than the persistent grids, and the chain through the Python
layers and the command line.  The gates are stoich_ref's."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import readllr_ref as RF
import stoich_ref as F
from nanomod_amd import _lib as L
from nanomod_amd import readllr as RL
from nanomod_amd.engine import site_stoich_host          # K14's entry: without it nothing here can pass

pytestmark = pytest.mark.gpu

INT_FIELDS = ('n_valid', 'iters', 'status')
_worst = {}                                             # the worst ratio of a deviation to its gate over the session, printed per test


def _engine():
    from nanomod_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _share(name, dev, gate, worst):
    """the deviation as a share of its gate; a deviation where the gate is 0 must be 0"""
    if gate == 0.0:
        assert dev == 0.0, '%s differs where its gate is 0: %r' % (name, dev)
        return
    worst[name] = max(worst.get(name, 0.0), dev / gate)


def _check_rows(got, exp, off, rows=None, converged=True):
    """status, n_valid and the NaN pattern exactly; the estimates of a row that has one within the restatement's gates (exactly at
    either end of [0, 1]); resp, where asked for, within its gate.  converged=False: the options stop the roots early, and only the
    pattern, the order lo <= pi <= hi and the counts are compared here"""
    worst = {}
    for i in (range(len(exp)) if rows is None else rows):
        e = exp[i]
        assert int(got['status'][i]) == e['status'] and int(got['n_valid'][i]) == e['n_valid'], (i, got['status'][i], e['status'], got['n_valid'][i], e['n_valid'])
        sl = slice(int(off[i]), int(off[i + 1]))
        if 'resp' in got:
            assert np.array_equal(np.isnan(got['resp'][sl]), np.isnan(e['resp'])), (i, 'resp NaN pattern')
        if e['gates'] is None:
            assert all(np.isnan(got[f][i]) for f in F.FIELDS) and got['iters'][i] == 0, i
            continue
        assert not any(np.isnan(got[f][i]) for f in F.FIELDS), i
        assert 0.0 <= got['pi_lo'][i] <= got['pi'][i] <= got['pi_hi'][i] <= 1.0, i
        if e['status'] & (F.AT_ZERO | F.AT_ONE):
            assert got['iters'][i] == 0 and got['pi'][i] == e['pi'], i
        if not converged:
            continue
        g = e['gates']
        for f in ('pi', 'pi_lo', 'pi_hi'):
            _share(f, abs(got[f][i] - e[f]), g[f], worst)
        if np.isinf(e['stat']):
            assert got['stat'][i] == e['stat'], i
        else:
            _share('stat', abs(got['stat'][i] - e['stat']), g['stat'], worst)
        lo, hi = g['p_null']
        assert lo <= got['p_null'][i] <= hi, (i, lo, got['p_null'][i], hi)
        room = max(hi - e['p_null'], e['p_null'] - lo)
        if room > 0.0:
            worst['p_null'] = max(worst.get('p_null', 0.0), abs(got['p_null'][i] - e['p_null']) / room)
        if 'resp' in got:
            ok = ~np.isnan(e['resp'])
            d, gr = np.abs(got['resp'][sl][ok] - e['resp'][ok]), g['resp'][ok]
            assert (d[gr == 0.0] == 0.0).all(), (i, 'resp differs where its gate is 0')
            if (gr > 0.0).any():
                worst['resp'] = max(worst.get('resp', 0.0), float((d[gr > 0.0] / gr[gr > 0.0]).max()))
    for k, v in worst.items():
        _worst[k] = max(_worst.get(k, 0.0), v)
    fmt = lambda w: ', '.join('%s %.3g' % kv for kv in sorted(w.items())) or 'none compared'
    print('worst deviation as a share of its gate: %s (over the session: %s)' % (fmt(worst), fmt(_worst)))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_parity_over_the_row_lengths():
    """two rows of each length: 0, 1, 2, 15, 16, 17 (a lane's register chain), 255, 256, 257 (16 lanes / a wave), 1 023, 1 024, 1 025 (a
    wave / a workgroup), and the LDS-staged limit of the workgroup form and one score past it"""
    score, off = F.parity_batch()
    assert sorted(set(np.diff(off).tolist())) == sorted(F.PARITY_LENGTHS) and F.STAGE + 1 in np.diff(off)
    exp = F.expected('parity')
    got = site_stoich_host(score, off, resp=True)
    _check_rows(got, exp, off)
    assert sum(e['gates'] is not None and not e['status'] for e in exp) >= 16          # most rows have an interior estimate
    # min_valid = 1: the rows of one and two scores get their estimate, at an end or not
    exp1 = F.expected('parity', min_valid=1)
    got1 = site_stoich_host(score, off, min_valid=1, resp=True)
    _check_rows(got1, exp1, off)
    assert [e['status'] for e in exp1[:2]] == [F.TOO_FEW] * 2 and all(e['gates'] is not None for e in exp1[2:])


@pytest.mark.parametrize('min_valid', [1, 3, 6])
def test_content(min_valid):
    """separations of 0.3, 1, 3 and 8 sd at shares 0, 0.02, 0.5, 0.98 and 1 in all three forms; scaled sums; rows holding +-800, +-1e300,
    +-0.0, NaN and +-inf; rows of invalid scores only; flat rows; min_valid below and above the rows' counts"""
    score, off = F.content_batch()
    exp = F.expected('content', min_valid=min_valid)
    got = site_stoich_host(score, off, min_valid=min_valid, resp=True)
    _check_rows(got, exp, off)
    st = np.array([e['status'] for e in exp])
    assert ((st == F.FLAT).any() or min_valid > 4) and (st == F.TOO_FEW).any() and (st == F.AT_ZERO).any() and (st == F.AT_ONE).any() and (st == 0).sum() >= 20
    assert any(np.isinf(e['stat']) for e in exp) or min_valid > 4
    if min_valid == 6:
        assert (st == F.TOO_FEW).sum() > sum(e['status'] == F.TOO_FEW for e in F.expected('content', min_valid=3))


def test_max_iter_one_and_tol_zero():
    score, off = F.content_batch()
    # one evaluation per root: every root that is searched for stops unconverged, and says so
    exp = F.expected('content', max_iter=1)
    got = site_stoich_host(score, off, max_iter=1, resp=True)
    _check_rows(got, exp, off, converged=False)
    searched = [i for i, e in enumerate(exp) if e['gates'] is not None and e['status'] & F.NOT_CONVERGED]
    assert len(searched) >= 30 and all(got['iters'][i] == (0 if exp[i]['status'] & (F.AT_ZERO | F.AT_ONE) else 1) for i in searched)
    # tol == 0 runs max_iter evaluations; the roots sit where a step falls below the spacing of doubles: inside the gates at tol = 0
    exp = F.expected('content', tol=0.0, max_iter=40)
    got = site_stoich_host(score, off, tol=0.0, max_iter=40, resp=True)
    _check_rows(got, exp, off)
    interior = [i for i, e in enumerate(exp) if e['gates'] is not None and not e['status'] & (F.AT_ZERO | F.AT_ONE)]
    assert len(interior) >= 20 and all(got['iters'][i] == 40 and got['status'][i] & F.NOT_CONVERGED for i in interior)


def _raw(score, off, stride, fields, memspace=L.MEM_HOST, **opts):
    """nmod_site_stoich through ctypes with the outputs named in `fields` alone; host arrays in and out (device memory by torch)"""
    lib = L.load()
    o = dict(F.DEFAULTS, **opts)
    npos = len(off) - 1 if off is not None else len(score) // stride
    shapes = _engine()._stoich_shapes(npos, len(score))
    res = {f: np.full(shapes[f][1], 0, np.dtype(shapes[f][0])) for f in fields}
    if memspace == L.MEM_HOST:
        out = L.make_stoich_out(**{f: a.ctypes.data for f, a in res.items()})
        prm = L.make_params(memspace=L.MEM_HOST, dtype=L.DTYPE_F64, stride0=stride if off is None else 0)
        rc = lib.nmod_site_stoich(C.byref(prm), npos, score.ctypes.data, off.ctypes.data if off is not None else None,
                                  C.byref(L.make_stoich_opts(o['max_iter'], o['min_valid'], o['tol'], o['ci_drop'])), C.byref(out))
        assert rc == 0
        return res
    import torch
    d_score = torch.from_numpy(score).cuda()
    d_off = torch.from_numpy(off).cuda() if off is not None else None
    d_res = {f: torch.from_numpy(a).cuda() for f, a in res.items()}
    out = L.make_stoich_out(**{f: t.data_ptr() for f, t in d_res.items()})
    prm = L.make_params(memspace=L.MEM_DEVICE, dtype=L.DTYPE_F64, stride0=stride if off is None else 0, stream=torch.cuda.current_stream().cuda_stream)
    rc = lib.nmod_site_stoich(C.byref(prm), npos, d_score.data_ptr(), d_off.data_ptr() if d_off is not None else None,
                              C.byref(L.make_stoich_opts(o['max_iter'], o['min_valid'], o['tol'], o['ci_drop'])), C.byref(out))
    assert rc == 0
    torch.cuda.synchronize()
    return {f: t.cpu().numpy() for f, t in d_res.items()}


ALL = F.FIELDS + INT_FIELDS + ('resp',)


def test_a_rows_bits_depend_on_the_row_alone():
    """the same row alone, in a shuffled batch, in CSR and in stride form, from host and from device memory, with and without resp and
    with single outputs requested: the same bits"""
    score, off = F.content_batch()
    rows = [score[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    full = _raw(score, off, 0, ALL)
    per_row = lambda res, i, o: {f: (res[f][o[i]:o[i + 1]] if f == 'resp' else res[f][i:i + 1]) for f in res}
    same = lambda a, b: all(_bits(a[f]) == _bits(b[f]) for f in a)
    # shuffled
    perm = np.random.default_rng(1406).permutation(len(rows))
    sc2, off2 = F._csr([rows[j] for j in perm])
    shuf = _raw(sc2, off2, 0, ALL)
    assert all(same(per_row(shuf, k, off2), per_row(full, int(j), off)) for k, j in enumerate(perm))
    # alone: one row of each form and kind
    lens = np.diff(off)
    picks = [int(np.flatnonzero(lens == n)[k]) for n in (60, 300, 1500) for k in (1, 2, 4)] + list(range(len(rows) - 16, len(rows)))
    for i in picks:
        alone = _raw(np.ascontiguousarray(rows[i]), np.array([0, len(rows[i])], np.int64), 0, ALL)
        assert same(per_row(alone, 0, np.array([0, len(rows[i])])), per_row(full, i, off)), i
    # stride form: the rows of one length as a fixed-stride batch
    for n in (60, 300, 1500):
        idx = np.flatnonzero(lens == n)
        st = _raw(np.concatenate([rows[i] for i in idx]), None, n, ALL)
        so = np.arange(len(idx) + 1) * n
        assert all(same(per_row(st, k, so), per_row(full, int(i), off)) for k, i in enumerate(idx)), n
    # device memory
    dev = _raw(score, off, 0, ALL, memspace=L.MEM_DEVICE)
    assert same(dev, full)
    # fewer outputs
    for fields in (tuple(f for f in ALL if f != 'resp'), ('pi',), ('pi_lo', 'pi_hi'), ('p_null',), ('stat', 'status'), ('iters',), ('resp',), ('n_valid',)):
        part = _raw(score, off, 0, fields)
        assert all(_bits(part[f]) == _bits(full[f]) for f in fields), fields
    # and through the engine's two layers
    host = site_stoich_host(score, off, resp=True)
    assert all(_bits(host[f]) == _bits(full[f]) for f in ALL)
    import torch
    det = _engine().DeviceDetector(0)
    d = det.site_stoich(torch.from_numpy(score).cuda(), off=torch.from_numpy(off).cuda(), resp=True)
    assert all(_bits(d[f].cpu().numpy()) == _bits(full[f]) for f in ALL)


def test_a_batch_larger_than_the_grids():
    """more than twice as many rows of each class as the largest persistent grid has units — 16-lane groups, waves, workgroups — built by
    repeating a pool of 16 rows per class: every repeat has the bits of its first copy, and the first copies match the restatement"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    units = (cus * 8 * 16, cus * 8 * 4, cus * 2)          # site_stoich.hip: cap = num_cus * 8 blocks of 256 threads; num_cus * 2 workgroups
    rng = np.random.default_rng(1407)
    pool = [[F.simulate_row(rng, n, F.SEPARATIONS[j % 4], (0.5, 0.05, 0.9, 0.0)[(j // 4) % 4]) for j in range(16)] for n in (20, F.SMALL + 1, F.WAVE + 1)]
    counts = [2 * u + 5 for u in units]
    order = np.concatenate([np.full(c, k) for k, c in enumerate(counts)])
    rng.shuffle(order)                                     # the classes interleaved
    seen = [0, 0, 0]
    which = np.empty(len(order), np.int64)
    for i, k in enumerate(order):
        which[i] = seen[k] % 16
        seen[k] += 1
    lens = np.array([len(pool[k][0]) for k in range(3)])[order]
    off = np.zeros(len(order) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    score = np.empty(int(off[-1]))
    flat = [np.stack(p) for p in pool]
    for k in range(3):
        m = np.flatnonzero(order == k)
        score[(off[m][:, None] + np.arange(lens[m[0]])[None, :]).ravel()] = flat[k][which[m]].ravel()
    got = site_stoich_host(score, off, resp=True)
    first = {}
    for i in range(len(order)):
        first.setdefault((int(order[i]), int(which[i])), i)
    assert len(first) == sum(min(c, 16) for c in counts)
    rep = np.array([first[(int(k), int(j))] for k, j in zip(order, which)])
    for f in F.FIELDS + INT_FIELDS:
        assert _bits(got[f]) == _bits(got[f][rep]), f
    for k in range(3):
        m = np.flatnonzero(order == k)
        r = got['resp'][(off[m][:, None] + np.arange(lens[m[0]])[None, :])]
        r0 = got['resp'][(off[rep[m]][:, None] + np.arange(lens[m[0]])[None, :])]
        assert _bits(r) == _bits(r0), k
    sample = sorted(first.values())
    exp = {i: F.row(score[off[i]:off[i + 1]]) for i in sample}
    _check_rows(got, exp, off, rows=sample)


def test_a_row_beyond_max_deep_is_too_large():
    """2^24 scores: one more than NMOD_MAX_DEEP.  The row gets NaN outputs, NaN resp and its status; its neighbours are computed"""
    n = 2 ** 24
    rng = np.random.default_rng(1408)
    a, b = F.simulate_row(rng, 50, 3.0, 0.5), F.simulate_row(rng, 1200, 1.0, 0.3)
    score = np.concatenate([a, np.tile(np.array([1.0, -1.0, 0.5, -2.0]), n // 4), b])
    off = np.array([0, 50, 50 + n, 50 + n + 1200], np.int64)
    got = site_stoich_host(score, off, resp=True)
    assert got['status'].tolist() == [0, F.TOO_LARGE, 0] and got['n_valid'].tolist() == [50, 0, 1200] and got['iters'][1] == 0
    assert all(np.isnan(got[f][1]) for f in F.FIELDS) and np.isnan(got['resp'][50:50 + n]).all()
    exp = {0: F.row(a), 2: F.row(b)}
    _check_rows(got, exp, off, rows=[0, 2])


# ----------------------------------------------------------------------------------------------- the chain
def _chain():
    """about 60 reads over one short reference, the modified table 2 sd higher at the k-mers that cover one planted base, half of the
    reads of each strand modified there: one site at a share of 0.5 among canonical sites"""
    return RF.chain_inputs(n_reads=60, shift_sd=2.0)


def test_chain_finds_the_planted_site_and_leaves_the_rest_alone():
    reads, model, alt, planted = _chain()
    lines, lines0 = [], []
    table0, sites0 = RL.call_reads_llr(reads, model, alt, log=lines0.append)
    table, sites = RL.call_reads_llr(reads, model, alt, stoich={}, log=lines.append)
    assert set(sites) == set(sites0) | {'pi', 'pi_lo', 'pi_hi', 'stat', 'p_null', 'iters', 'stoich_status'}
    assert all(_bits(sites[f]) == _bits(sites0[f]) for f in sites0) and all(_bits(table[f]) == _bits(table0[f]) for f in table0)
    assert len(lines) == len(lines0) == 1 and lines[0].startswith(lines0[0] + '; ') and 'modified share' in lines[0] and 'modified share' not in lines0[0]
    # the device chain against the restatement over the same pivoted rows
    piv = _engine().pivot_reads(reads, 0, val=_window_sums(reads, model, alt))
    score, off = piv['sig'].cpu().numpy(), piv['off'].cpu().numpy()
    exp = F.site_stoich(score, off)
    got = dict({f: sites[f] for f in F.FIELDS}, n_valid=sites['n_valid'], iters=sites['iters'], status=sites['stoich_status'])
    _check_rows(got, exp, off)
    # the planted site: an interval above 0 on either strand, and the smallest p_null of its strand but for the bases within k - 1, whose
    # window sums share its events
    k = model['k']
    for strand in '+-':
        m = np.flatnonzero((sites['strand'] == strand) & ((sites['stoich_status'] & L.STOICH_NO_ESTIMATE) == 0))
        at = m[sites['pos'][m] == planted]
        assert len(at) == 1 and sites['pi_lo'][at[0]] > 0.0 and 0.2 < sites['pi'][at[0]] < 0.8 and sites['n_valid'][at[0]] >= 20
        far = m[np.abs(sites['pos'][m] - planted) >= k]
        assert sites['p_null'][at[0]] < sites['p_null'][far].min()
        assert abs(int(sites['pos'][m][np.argmin(sites['p_null'][m])]) - planted) < k
        assert (sites['pi_lo'][far] > 0.0).mean() < 0.1                        # canonical sites: the 95 % interval reaches 0 almost always


def _window_sums(reads, model, alt):
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    det = _engine().DeviceDetector(0)
    base = np.ascontiguousarray(np.asarray(reads['base']).astype('S1')).view(np.uint8)
    calls = det.read_llr(t(reads['norm_mean']), t(np.asarray(reads['off'], np.int64)), t(base), t(model['mean']), t(model['sd']), t(alt['mean']),
                         t(alt['sd']), model['k'], model['center'], want=('llr_win',))
    return calls['llr_win']


def test_end_to_end_through_the_command_line(capsys):
    """readllr --siteFraction 1 writes <FileID>_site_stoich.txt in the documented format; without the option the two files and the
    printed lines are those of a run with it, less the third file and the one clause"""
    from nanomod_amd import cli, container, kmermodel
    reads, model, alt, planted = _chain()
    with tempfile.TemporaryDirectory() as tmp:
        r_path, m_path, a_path = (os.path.join(tmp, n) for n in ('reads.npz', 'model.npz', 'alt.npz'))
        container.save_reads(r_path, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
        zeros = np.zeros(64, np.int64)
        for path, m in ((m_path, model), (a_path, alt)):
            kmermodel.save_kmer_model(path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                                 n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
        argv = ['readllr', '--wrkBase1', r_path, '--kmerModel', m_path, '--altModel', a_path, '--FileID', 'run']
        outs, printed = [os.path.join(tmp, n) for n in ('plain', 'zero', 'on')], []
        capsys.readouterr()
        for out, extra in zip(outs, ([], ['--siteFraction', '0'], ['--siteFraction', '1', '--minValid', '5', '--ciLevel', '0.9'])):
            assert cli.main(argv + ['--outFolder', out] + extra) == 0
            printed.append(capsys.readouterr().out.replace(out, 'OUT'))
        assert sorted(os.listdir(outs[0])) == sorted(os.listdir(outs[1])) == ['run_read_llr.txt', 'run_site_llr.txt']
        assert sorted(os.listdir(outs[2])) == ['run_read_llr.txt', 'run_site_llr.txt', 'run_site_stoich.txt']
        for f in ('run_read_llr.txt', 'run_site_llr.txt'):
            assert open(os.path.join(outs[0], f)).read() == open(os.path.join(outs[1], f)).read() == open(os.path.join(outs[2], f)).read()
        assert printed[0] == printed[1] and 'modified share' not in printed[0]
        with_clause = [ln for ln in printed[2].splitlines() if 'modified share' in ln]
        assert len(with_clause) == 1 and printed[2].replace(with_clause[0][with_clause[0].index('; ', with_clause[0].index('modified call')):], '') == printed[0]
        _, want = RL.call_reads_llr(reads, kmermodel.load_kmer_model(m_path), kmermodel.load_kmer_model(a_path),
                                    stoich=dict(min_valid=5, ci_level=0.9), log=lambda *a: None)
        u = [ln.split() for ln in open(os.path.join(outs[2], 'run_site_stoich.txt')).read().splitlines()]
        assert len(u) == len(want['pos']) and all(len(r) == 12 for r in u)
        assert [r[0] for r in u] == want['chrom'].tolist() and [r[1] for r in u] == want['strand'].tolist() and {r[3] for r in u} <= set('ACGT')
        for col, f in ((2, want['pos'] + 1), (4, want['n_reads']), (5, want['n_valid']), (11, want['stoich_status'])):
            assert [int(r[col]) for r in u] == np.asarray(f).tolist(), col
        for col, f, fmt in ((6, 'pi', '%.6f'), (7, 'pi_lo', '%.6f'), (8, 'pi_hi', '%.6f'), (9, 'stat', '%.3f')):
            assert [r[col] for r in u] == [fmt % v for v in want[f]], f
        assert [r[10] for r in u] == ['%.3E' % v if v == v else 'nan' for v in want['p_null']]
        assert any(r[6] == 'nan' for r in u) and any(r[6] != 'nan' for r in u) and (want['n_valid'][want['stoich_status'] == F.TOO_FEW] < 5).all()


def test_p_null_goes_straight_into_the_device_fdr():
    import torch
    reads, model, alt, planted = _chain()
    det = _engine().DeviceDetector(0)
    piv = _engine().pivot_reads(reads, 0, val=_window_sums(reads, model, alt))
    st = det.site_stoich(piv['sig'], off=piv['off'])
    (q,), summary = det.fdr(st, tracks=('p_null',), method='bh', alpha=0.05)
    torch.cuda.synchronize()
    p, q = st['p_null'].cpu().numpy(), q.cpu().numpy()
    (want,), (summ,) = _engine().fdr_adjust_host([p])
    assert _bits(q) == _bits(want) and _engine().fdr_summary_dicts(summary)[0] == summ
    assert summ['tested'] == int((~np.isnan(p)).sum()) and summ['excluded'] == int(np.isnan(p).sum()) and summ['rejected'] >= 2
    pos = piv['key'].cpu().numpy() & ((1 << 40) - 1)
    assert planted in pos[np.flatnonzero(q <= 0.05)].tolist()
