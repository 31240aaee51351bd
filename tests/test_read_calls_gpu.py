"""nmod_read_calls / nmod_site_calls (K12) on the GPU against the numpy restatement of their definition (tests/readcalls_ref.py, pinned
against mpmath in tests/test_read_calls.py): parity over every length at which the code takes another path, the deep tails, ineligible
events, reads as walls, the independence of a read's bits from the batch, the per-position counts, and the chain through the Python
layers and the command line."""
import os
import tempfile

import numpy as np
import pytest

import readcalls_ref as Q
import rescale_ref as R
from nanomod_amd import readcalls as RC           # K12's module: without it nothing here can pass

pytestmark = pytest.mark.gpu

P_GATE = 1e-9                                     # the library's p-value gate, relative
EVENT_FIELDS = ('z', 'p', 'p_win')
READ_FIELDS = ('n_sites', 'n_called', 'status')


def _engine():
    from nanomod_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _model(p, k, center):
    return dict(k=k, center=center, mean=p['mean'], sd=p['sd'])


def _check_p(got, exp, name):
    """within 1e-9 relative where the restatement is above DBL_MIN, exactly DBL_MIN where it clamps, the NaN pattern identical"""
    nan = np.isnan(exp)
    assert np.array_equal(np.isnan(got), nan), '%s: NaN pattern differs' % name
    clamped = exp == Q.DBL_MIN
    assert (got[clamped] == Q.DBL_MIN).all(), '%s: %d clamped value(s) differ' % (name, int((got[clamped] != Q.DBL_MIN).sum()))
    m = ~nan & ~clamped
    err = np.abs(got[m] / exp[m] - 1.0)
    print('%s: worst relative deviation %.3g over %d value(s)' % (name, err.max() if m.any() else 0.0, int(m.sum())))
    assert (err <= P_GATE).all(), '%s: worst relative deviation %g' % (name, err.max())


def _check_against(got, exp):
    nan = np.isnan(exp['z'])
    assert np.array_equal(np.isnan(got['z']), nan) and _bits(got['z'][~nan]) == _bits(exp['z'][~nan]), 'z is not bit-equal to (x - mu) / sd'
    _check_p(got['p'], exp['p'], 'p')
    _check_p(got['p_win'], exp['p_win'], 'p_win')
    assert exp['alpha_margin'] > P_GATE                          # no restated P within the gate of alpha: the counts are exact
    for f in READ_FIELDS:
        assert np.array_equal(got[f], exp[f]), (f, got[f], exp[f])


@pytest.mark.parametrize('k,center,nb,dtype', Q.PARITY_CASES)
def test_parity_with_the_restatement(k, center, nb, dtype):
    p = Q.parity_inputs(k, center, nb, dtype)
    exp = Q.parity_expected(k, center, nb, dtype)
    got = _engine().read_calls_host(p['val'], p['off'], p['base'], _model(p, k, center), nb=nb, alpha=Q.PARITY_ALPHA)
    _check_against(got, exp)
    if nb == 0:
        assert _bits(got['p_win']) == _bits(got['p'])            # the same bits


@pytest.mark.parametrize('nb', [2, 64])
def test_deep_tails(nb):
    """runs of |z| in {0, 5, 20, 37, 39, 60} and lone events of 38 and 39 inside the zeros: p clamps at DBL_MIN from |z| = 37.52 on, and
    the windows around a lone clamped event are still right, because the unclamped l feeds them — against mpmath itself there"""
    d = Q.deep_tail_read()
    exp = Q.read_calls(d['val'], d['off'], d['base'], 1, 0, d['mean'], d['sd'], nb, 0.01)
    got = _engine().read_calls_host(d['val'], d['off'], d['base'], dict(k=1, center=0, mean=d['mean'], sd=d['sd']), nb=nb, alpha=0.01)
    _check_against(got, exp)
    az = np.abs(d['val'])
    assert _bits(got['z']) == _bits(d['val'])
    assert (got['p'][az >= 38.0] == Q.DBL_MIN).all() and (got['p'][az <= 37.0] > Q.DBL_MIN).all() and (az >= 38.0).sum() == 2 * Q.DEEP_RUN + 2
    inside = np.arange(len(az)) >= 3 * Q.DEEP_RUN + 3 * Q.DEEP_RUN + nb     # well inside the runs of 39 and 60: every window clamps
    assert (got['p_win'][inside & (np.arange(len(az)) < len(az) - nb)] == Q.DBL_MIN).all()
    import mpmath as mp
    seen = 0
    for j, z in Q.DEEP_SINGLES:
        for jj in (j - nb, j - 1, j, j + 1, j + nb):                         # windows that hold the lone event: all zeros but it
            want = Q.mp_window([0.0] * (2 * nb) + [z])
            if want >= Q.DBL_MIN:
                assert abs(got['p_win'][jj] / float(want) - 1.0) <= P_GATE, (nb, j, jj, got['p_win'][jj], float(want))
                # what a clamped tail would have given is far outside the gate: the check sees the difference
                wrong = mp.gammainc(2 * nb + 1, -mp.log(mp.mpf(Q.DBL_MIN)), mp.inf, regularized=True)
                assert abs(float(wrong / want) - 1.0) > 1e-3
                seen += 1
            else:
                assert got['p_win'][jj] == Q.DBL_MIN
    assert seen == (5 if nb == 2 else 10)
    assert got['n_sites'].tolist() == [len(az)] and got['n_called'].tolist() == exp['n_called'].tolist()


@pytest.mark.parametrize('dtype', ['float32', 'float64', 'int16'])
def test_ineligible_events(dtype):
    """'N' and lower-case bytes, model holes (NaN level, NaN / zero / negative spread), NaN and infinite values, a read shorter than k,
    and a read of ineligible events only: NaN outputs exactly there, and the windows of the neighbours shrink accordingly"""
    k, center, nb = 3, 1, 2
    rng = np.random.default_rng(5)
    mean, sd = R.make_model(k)                                               # holes at codes 3, 6, 9, 12
    b1, x1 = R.draw_read(rng, 400, k, center, mean, sd, 0.0, 1.0)
    b1[[10, 11, 150, 151, 153, 399]] = [ord(c) for c in 'NacgtN']
    b2 = np.tile(np.frombuffer(b'AATACGGCGTAACC', np.uint8), 30)             # runs through the holes of the model
    x2 = R.draw_values(rng, b2, k, center, mean, sd, 0.0, 1.0)
    b3, x3 = R.draw_read(rng, 300, k, center, mean, sd, 0.0, 1.0)
    if dtype != 'int16':
        x3[[0, 3, 50, 51, 200, 299]] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    b4, x4 = R.draw_read(rng, 2, k, center, mean, sd, 0.0, 1.0)              # shorter than k
    b5, x5 = np.full(100, ord('n'), np.uint8), np.zeros(100)                 # nothing eligible
    b6, x6 = R.draw_read(rng, 70, k, center, mean, sd, 0.0, 1.0)
    reads = [(b1, x1), (b2, x2), (b3, x3), (b4, x4), (b5, x5), (b6, x6)]
    off = np.zeros(len(reads) + 1, np.int64)
    off[1:] = np.cumsum([len(r[1]) for r in reads])
    val, base = R.cast(np.concatenate([r[1] for r in reads]), dtype), np.concatenate([r[0] for r in reads])
    exp = Q.read_calls(val, off, base, k, center, mean, sd, nb, 0.01)
    got = _engine().read_calls_host(val, off, base, dict(k=k, center=center, mean=mean, sd=sd), nb=nb, alpha=0.01)
    _check_against(got, exp)
    # the restatement's own pattern is the one the definition gives
    codes = np.concatenate([R.read_codes(r[0], k, center) for r in reads])
    bad = (codes < 0) | np.isin(codes, (3, 6, 9, 12)) | ~np.isfinite(R.to_double(val))
    assert np.array_equal(np.isnan(exp['p_win']), bad) and bad[off[0] + 9:off[0] + 13].all() and bad[off[1]:off[2]].sum() > 80
    assert all(np.array_equal(np.isnan(got[f]), bad) for f in EVENT_FIELDS)
    assert got['n_sites'].tolist() == [int((~bad[off[i]:off[i + 1]]).sum()) for i in range(len(reads))]
    assert got['n_sites'][3] == got['n_sites'][4] == 0 and got['n_called'][3] == got['n_called'][4] == 0 and not got['status'].any()
    W = exp['W'][~bad]
    assert W.min() >= 1 and W.max() == 5 and (W < 5).sum() > 100             # shrunk windows: checked through p_win above


def test_reads_are_walls():
    """two adjacent reads: changing every value of the second leaves every bit of the first unchanged, its last nb events included"""
    k, center = 3, 1
    rng = np.random.default_rng(6)
    mean, sd = R.make_model(k, holes=False)
    for nb, n1 in ((2, 300), (64, 300), (64, 3000)):
        b1, x1 = R.draw_read(rng, n1, k, center, mean, sd, 0.0, 1.0, contaminate=False)
        b2, x2 = R.draw_read(rng, 500, k, center, mean, sd, 0.0, 1.0, contaminate=False)
        off = np.array([0, n1, n1 + 500], np.int64)
        base = np.concatenate([b1, b2])
        model = dict(k=k, center=center, mean=mean, sd=sd)
        a = _engine().read_calls_host(np.concatenate([x1, x2]), off, base, model, nb=nb)
        b = _engine().read_calls_host(np.concatenate([x1, x2 + 7.0]), off, base, model, nb=nb)
        exp = Q.read_calls(np.concatenate([x1, x2]), off, base, k, center, mean, sd, nb, 0.01)
        for f in EVENT_FIELDS:
            assert _bits(a[f][:n1]) == _bits(b[f][:n1]) and _bits(a[f][n1:]) != _bits(b[f][n1:]), (nb, f)
        assert all(a[f][0] == b[f][0] for f in READ_FIELDS) and a['n_called'][1] != b['n_called'][1]
        _check_p(a['p_win'][n1 - nb:n1 + nb], exp['p_win'][n1 - nb:n1 + nb], 'p_win at the wall')
        # (k = 3: the first and the last event of a read have no k-mer) the last scored event of a read sees nothing of the next read
        assert exp['W'][n1 - 2] == nb + 1 == exp['W'][n1 + 1] and exp['W'][n1 - 1] == 0 == exp['W'][n1]


def _permuted(p, order):
    lens = np.diff(p['off'])[order]
    off = np.zeros(len(order) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    ev = np.concatenate([np.arange(p['off'][i], p['off'][i + 1]) for i in order]) if len(order) else np.zeros(0, np.int64)
    return ev, off


@pytest.mark.parametrize('dtype,k,center,nb', [('int16', 5, 2, 2), ('float64', 6, 2, 64), ('float32', 1, 0, 0)])
def test_bits_do_not_depend_on_order_batch_memspace_or_requested_outputs(dtype, k, center, nb):
    import torch
    from nanomod_amd import DeviceDetector
    p = Q.parity_inputs(k, center, nb, dtype)
    model = _model(p, k, center)
    first = _engine().read_calls_host(p['val'], p['off'], p['base'], model, nb=nb)
    nreads = len(p['off']) - 1
    for order in (np.random.default_rng(9).permutation(nreads), np.array([15, 5]), np.array([14]), np.array([10])):   # a batch of one, both classes
        ev, off = _permuted(p, order)
        again = _engine().read_calls_host(p['val'][ev], off, p['base'][ev], model, nb=nb)
        assert all(_bits(again[f]) == _bits(first[f][order]) for f in READ_FIELDS)
        assert all(_bits(again[f]) == _bits(first[f][ev]) for f in EVENT_FIELDS)
    only = _engine().read_calls_host(p['val'], p['off'], p['base'], model, nb=nb, want=('p_win',))
    assert set(only) == {'p_win'} | set(READ_FIELDS) and all(_bits(only[f]) == _bits(first[f]) for f in only)
    det = DeviceDetector(0)
    t = lambda x: torch.from_numpy(np.array(x)).cuda()
    args = (t(p['val']), t(p['off']), t(R.as_bytes(p['base'])), t(p['mean']), t(p['sd']), k, center)
    out = det.read_calls(*args, nb=nb)
    assert all(_bits(out[f].cpu().numpy()) == _bits(first[f]) for f in EVENT_FIELDS + READ_FIELDS)
    with torch.cuda.stream(torch.cuda.Stream()):
        side = det.read_calls(*args, nb=nb, want=('p_win',))
        torch.cuda.current_stream().synchronize()
    assert set(side) == {'p_win'} | set(READ_FIELDS) and all(_bits(side[f].cpu().numpy()) == _bits(first[f]) for f in side)
    again = det.read_calls(*args, nb=nb, out=out)
    assert again is out
    for kw in (dict(nb=65), dict(alpha=0.0), dict(want=('x',)), dict(out=dict(out, status=out['status'][:3]))):
        with pytest.raises(ValueError):
            det.read_calls(*args, **kw)
    with pytest.raises(ValueError):
        det.read_calls(args[0], args[1], args[2][:-1], *args[3:])


def test_site_calls():
    """rows of lengths {0, 1, 63, 64, 65, 1 000, 70 000} with NaN, values outside [0, 1] and values exactly alpha: the counts equal
    numpy's, frac is bit-equal, the NaN frac sits on the empty and the all-invalid rows, CSR equals the stride form"""
    import torch
    from nanomod_amd import DeviceDetector
    alpha = 0.01
    rng = np.random.default_rng(12)
    lens = [0, 1, 63, 64, 65, 1000, 70000, 64, 5, 1, 0]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    s = np.where(rng.random(off[-1]) < 0.3, rng.uniform(0.0, 0.02, off[-1]), rng.random(off[-1]))
    u = rng.random(off[-1])
    s[u < 0.1] = np.nan
    s[(u >= 0.1) & (u < 0.15)] = alpha                                       # exactly alpha: called
    s[(u >= 0.15) & (u < 0.2)] = rng.choice([-0.5, 1.5, np.inf, -np.inf, -1e-300, 1.0 + 2.0 ** -52], int(((u >= 0.15) & (u < 0.2)).sum()))
    s[(u >= 0.2) & (u < 0.22)] = rng.choice([0.0, 1.0, np.nextafter(alpha, 1.0), np.nextafter(alpha, 0.0)], int(((u >= 0.2) & (u < 0.22)).sum()))
    s[off[7]:off[8]] = np.nan                                                # all invalid
    s[off[8]:off[9]] = [2.0, -1.0, np.nan, np.inf, 1.5]
    s[off[9]] = alpha
    exp = Q.site_calls(s, off, alpha)
    assert np.isnan(exp['frac'][[0, 7, 8, 10]]).all() and exp['frac'][9] == 1.0 and exp['n_valid'][6] > 50000 and (s == alpha).sum() > 3000
    got = _engine().site_calls_host(s, off, alpha=alpha)
    for f in ('n_valid', 'n_called'):
        assert got[f].dtype == np.int32 and np.array_equal(got[f], exp[f]), f
    assert _bits(got['frac']) == _bits(exp['frac'])
    det = DeviceDetector(0)
    dev = det.site_calls(torch.from_numpy(s).cuda(), off=torch.from_numpy(off).cuda(), alpha=alpha)
    assert all(_bits(dev[f].cpu().numpy()) == _bits(got[f]) for f in got)
    for stride in (3, 64, 65, 1000):                                          # the stride form over the same values, whole rows
        n = (len(s) // stride) * stride
        soff = np.arange(0, n + 1, stride, dtype=np.int64)
        a = _engine().site_calls_host(s[:n], None, stride=stride, alpha=alpha)
        b = _engine().site_calls_host(s[:n], soff, alpha=alpha)
        e = Q.site_calls(s[:n], soff, alpha)
        assert all(_bits(a[f]) == _bits(b[f]) == _bits(e[f].astype(a[f].dtype)) for f in a), stride
        d = det.site_calls(torch.from_numpy(s[:n]).cuda(), stride=stride, alpha=alpha)
        assert all(_bits(d[f].cpu().numpy()) == _bits(a[f]) for f in a)
    other = _engine().site_calls_host(s, off, alpha=0.5)
    assert np.array_equal(other['n_valid'], exp['n_valid']) and np.array_equal(other['n_called'], Q.site_calls(s, off, 0.5)['n_called'])
    for kw in (dict(alpha=2.0), dict(stride=0), dict(off=torch.from_numpy(off))):
        with pytest.raises(ValueError):
            det.site_calls(torch.from_numpy(s).cuda(), **kw)


def _expected_chain(reads, model, nb, alpha):
    exp = Q.read_calls(reads['norm_mean'], reads['off'], reads['base'], model['k'], model['center'], model['mean'], model['sd'], nb, alpha)
    assert exp['alpha_margin'] > P_GATE
    rows = Q.pivot(reads, exp['p_win'])
    return exp, rows, Q.site_calls(rows['val'], rows['off'], alpha)


def _check_chain(table, sites, reads, exp, rows, s):
    for f in READ_FIELDS:
        assert np.array_equal(table[f], exp[f]), f
    assert np.array_equal(table['events'], np.diff(reads['off'])) and np.array_equal(table['start'], reads['start'])
    assert table['chrom'].tolist() == reads['chrom'].tolist() and table['strand'].tolist() == reads['strand'].tolist()
    for f in ('chrom', 'strand', 'pos'):
        assert np.array_equal(np.asarray(sites[f]).astype(rows[f].dtype), rows[f]), f
    assert np.array_equal(sites['n_reads'], np.diff(rows['off']))
    assert np.array_equal(sites['n_valid'], s['n_valid']) and np.array_equal(sites['n_called'], s['n_called'])
    assert _bits(sites['frac']) == _bits(s['frac'])


@pytest.mark.parametrize('nb', Q.CHAIN_NB)
def test_chain_equals_the_restatement(nb):
    """call_reads — calls, pivot and counts on the device — against the restatement chained through a numpy pivot: exact integers.  (That
    the planted position stands out in the restatement is tests/test_read_calls.py's.)"""
    reads, model, planted = Q.chain_inputs()
    exp, rows, s = _expected_chain(reads, model, nb, 0.01)
    lines = []
    table, sites, ev = RC.call_reads(reads, model, nb=nb, alpha=0.01, events=True, log=lines.append)
    _check_chain(table, sites, reads, exp, rows, s)
    _check_p(ev['p_win'], exp['p_win'], 'p_win')
    assert _bits(ev['z']) == _bits(exp['z'])
    assert len(lines) == 1 and lines[0].startswith('readcalls: 200 read(s), %d of %d event(s) scored, %d called' % (
        exp['n_sites'].sum(), len(reads['norm_mean']), exp['n_called'].sum()))
    table2, sites2 = RC.call_reads(reads, model, nb=nb, alpha=0.01, log=lambda *a: None)
    assert all(_bits(table2[f]) == _bits(table[f]) for f in READ_FIELDS) and all(_bits(sites2[f]) == _bits(sites[f]) for f in sites)
    for strand in '+-':                                                      # the device chain finds the planted position too
        m = sites['strand'] == strand
        assert abs(sites['pos'][m][np.argmax(sites['n_called'][m])] - planted) <= nb
    thin = dict(model, n_positions=np.where(np.arange(64) % 2, 5, 1))       # min_positions masks half of the model
    t3, s3 = RC.call_reads(reads, thin, nb=nb, min_positions=2, log=lambda *a: None)
    e3, r3, c3 = _expected_chain(reads, dict(model, mean=np.where(np.arange(64) % 2, model['mean'], np.nan)), nb, 0.01)
    _check_chain(t3, s3, reads, e3, r3, c3)
    assert 0 < t3['n_sites'].sum() < table['n_sites'].sum()


def test_chain_with_rescale_equals_rescaling_first():
    """rescale=dict(...): K11 on the device feeding its tensor straight in, bit for bit what rescale.rescale_reads and a plain call give"""
    from nanomod_amd import rescale
    k, center = 3, 1
    mean, sd = R.make_model(k, holes=False)
    reads = R.make_read_set(4243, k, center, mean, sd, reads_per_strand=10, planted=True, contaminate=True)
    model = dict(k=k, center=center, mean=mean, sd=sd, n_positions=np.ones(64, np.int64))
    opts = dict(min_events=60, clip_sigma=2.5)
    first, fit = rescale.rescale_reads(reads, model, log=lambda *a: None, **opts)
    assert (fit['status'] == 0).all() and np.abs(fit['scale'] - 1.0).max() > 0.1
    want_t, want_s, want_e = RC.call_reads(first, model, events=True, log=lambda *a: None)
    got_t, got_s, got_e = RC.call_reads(reads, model, rescale=opts, events=True, log=lambda *a: None)
    assert all(_bits(got_e[f]) == _bits(want_e[f]) for f in EVENT_FIELDS)
    assert all(_bits(got_t[f]) == _bits(want_t[f]) for f in want_t) and all(_bits(got_s[f]) == _bits(want_s[f]) for f in want_s)
    assert _bits(got_t['shift']) == _bits(fit['shift']) and _bits(got_t['scale']) == _bits(fit['scale']) and not got_t['rescale_status'].any()
    plain = RC.call_reads(reads, model, events=True, log=lambda *a: None)[2]
    assert _bits(plain['z']) != _bits(got_e['z'])                            # the rescaling is not a no-op here


def test_end_to_end_through_the_command_line():
    from nanomod_amd import cli, container, kmermodel
    reads, model, planted = Q.chain_inputs()
    exp, rows, s = _expected_chain(reads, model, 2, 0.01)
    with tempfile.TemporaryDirectory() as tmp:
        r_path, m_path, g_path, e_path, out = (os.path.join(tmp, n) for n in ('reads.npz', 'model.npz', 'group.npz', 'events.npz', 'cli'))
        container.save_reads(r_path, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
        zeros = np.zeros(64, np.int64)
        kmermodel.save_kmer_model(m_path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=1, mean=model['mean'], sd=model['sd'], n_positions=model['n_positions'],
                                               n_samples=zeros + 10, n_clipped=zeros))
        assert cli.main(['readcalls', '--wrkBase1', r_path, '--kmerModel', m_path, '--outFolder', out, '--FileID', 'run', '--outLevel', '3',
                         '--outEvents', e_path]) == 0
        t = [ln.split() for ln in open(os.path.join(out, 'run_read_calls.txt')).read().splitlines()]
        assert len(t) == 200 and all(len(r) == 8 for r in t)
        assert [int(r[0]) for r in t] == list(range(200)) and [r[1] for r in t] == reads['chrom'].tolist() and [r[2] for r in t] == reads['strand'].tolist()
        for col, want in ((3, reads['start']), (4, np.diff(reads['off'])), (5, exp['n_sites']), (6, exp['n_called']), (7, exp['status'])):
            assert [int(r[col]) for r in t] == np.asarray(want).tolist(), col
        u = [ln.split() for ln in open(os.path.join(out, 'run_site_calls.txt')).read().splitlines()]
        assert len(u) == len(rows['pos']) and all(len(r) == 8 for r in u)
        assert [r[0] for r in u] == rows['chrom'].tolist() and [r[1] for r in u] == rows['strand'].tolist()
        for col, want in ((2, rows['pos'] + 1), (4, np.diff(rows['off'])), (5, s['n_valid']), (6, s['n_called'])):
            assert [int(r[col]) for r in u] == np.asarray(want).tolist(), col
        assert [r[7] for r in u] == ['%.6f' % v for v in s['frac']] and {r[3] for r in u} <= set('ACGT')
        ev = np.load(e_path)
        assert sorted(ev.files) == ['off', 'p', 'p_win', 'z'] and np.array_equal(ev['off'], reads['off']) and _bits(ev['z']) == _bits(exp['z'])
        _check_p(ev['p_win'], exp['p_win'], 'p_win')
        _check_p(ev['p'], exp['p'], 'p')
        # --rescale 1: the fit of `rescale` with its defaults, then the calls
        assert cli.main(['readcalls', '--wrkBase1', r_path, '--kmerModel', m_path, '--outFolder', out, '--FileID', 'rs', '--outLevel', '3',
                         '--rescale', '1', '--neighborPvalues', '0', '--callAlpha', '0.001']) == 0
        want_t, _ = RC.call_reads(reads, kmermodel.load_kmer_model(m_path), nb=0, alpha=0.001, rescale={}, log=lambda *a: None)
        t = [ln.split() for ln in open(os.path.join(out, 'rs_read_calls.txt')).read().splitlines()]
        assert [int(r[6]) for r in t] == want_t['n_called'].tolist() and sum(int(r[6]) for r in t) > 50
        # a per-position container is refused, with the message
        container.save_group(g_path, ['c'], ['+'], [0], ['A'], [0, 1], np.zeros(1, np.float32))
        assert cli.main(['readcalls', '--wrkBase1', g_path, '--kmerModel', m_path, '--outFolder', out]) == 1


def test_a_read_beyond_max_deep_is_too_large():
    """2^24 events: one more than NMOD_MAX_DEEP.  The read gets NaN events, zero counts and its status; its neighbour is called"""
    k, center = 3, 1
    mean, sd = R.make_model(k, holes=False)
    rng = np.random.default_rng(8)
    b0, x0 = R.draw_read(rng, 200, k, center, mean, sd, 0.0, 1.0)
    n = Q.MAX_DEEP + 1
    val = np.concatenate([(np.arange(n, dtype=np.int64) % 2001 - 1000).astype(np.int16), R.cast(x0, 'int16')])
    base = np.concatenate([np.tile(np.frombuffer(b'ACGTTGCA', np.uint8), n // 8), b0])
    off = np.array([0, n, n + 200], np.int64)
    got = _engine().read_calls_host(val, off, base, dict(k=k, center=center, mean=mean, sd=sd), want=('p_win',))
    exp = Q.read_calls(val[n:], np.array([0, 200], np.int64), b0, k, center, mean, sd, 2, 0.01)
    assert got['status'].tolist() == [Q.TOO_LARGE, 0] and got['n_sites'].tolist() == [0, exp['n_sites'][0]]
    assert got['n_called'].tolist() == [0, exp['n_called'][0]] and np.isnan(got['p_win'][:n]).all()
    _check_p(got['p_win'][n:], exp['p_win'], 'p_win')
