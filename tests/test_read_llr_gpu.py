"""nmod_read_llr / nmod_site_llr (K13) on the GPU against the numpy restatement of their definition (tests/readllr_ref.py, pinned against
mpmath in tests/test_read_llr.py): parity over every length, window and table size at which the code takes another path, bit-equality
where the spreads are equal, the orientation of the window, ineligible events, reads as walls, the independence of a read's bits from
the batch, the per-position counts, and the chain through the Python layers and the command line.  The gates are readllr_ref's."""
import os
import tempfile

import numpy as np
import pytest

import readllr_ref as F
import rescale_ref as R
from nanomod_amd import readllr as RL             # K13's module: without it nothing here can pass

pytestmark = pytest.mark.gpu

EVENT_FIELDS = ('llr', 'llr_win', 'p_mod')
READ_FIELDS = ('n_sites', 'n_mod', 'n_can', 'status')
_worst = dict(llr=0.0, llr_win=0.0, p_mod=0.0)    # the worst ratio of a deviation to its gate over the session, printed per test


def _engine():
    from nanomod_amd import engine
    return engine


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _models(p, k, center):
    return dict(k=k, center=center, mean=p['mean'], sd=p['sd']), dict(k=k, center=center, mean=p['alt_mean'], sd=p['alt_sd'])


def _ratio(name, dev, gate):
    """the worst deviation as a share of its gate; a deviation where the gate is 0 must be 0"""
    assert (dev[gate == 0.0] == 0.0).all(), '%s differs where its gate is 0' % name
    m = gate > 0.0
    r = float((dev[m] / gate[m]).max()) if m.any() else 0.0
    _worst[name] = max(_worst[name], r)
    return r


def _check_events(got, exp, sel=slice(None)):
    """llr within 2^-49 max(|g|, |d|, |llr|), llr_win within gate_L, p_mod within gate_L + 2^-49 relative (absolute DBL_MIN where the
    restated value is below DBL_MIN); the NaN pattern identical"""
    e = {f: exp[f][sel] for f in EVENT_FIELDS + ('gate_llr', 'gate_L')}
    got = {f: got[f][sel] for f in EVENT_FIELDS if f in got}
    nan = np.isnan(e['llr'])
    for f in EVENT_FIELDS:
        if f in got:
            assert np.array_equal(np.isnan(got[f]), nan), '%s: NaN pattern differs' % f
    ok = ~nan
    ratios = {}
    if 'llr' in got:
        ratios['llr'] = _ratio('llr', np.abs(got['llr'][ok] - e['llr'][ok]), e['gate_llr'][ok])
    if 'llr_win' in got:
        ratios['llr_win'] = _ratio('llr_win', np.abs(got['llr_win'][ok] - e['llr_win'][ok]), e['gate_L'][ok])
    if 'p_mod' in got:
        p, q = got['p_mod'][ok], e['p_mod'][ok]
        tiny = q < F.DBL_MIN
        assert (np.abs(p[tiny] - q[tiny]) <= F.DBL_MIN).all(), 'p_mod differs below DBL_MIN'
        ratios['p_mod'] = _ratio('p_mod', np.abs(p[~tiny] - q[~tiny]), (e['gate_L'][ok][~tiny] + F.GATE_P_EXTRA) * q[~tiny])
        assert ((p >= 0.0) & (p <= 1.0)).all()
    print('worst deviation as a share of its gate: %s (over the session: %s)'
          % (', '.join('%s %.3g' % kv for kv in ratios.items()), ', '.join('%s %.3g' % kv for kv in _worst.items())))
    assert all(r <= 1.0 for r in ratios.values()), ratios


def _check_against(got, exp):
    _check_events(got, exp)
    assert exp['thr_margin'] > 0.0                               # no restated sum within its gate of a threshold: the counts are exact
    for f in READ_FIELDS:
        assert np.array_equal(got[f], exp[f]), (f, got[f], exp[f])


def _run(p, k, center, window, **kw):
    m0, m1 = _models(p, k, center)
    return _engine().read_llr_host(p['val'], p['off'], p['base'], m0, m1, window=window, thr=kw.pop('thr', F.PARITY_THR),
                                   prior_logit=kw.pop('prior_logit', F.PARITY_PRIOR_LOGIT), **kw)


@pytest.mark.parametrize('k,center,window,dtype', F.PARITY_CASES)
def test_parity_with_the_restatement(k, center, window, dtype):
    p = F.parity_inputs(k, center, window, dtype)
    exp = F.parity_expected(k, center, window, dtype)
    got = _run(p, k, center, window)
    _check_against(got, exp)
    if F.window_of(window, k, center) == (0, 0):
        assert _bits(got['llr_win']) == _bits(got['llr'])        # the same bits


@pytest.mark.parametrize('k,center,window,dtype', F.PARITY_CASES)
def test_equal_spreads_are_bit_equal(k, center, window, dtype):
    """sd1 = sd0: g is an exact 0, every remaining operation is a correctly rounded one in a fixed order, so llr and the window sums are
    the restatement's bits"""
    p = F.parity_inputs(k, center, window, dtype, True)
    exp = F.parity_expected(k, center, window, dtype, True)
    got = _run(p, k, center, window)
    assert _bits(got['llr']) == _bits(exp['llr']) and _bits(got['llr_win']) == _bits(exp['llr_win'])
    _check_against(got, exp)


@pytest.mark.parametrize('n,i0', [(700, 2), (700, 380), (700, 383), (700, 385), (700, 390), (700, 447), (700, 449), (700, 490), (700, 496), (700, 500),
                                   (700, 505), (700, 511), (700, 512), (700, 520), (700, 697), (3000, 2), (3000, 495), (3000, 497), (3000, 1490),
                                   (3000, 2049), (3000, 2990)])
def test_window_orientation(n, i0):
    """one read over a 1-mer pair of equal spreads whose levels differ for base C alone: llr is an exact 0 but at the one event i0 that
    carries a C.  With window (2, 5) — two events back, five ahead — llr_win is nonzero exactly on j in [i0 - 5, i0 + 2]; i0 within 8 of
    the edges of the staged tile (512 events) and of the tile's own events (496 of them with a halo of one run a side, 448 with (0, 64),
    384 with (64, 64)), at both ends of the read, and in a read of 3 000 events, the workgroup form"""
    mean, sd = np.zeros(4), np.ones(4)
    alt_mean = np.array([0.0, 1.0, 0.0, 0.0])
    base = np.full(n, ord('A'), np.uint8)
    base[i0] = ord('C')
    val = np.full(n, 2.0)
    m0, m1 = dict(k=1, center=0, mean=mean, sd=sd), dict(k=1, center=0, mean=alt_mean, sd=sd)
    for window, lo, hi in (((2, 5), 2, 5), ((5, 2), 5, 2), ((0, 64), 0, 64), ((9, 0), 9, 0), ((64, 64), 64, 64)):
        got = _engine().read_llr_host(val, np.array([0, n], np.int64), base, m0, m1, window=window, thr=1.0)
        want = np.zeros(n)
        want[i0] = 1.5                                           # x - 1/2 for a gap of one spread
        assert _bits(got['llr']) == _bits(want)
        seen = np.flatnonzero(got['llr_win'] != 0.0)
        assert seen.tolist() == list(range(max(0, i0 - hi), min(n, i0 + lo + 1))), (window, seen)
        assert (got['llr_win'][seen] == 1.5).all() and got['n_mod'].tolist() == [len(seen)] and got['n_can'].tolist() == [0]
        assert got['n_sites'].tolist() == [n]


@pytest.mark.parametrize('dtype', ['float32', 'float64', 'int16'])
def test_ineligible_events(dtype):
    """K12's list, a code usable in one table only, and a code whose sd0 = 1e-200 (|llr| beyond NMOD_LLR_MAX): NaN outputs exactly there,
    the windows of the neighbours shrink accordingly (through llr_win), and n_sites is the count"""
    k, center = F.INELIGIBLE_KC
    p = F.ineligible_inputs(dtype)
    exp = F.restate(p['val'], p['off'], p['base'], k, center, p['mean'], p['sd'], p['alt_mean'], p['alt_sd'], F.INELIGIBLE_WINDOW, F.PARITY_THR,
                    F.PARITY_PRIOR_LOGIT)
    got = _run(p, k, center, F.INELIGIBLE_WINDOW)
    _check_against(got, exp)
    bad = (p['codes'] < 0) | np.isin(p['codes'], (3, 6, 9, 12, 5, 10, 15, F.TINY_SD_CODE)) | ~np.isfinite(R.to_double(p['val']))
    assert all(np.array_equal(np.isnan(got[f]), bad) for f in EVENT_FIELDS)
    off = p['off']
    assert got['n_sites'].tolist() == [int((~bad[off[i]:off[i + 1]]).sum()) for i in range(len(off) - 1)]
    assert got['n_sites'][3] == got['n_sites'][4] == 0 and got['n_mod'][3] == got['n_can'][4] == 0 and not got['status'].any()


def test_reads_are_walls():
    """two adjacent reads: changing every value of the second leaves every bit of the first unchanged, its last events included"""
    k, center = 3, 1
    rng = np.random.default_rng(6)
    mean, sd = R.make_model(k, holes=False)
    mean1, sd1 = F.make_alt_model(k, mean, sd, holes=False)
    m0, m1 = dict(k=k, center=center, mean=mean, sd=sd), dict(k=k, center=center, mean=mean1, sd=sd1)
    for window, n1 in (((2, 2), 300), ((64, 64), 300), ((0, 64), 300), ((2, 2), 3000), ((64, 64), 3000), ((0, 64), 3000)):
        b1, x1 = R.draw_read(rng, n1, k, center, mean, sd, 0.0, 1.0, contaminate=False)
        b2, x2 = R.draw_read(rng, 500, k, center, mean, sd, 0.0, 1.0, contaminate=False)
        off = np.array([0, n1, n1 + 500], np.int64)
        base = np.concatenate([b1, b2])
        a = _engine().read_llr_host(np.concatenate([x1, x2]), off, base, m0, m1, window=window)
        b = _engine().read_llr_host(np.concatenate([x1, x2 + 0.25]), off, base, m0, m1, window=window)
        exp = F.restate(np.concatenate([x1, x2]), off, base, k, center, mean, sd, mean1, sd1, window)
        for f in EVENT_FIELDS:
            assert _bits(a[f][:n1]) == _bits(b[f][:n1]) and _bits(a[f][n1:]) != _bits(b[f][n1:]), (window, n1, f)
        assert all(a[f][0] == b[f][0] for f in READ_FIELDS)
        _check_events(a, exp, slice(n1 - 70, n1 + 70))


def _permuted(p, order):
    lens = np.diff(p['off'])[order]
    off = np.zeros(len(order) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    ev = np.concatenate([np.arange(p['off'][i], p['off'][i + 1]) for i in order]) if len(order) else np.zeros(0, np.int64)
    return ev, off


@pytest.mark.parametrize('dtype,k,center,window', [('int16', 5, 2, 'kmer'), ('float64', 6, 2, (64, 64)), ('float32', 1, 0, (0, 0)), ('int16', 3, 1, (9, 0))])
def test_bits_do_not_depend_on_order_batch_memspace_or_requested_outputs(dtype, k, center, window):
    import torch
    from nanomod_amd import DeviceDetector
    p = F.parity_inputs(k, center, window, dtype)
    first = _run(p, k, center, window)
    nreads = len(p['off']) - 1
    for order in (np.random.default_rng(9).permutation(nreads), np.array([15, 5]), np.array([14]), np.array([10])):   # a batch of one, both classes
        ev, off = _permuted(p, order)
        again = _run(dict(p, val=p['val'][ev], off=off, base=p['base'][ev]), k, center, window)
        assert all(_bits(again[f]) == _bits(first[f][order]) for f in READ_FIELDS)
        assert all(_bits(again[f]) == _bits(first[f][ev]) for f in EVENT_FIELDS)
    only = _run(p, k, center, window, want=('llr_win',))
    assert set(only) == {'llr_win'} | set(READ_FIELDS) and all(_bits(only[f]) == _bits(first[f]) for f in only)
    det = DeviceDetector(0)
    t = lambda x: torch.from_numpy(np.array(x)).cuda()
    args = (t(p['val']), t(p['off']), t(R.as_bytes(p['base'])), t(p['mean']), t(p['sd']), t(p['alt_mean']), t(p['alt_sd']), k, center)
    kw = dict(window=window, thr=F.PARITY_THR, prior_logit=F.PARITY_PRIOR_LOGIT)
    out = det.read_llr(*args, **kw)
    assert all(_bits(out[f].cpu().numpy()) == _bits(first[f]) for f in EVENT_FIELDS + READ_FIELDS)
    with torch.cuda.stream(torch.cuda.Stream()):
        side = det.read_llr(*args, want=('llr_win',), **kw)
        torch.cuda.current_stream().synchronize()
    assert set(side) == {'llr_win'} | set(READ_FIELDS) and all(_bits(side[f].cpu().numpy()) == _bits(first[f]) for f in side)
    for f in EVENT_FIELDS:
        out[f].zero_()
    again = det.read_llr(*args, out=out, **kw)
    assert again is out and all(_bits(out[f].cpu().numpy()) == _bits(first[f]) for f in EVENT_FIELDS + READ_FIELDS)
    for bad in (dict(window=(65, 0)), dict(thr=0.0), dict(want=('x',)), dict(prior_logit=701.0), dict(out=dict(out, status=out['status'][:3]))):
        with pytest.raises(ValueError):
            det.read_llr(*args, **dict(kw, **bad))
    with pytest.raises(ValueError):
        det.read_llr(args[0], args[1], args[2][:-1], *args[3:])
    with pytest.raises(ValueError):
        det.read_llr(*args[:6], args[6][:-1], k, center)


def test_site_llr():
    """rows of lengths {0, 1, 63, 64, 65, 1 000, 70 000} with NaN, +-inf, values exactly +-thr and their neighbours both ways, an all-NaN
    row and an all-ambiguous row: the counts equal numpy's, frac is bit-equal, CSR equals the stride form"""
    import torch
    from nanomod_amd import DeviceDetector
    thr = 2.5
    rng = np.random.default_rng(12)
    lens = [0, 1, 63, 64, 65, 1000, 70000, 64, 5, 1, 0, 40]
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    s = rng.normal(0.0, 4.0, off[-1])
    u = rng.random(off[-1])
    s[u < 0.1] = np.nan
    edge = [thr, -thr, np.nextafter(thr, 9.0), np.nextafter(thr, 0.0), np.nextafter(-thr, -9.0), np.nextafter(-thr, 0.0), np.inf, -np.inf, 0.0, -0.0]
    s[(u >= 0.1) & (u < 0.3)] = rng.choice(edge, int(((u >= 0.1) & (u < 0.3)).sum()))
    s[off[7]:off[8]] = np.nan                                                # all NaN
    s[off[8]:off[9]] = [np.inf, -np.inf, np.nan, thr, -thr]
    s[off[9]] = -thr
    s[off[11]:off[12]] = rng.uniform(-2.4, 2.4, 40)                          # all ambiguous
    exp = F.site_llr(s, off, thr)
    assert np.isnan(exp['frac'][[0, 7, 10, 11]]).all() and exp['n_valid'][11] == 40 and exp['n_valid'][7] == 0 and exp['frac'][9] == 0.0
    assert exp['n_valid'][6] > 50000 and (s == thr).sum() > 1000 and (s == -thr).sum() > 1000 and exp['n_mod'][8] == 2 and exp['n_valid'][8] == 2
    got = _engine().site_llr_host(s, off, thr=thr)
    for f in ('n_valid', 'n_mod', 'n_can'):
        assert got[f].dtype == np.int32 and np.array_equal(got[f], exp[f]), f
    assert _bits(got['frac']) == _bits(exp['frac'])
    det = DeviceDetector(0)
    dev = det.site_llr(torch.from_numpy(s).cuda(), off=torch.from_numpy(off).cuda(), thr=thr)
    assert all(_bits(dev[f].cpu().numpy()) == _bits(got[f]) for f in got)
    for stride in (3, 64, 65, 1000):                                          # the stride form over the same values, whole rows
        n = (len(s) // stride) * stride
        soff = np.arange(0, n + 1, stride, dtype=np.int64)
        a = _engine().site_llr_host(s[:n], None, stride=stride, thr=thr)
        b = _engine().site_llr_host(s[:n], soff, thr=thr)
        e = F.site_llr(s[:n], soff, thr)
        assert all(_bits(a[f]) == _bits(b[f]) == _bits(e[f].astype(a[f].dtype)) for f in a), stride
        d = det.site_llr(torch.from_numpy(s[:n]).cuda(), stride=stride, thr=thr)
        assert all(_bits(d[f].cpu().numpy()) == _bits(a[f]) for f in a)
    other = _engine().site_llr_host(s, off, thr=1.0)
    assert np.array_equal(other['n_valid'], exp['n_valid']) and np.array_equal(other['n_mod'], F.site_llr(s, off, 1.0)['n_mod'])
    for kw in (dict(thr=0.0), dict(stride=0), dict(off=torch.from_numpy(off))):
        with pytest.raises(ValueError):
            det.site_llr(torch.from_numpy(s).cuda(), **kw)


def _check_chain(table, sites, reads, exp, rows, s):
    for f in READ_FIELDS:
        assert np.array_equal(table[f], exp[f]), f
    assert np.array_equal(table['events'], np.diff(reads['off'])) and np.array_equal(table['start'], reads['start'])
    assert table['chrom'].tolist() == reads['chrom'].tolist() and table['strand'].tolist() == reads['strand'].tolist()
    for f in ('chrom', 'strand', 'pos'):
        assert np.array_equal(np.asarray(sites[f]).astype(rows[f].dtype), rows[f]), f
    assert np.array_equal(sites['n_reads'], np.diff(rows['off']))
    for f in ('n_valid', 'n_mod', 'n_can'):
        assert np.array_equal(sites[f], s[f]), f
    assert _bits(sites['frac']) == _bits(s['frac'])


@pytest.mark.parametrize('window', ['kmer', (0, 0), (1, 3)])
def test_chain_equals_the_restatement(window):
    """call_reads_llr — ratios, pivot and counts on the device — against the restatement chained through a numpy pivot: exact integers
    and frac bits.  (That the planted base stands out in the restatement is tests/test_read_llr.py's.)"""
    import math
    reads, model, alt, planted = F.chain_inputs()
    prior = 0.2
    exp, rows, s = F.restate_chain(reads, model, alt, window, 2.5, math.log(prior / (1.0 - prior)))
    assert exp['thr_margin'] > 0.0
    lines = []
    table, sites, ev = RL.call_reads_llr(reads, model, alt, window=window, thr=2.5, prior=prior, events=True, log=lines.append)
    _check_chain(table, sites, reads, exp, rows, s)
    _check_events(ev, exp)
    assert len(lines) == 1 and lines[0].startswith('readllr: 200 read(s), %d of %d event(s) scored, %d modified and %d canonical' % (
        exp['n_sites'].sum(), len(reads['norm_mean']), exp['n_mod'].sum(), exp['n_can'].sum()))
    table2, sites2 = RL.call_reads_llr(reads, model, alt, window=window, log=lambda *a: None)
    assert all(_bits(table2[f]) == _bits(table[f]) for f in READ_FIELDS) and all(_bits(sites2[f]) == _bits(sites[f]) for f in sites)
    if window == 'kmer':                                                     # the device chain finds the planted base too
        for strand in '+-':
            m = sites['strand'] == strand
            assert sites['pos'][m][np.argmax(sites['n_mod'][m])] == planted
        thin = dict(model, n_positions=np.where(np.arange(64) % 2, 5, 1))   # min_positions masks half of the unmodified model
        t3, s3 = RL.call_reads_llr(reads, thin, dict(alt, n_positions=np.full(64, 5)), min_positions=2, log=lambda *a: None)
        e3, r3, c3 = F.restate_chain(reads, dict(model, mean=np.where(np.arange(64) % 2, model['mean'], np.nan)), alt)
        assert e3['thr_margin'] > 0.0
        _check_chain(t3, s3, reads, e3, r3, c3)
        assert 0 < t3['n_sites'].sum() < table['n_sites'].sum()


def test_chain_with_rescale_equals_rescaling_first():
    """rescale=dict(...): K11 on the device feeding its tensor straight in, bit for bit what rescale.rescale_reads and a plain call give"""
    from nanomod_amd import rescale
    k, center = 3, 1
    mean, sd = R.make_model(k, holes=False)
    mean1, sd1 = F.make_alt_model(k, mean, sd, holes=False)
    reads = R.make_read_set(4243, k, center, mean, sd, reads_per_strand=10, planted=True, contaminate=True)
    ones = np.ones(64, np.int64)
    model, alt = dict(k=k, center=center, mean=mean, sd=sd, n_positions=ones), dict(k=k, center=center, mean=mean1, sd=sd1, n_positions=ones)
    opts = dict(min_events=60, clip_sigma=2.5)
    first, fit = rescale.rescale_reads(reads, model, log=lambda *a: None, **opts)
    assert (fit['status'] == 0).all() and np.abs(fit['scale'] - 1.0).max() > 0.1
    want_t, want_s, want_e = RL.call_reads_llr(first, model, alt, events=True, log=lambda *a: None)
    got_t, got_s, got_e = RL.call_reads_llr(reads, model, alt, rescale=opts, events=True, log=lambda *a: None)
    assert all(_bits(got_e[f]) == _bits(want_e[f]) for f in EVENT_FIELDS)
    assert all(_bits(got_t[f]) == _bits(want_t[f]) for f in want_t) and all(_bits(got_s[f]) == _bits(want_s[f]) for f in want_s)
    assert _bits(got_t['shift']) == _bits(fit['shift']) and _bits(got_t['scale']) == _bits(fit['scale']) and not got_t['rescale_status'].any()
    plain = RL.call_reads_llr(reads, model, alt, events=True, log=lambda *a: None)[2]
    assert _bits(plain['llr']) != _bits(got_e['llr'])                        # the rescaling is not a no-op here


def test_end_to_end_through_the_command_line():
    from nanomod_amd import cli, container, kmermodel
    reads, model, alt, planted = F.chain_inputs()
    exp, rows, s = F.restate_chain(reads, model, alt)
    assert exp['thr_margin'] > 0.0
    with tempfile.TemporaryDirectory() as tmp:
        r_path, m_path, a_path, g_path, e_path, out = (os.path.join(tmp, n) for n in ('reads.npz', 'model.npz', 'alt.npz', 'group.npz', 'events.npz', 'cli'))
        container.save_reads(r_path, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
        zeros = np.zeros(64, np.int64)
        for path, m in ((m_path, model), (a_path, alt)):
            kmermodel.save_kmer_model(path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                                 n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
        argv = ['readllr', '--wrkBase1', r_path, '--kmerModel', m_path, '--altModel', a_path, '--outFolder', out, '--outLevel', '3']
        assert cli.main(argv + ['--FileID', 'run', '--outEvents', e_path]) == 0
        t = [ln.split() for ln in open(os.path.join(out, 'run_read_llr.txt')).read().splitlines()]
        assert len(t) == 200 and all(len(r) == 9 for r in t)
        assert [int(r[0]) for r in t] == list(range(200)) and [r[1] for r in t] == reads['chrom'].tolist() and [r[2] for r in t] == reads['strand'].tolist()
        for col, want in ((3, reads['start']), (4, np.diff(reads['off'])), (5, exp['n_sites']), (6, exp['n_mod']), (7, exp['n_can']), (8, exp['status'])):
            assert [int(r[col]) for r in t] == np.asarray(want).tolist(), col
        u = [ln.split() for ln in open(os.path.join(out, 'run_site_llr.txt')).read().splitlines()]
        assert len(u) == len(rows['pos']) and all(len(r) == 9 for r in u)
        assert [r[0] for r in u] == rows['chrom'].tolist() and [r[1] for r in u] == rows['strand'].tolist()
        for col, want in ((2, rows['pos'] + 1), (4, np.diff(rows['off'])), (5, s['n_valid']), (6, s['n_mod']), (7, s['n_can'])):
            assert [int(r[col]) for r in u] == np.asarray(want).tolist(), col
        assert [r[8] for r in u] == ['%.6f' % v for v in s['frac']] and {r[3] for r in u} <= set('ACGT')
        ev = np.load(e_path)
        assert sorted(ev.files) == ['llr', 'llr_win', 'off', 'p_mod'] and np.array_equal(ev['off'], reads['off'])
        _check_events({f: ev[f] for f in EVENT_FIELDS}, exp)
        # --llrWindow LO,HI, --llrThreshold, --prior and --rescale 1: the fit of `rescale` with its defaults, then the calls
        assert cli.main(argv + ['--FileID', 'rs', '--rescale', '1', '--llrWindow', '0,2', '--llrThreshold', '4', '--prior', '0.1']) == 0
        want_t, _ = RL.call_reads_llr(reads, kmermodel.load_kmer_model(m_path), kmermodel.load_kmer_model(a_path), window=(0, 2), thr=4.0, prior=0.1,
                                      rescale={}, log=lambda *a: None)
        t = [ln.split() for ln in open(os.path.join(out, 'rs_read_llr.txt')).read().splitlines()]
        assert [int(r[6]) for r in t] == want_t['n_mod'].tolist() and [int(r[7]) for r in t] == want_t['n_can'].tolist()
        assert sum(int(r[6]) for r in t) > 50
        # a per-position container is refused, with the message
        container.save_group(g_path, ['c'], ['+'], [0], ['A'], [0, 1], np.zeros(1, np.float32))
        assert cli.main(['readllr', '--wrkBase1', g_path, '--kmerModel', m_path, '--altModel', a_path, '--outFolder', out]) == 1


def test_a_read_beyond_max_deep_is_too_large():
    """2^24 events: one more than NMOD_MAX_DEEP.  The read gets NaN events, zero counts and its status; its neighbour is called"""
    k, center = 3, 1
    mean, sd = R.make_model(k, holes=False)
    mean1, sd1 = F.make_alt_model(k, mean, sd, holes=False)
    rng = np.random.default_rng(8)
    b0, x0 = R.draw_read(rng, 200, k, center, mean, sd, 0.0, 1.0)
    n = F.MAX_DEEP + 1
    val = np.concatenate([(np.arange(n, dtype=np.int64) % 2001 - 1000).astype(np.int16), R.cast(x0, 'int16')])
    base = np.concatenate([np.tile(np.frombuffer(b'ACGTTGCA', np.uint8), n // 8), b0])
    off = np.array([0, n, n + 200], np.int64)
    m0, m1 = dict(k=k, center=center, mean=mean, sd=sd), dict(k=k, center=center, mean=mean1, sd=sd1)
    got = _engine().read_llr_host(val, off, base, m0, m1, want=('llr_win',))
    exp = F.restate(val[n:], np.array([0, 200], np.int64), b0, k, center, mean, sd, mean1, sd1)
    assert exp['thr_margin'] > 0.0
    assert got['status'].tolist() == [F.TOO_LARGE, 0] and got['n_sites'].tolist() == [0, exp['n_sites'][0]]
    assert got['n_mod'].tolist() == [0, exp['n_mod'][0]] and got['n_can'].tolist() == [0, exp['n_can'][0]] and np.isnan(got['llr_win'][:n]).all()
    _check_events(dict(llr_win=got['llr_win'][n:]), exp)
