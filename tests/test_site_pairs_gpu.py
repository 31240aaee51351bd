"""-m gpu: nmod_pair_index / nmod_site_pairs (K16) on the device against the restatement (tests/pairs_ref.py): the counts as exact
integers on constructed reads, the two forms of the read kernel and the invariances as identical bytes, the pair kernel on planted
tables within the derived gate, the stream contract, and the chain K13 -> K16 through readllr.cooccur_reads_llr and `cli readpairs`."""
import os
import tempfile

import numpy as np
import pytest

import pairs_ref as P
import readllr_ref as RF
import stream_cases as S
from nanomod_amd import _lib as L
from test_engine_device_args_gpu import same
from test_site_pairs import LARGE_TABLES, _key

pytestmark = pytest.mark.gpu

THR = 2.5
IN = float(np.nextafter(THR, 0.0))                                            # one ulp inside the threshold: not called
ALL = ('counts', 'first', 'second', 'log_or', 'se', 'phi', 'p_fisher', 'status')


def _engine():
    from nanomod_amd import engine
    return engine


@pytest.fixture(scope='module')
def det():
    return _engine().DeviceDetector(0)


def _case(reads, key, max_dist):
    """reads: (cs, start, scores) triples; the flat arrays of the entries and the restated pair index"""
    cs = np.array([r[0] for r in reads], np.int32)
    start = np.array([r[1] for r in reads], np.int64)
    roff = np.zeros(len(reads) + 1, np.int64)
    roff[1:] = np.cumsum([len(r[2]) for r in reads])
    score = np.concatenate([np.asarray(r[2], np.float64) for r in reads]) if reads else np.zeros(0)
    key = np.asarray(key, np.int64)
    return dict(cs=cs, start=start, roff=roff, score=score, key=key, max_dist=max_dist, poff=P.pair_index_ref(key, max_dist))


def _device(det, c, **kw):
    """pair_index and site_pairs on device tensors of case c -> (poff, results) as numpy"""
    import torch
    t = {f: torch.from_numpy(c[f]).cuda() for f in ('cs', 'start', 'roff', 'score', 'key')}
    poff, npairs = det.pair_index(t['key'], c['max_dist'])
    res = det.site_pairs(t['cs'], t['start'], t['roff'], t['score'], t['key'], poff, npairs, thr=THR, **kw)
    return poff.cpu().numpy(), {f: v.cpu().numpy() for f, v in res.items()}


def _counts_ref(c):
    return P.counts_ref(c['cs'], c['start'], c['roff'], c['score'], c['key'], c['poff'], THR)


def _check_stats(res, counts, min_reads, poff):
    ref = P.pair_stats_ref(counts, min_reads, poff)
    assert same(res['status'], ref['status']) and same(res['first'], ref['first']) and same(res['second'], ref['second'])
    assert P.close_log_or(res['log_or'], ref['log_or']) and P.close_rel(res['se'], ref['se']) and P.close_rel(res['phi'], ref['phi'])
    few = (ref['status'] & P.TOO_FEW) != 0
    assert np.all(np.isnan(res['p_fisher'][few])) and not np.any(np.isnan(res['p_fisher'][~few]))
    for j in np.flatnonzero(~few):
        n00, n01, n10, n11 = (int(v) for v in counts[4 * j:4 * j + 4])
        assert P.p_within_gate(float(res['p_fisher'][j]), (n11, n10, n01, n00)), (j, counts[4 * j:4 * j + 4], res['p_fisher'][j])
    return ref


# ------------------------------------------------------------------------------------------------------------ constructed reads
@pytest.fixture(scope='module')
def mixed():
    """Three (chrom, strand) ids with the same site positions, reads of 1 .. 60 events on all of them with scores at, inside and beyond
    +-thr, NaN and infinities; sites 100, 110 and 111 with max_dist 10 (the boundary); reads that cover no site, one site, and two
    sites at their first and last event"""
    rng = np.random.default_rng(1611)
    pos = np.unique(np.concatenate((rng.choice(200, 70, replace=False), [100, 110, 111, 150, 160])))
    pos = pos[(pos < 151) | (pos > 159)]                                      # (150 and 160 are neighbours in key order)
    key = np.array([_key(cs, p) for cs in (0, 1, 2) for p in pos], np.int64)
    values = np.array([3.0, -3.0, THR, -THR, IN, -IN, np.nan, 0.0, np.inf, -np.inf, 40.0, -7.5])
    reads = []
    for _ in range(400):
        n = int(rng.integers(1, 61))
        reads.append((int(rng.integers(0, 3)), int(rng.integers(0, 215 - n)), values[rng.integers(0, len(values), n)]))
    reads.append((0, 300, np.full(30, 3.0)))                                  # covers no site
    reads.append((1, 151, np.full(9, 3.0)))                                   # 151 .. 159: none either
    reads.append((1, 152, np.full(9, 3.0)))                                   # 152 .. 160: one site, at its first event ('-')
    reads.append((0, 150, np.array([3.0] + [0.0] * 9 + [-3.0])))              # 150 .. 160: two sites, at the first and the last event
    reads.append((1, 150, np.array([3.0] + [0.0] * 9 + [-3.0])))              # the same on '-': event 0 lies at 160
    reads.append((2, 100, np.array([THR] + [0.0] * 9 + [-THR, IN])))          # 100 and 110 called exactly at +-thr, 111 one ulp inside
    c = _case(reads, key, 10)
    c['want'] = _counts_ref(c)
    return c


def test_counts_on_constructed_reads(det, mixed):
    poff, res = _device(det, mixed, min_reads=4)
    assert same(poff, mixed['poff'])
    assert same(res['counts'], mixed['want']) and res['counts'].sum() > 1000
    pos = mixed['key'] & P.POS_MASK
    a, b = res['first'].astype(np.int64), res['second'].astype(np.int64)
    assert np.all(mixed['key'][a] >> 40 == mixed['key'][b] >> 40) and (pos[b] - pos[a]).max() == 10      # the boundary is kept, 11 is not
    tab = res['counts'].reshape(-1, 4)
    j = {(int(mixed['key'][x]), int(mixed['key'][y])): i for i, (x, y) in enumerate(zip(a, b))}
    # the two-site reads: MOD at 150 and CAN at 160 on '+' (n10), CAN at 150 and MOD at 160 on '-' (n01) — the other reads there aside
    only = _case([r for r in zip(mixed['cs'][-3:-1], mixed['start'][-3:-1], (mixed['score'][-34:-23], mixed['score'][-23:-12]))], mixed['key'], 10)
    alone = _counts_ref(only).reshape(-1, 4)
    assert alone[j[_key(0, 150), _key(0, 160)]].tolist() == [0, 0, 1, 0] and alone[j[_key(1, 150), _key(1, 160)]].tolist() == [0, 1, 0, 0]
    # exactly +-thr is a call (n10 of (100, 110) on cs 2 counts that read), one ulp inside is none
    last = _counts_ref(_case([(2, 100, mixed['score'][-12:])], mixed['key'], 10)).reshape(-1, 4)
    assert last[j[_key(2, 100), _key(2, 110)]].tolist() == [0, 0, 1, 0] and last[j[_key(2, 110), _key(2, 111)]].sum() == 0
    assert tab[j[_key(2, 100), _key(2, 110)]][2] >= 1
    _check_stats(res, res['counts'], 4, poff)


def test_host_and_device_memspace_and_fewer_outputs_give_identical_bytes(det, mixed):
    _, dev = _device(det, mixed, min_reads=4)
    eng = _engine()
    poff = eng.pair_index_host(mixed['key'], mixed['max_dist'])
    assert same(poff, mixed['poff'])
    host = eng.site_pairs_host(mixed['cs'], mixed['start'], mixed['roff'], mixed['score'], mixed['key'], poff, thr=THR, min_reads=4)
    assert set(host) == set(dev) == set(ALL)
    for f in ALL:
        assert same(host[f], dev[f]), f
    for want in (('p_fisher',), ('counts',), ('phi', 'status'), ('first', 'second', 'log_or')):
        _, part = _device(det, mixed, min_reads=4, want=want)
        assert set(part) == set(want)
        for f in want:
            assert same(part[f], dev[f]), (want, f)


def test_a_permutation_of_the_reads_changes_nothing(det, mixed):
    _, dev = _device(det, mixed, min_reads=4)
    n = len(mixed['cs'])
    order = np.random.default_rng(1612).permutation(n)
    reads = [(mixed['cs'][r], mixed['start'][r], mixed['score'][mixed['roff'][r]:mixed['roff'][r + 1]]) for r in order]
    _, perm = _device(det, _case(reads, mixed['key'], 10), min_reads=4)
    for f in ALL:
        assert same(perm[f], dev[f]), f


@pytest.mark.parametrize('nsites', [L.PAIRS_LDS_MAX + 1, L.PAIRS_LDS_MAX + 2])
def test_direct_and_table_form_give_identical_bytes(det, nsites):
    """neighbouring positions with max_dist 1: nsites - 1 pairs, NMOD_PAIRS_LDS_MAX (the table form) and one more (the direct form);
    the same reads through the other form by the per-call flag"""
    rng = np.random.default_rng(1613)
    key = np.array([_key(1, p) for p in range(nsites)], np.int64)
    reads = [(1, int(rng.integers(0, nsites - 40)), rng.choice([3.0, -3.0, 0.0], int(rng.integers(2, 41)))) for _ in range(3000)]
    c = _case(reads, key, 1)
    assert c['poff'][-1] == nsites - 1
    _, res = _device(det, c, min_reads=1, want=('counts',))
    _, forced = _device(det, c, min_reads=1, want=('counts',), force_direct=True)
    assert same(res['counts'], forced['counts']) and same(res['counts'], _counts_ref(c)) and res['counts'].sum() > 10000


def test_reads_of_the_workgroup_class_with_partners_across_windows(det):
    """two reads beyond NMOD_CALLS_WAVE_MAX events, '+' and '-', every position a candidate site and max_dist beyond the 256 sites of a
    staged window: a site's partners lie in the next window and the one after"""
    rng = np.random.default_rng(1614)
    n = L.CALLS_WAVE_MAX + 150
    key = np.array([_key(cs, p) for cs in (0, 1) for p in range(n + 40)], np.int64)
    reads = [(0, 7, np.where(rng.random(n) < 0.12, rng.choice([3.0, -3.0], n), 0.0)),
             (1, 33, np.where(rng.random(n) < 0.12, rng.choice([3.0, -3.0], n), np.nan)),
             (1, 0, np.where(rng.random(500) < 0.3, 3.0, 0.0))]                  # a read of the wave class over the same pairs
    c = _case(reads, key, 300)
    poff, res = _device(det, c, want=('counts',))
    assert same(poff, c['poff']) and poff[-1] > 10 ** 6
    want = _counts_ref(c)
    assert same(res['counts'], want)
    far = res['counts'].reshape(-1, 4).sum(1)[np.arange(poff[-1]) - np.repeat(poff[:-1], np.diff(poff)) >= 256]
    assert far.sum() > 1000                                                   # pairs more than a window apart were counted


def test_more_short_reads_than_the_grid_has_waves(det):
    rng = np.random.default_rng(1615)
    key = np.array([_key(cs, p) for cs in (0, 1) for p in range(0, 400, 2)], np.int64)
    reads = [(int(rng.integers(0, 2)), int(rng.integers(0, 380)), rng.choice([3.0, -3.0, 0.0, 0.0], int(rng.integers(15, 26)))) for _ in range(20000)]
    c = _case(reads, key, 6)
    poff, res = _device(det, c, want=('counts',))
    assert same(res['counts'], _counts_ref(c)) and poff[-1] <= L.PAIRS_LDS_MAX
    _, forced = _device(det, c, want=('counts',), force_direct=True)
    assert same(res['counts'], forced['counts'])


# ------------------------------------------------------------------------------------------------------------ the pair kernel
def test_pair_kernel_on_planted_tables(det):
    """one pair of neighbouring sites per table, every read of two events: the support at NMOD_PAIRS_THREAD_MAX tables and one more, a
    table with margins of 2 000 and p about 1e-111, one whose p underflows, a zero margin, a pair below min_reads"""
    tables = LARGE_TABLES + [(5, 7, 0, 0), (2, 1, 1, 1), (30, 4, 6, 25)]
    reads = []
    for k, (n11, n10, n01, n00) in enumerate(tables):
        for n, ev in ((n11, (3.0, 3.0)), (n10, (3.0, -3.0)), (n01, (-3.0, 3.0)), (n00, (-3.0, -3.0))):
            reads += [(0, 10 * k, np.array(ev))] * n
    key = np.array([_key(0, 10 * k + d) for k in range(len(tables)) for d in (0, 1)], np.int64)
    c = _case(reads, key, 1)
    poff, res = _device(det, c, min_reads=10)
    assert same(poff, c['poff']) and poff[-1] == len(tables)
    assert res['counts'].reshape(-1, 4)[:, ::-1].tolist() == [list(t) for t in tables]
    ref = _check_stats(res, res['counts'], 10, poff)
    assert res['first'].tolist() == list(range(0, 2 * len(tables), 2)) and res['second'].tolist() == list(range(1, 2 * len(tables), 2))
    # the restated recurrence is the device's own order of operations: the same bits
    assert same(res['p_fisher'], ref['p_fisher']), (res['p_fisher'], ref['p_fisher'])
    assert 1e-112 < res['p_fisher'][2] < 1e-110 and res['p_fisher'][3] == P.DBL_MIN
    assert res['status'].tolist() == [0, 0, 0, 0, L.PAIRS_DEGENERATE, L.PAIRS_TOO_FEW, 0]
    assert res['p_fisher'][4] == 1.0 and np.isnan(res['phi'][4]) and np.isfinite(res['log_or'][4]) and np.isfinite(res['se'][4])
    assert all(np.isnan(res[f][5]) for f in ('log_or', 'se', 'phi', 'p_fisher')) and res['counts'][20:24].tolist() == [1, 1, 1, 2]


# ------------------------------------------------------------------------------------------------------------ the stream
def test_side_stream_and_no_wait_for_the_work_before_it(det, mixed):
    """On a side stream the result is the default stream's; and behind a stall of stream_cases.T_MS on a fresh stream (the inputs put in
    place behind the stall, a decoy behind the call: tests/stream_cases.py) the call returns while the stall still runs, and its result
    is the one of the real inputs"""
    import torch
    _, want = _device(det, mixed, min_reads=4)
    real = {f: mixed[f] for f in ('cs', 'start', 'roff', 'score', 'key')}
    decoy = dict(real, score=-mixed['score'], start=mixed['start'] + 1)
    sw = S.Swapped(real, decoy)
    poff = torch.from_numpy(mixed['poff']).cuda()
    npairs = int(mixed['poff'][-1])
    call = lambda out=None: det.site_pairs(sw.t['cs'], sw.t['start'], sw.t['roff'], sw.t['score'], sw.t['key'], poff, npairs, thr=THR, min_reads=4, out=out)
    side = torch.cuda.Stream()
    sw.load_real()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        first = call()
    side.synchronize()
    for f in ALL:
        assert same(first[f].cpu().numpy(), want[f]), f
    for _ in range(2):                                                        # (two streams, for stream_cases' reason: hardware queues)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            out = S.fill_sentinel({f: torch.empty_like(v) for f, v in first.items()})
        stream.synchronize()
        with torch.cuda.stream(stream):
            S.stall(stream, S.T_MS)
            event = torch.cuda.Event()
            event.record(stream)
            sw.load_real()
            got = call(out)
            sw.load_decoy()
            early = event.query()
        assert not early, 'the stall of %g ms had ended when the call returned' % S.T_MS
        stream.synchronize()
        for f in ALL:
            assert same(got[f].cpu().numpy(), want[f]), f
        assert sw.holds('decoy')


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def chain():
    reads, model, alt, planted, modified = P.cooccur_inputs()
    exp = RF.restate(reads['norm_mean'], reads['off'], reads['base'], model['k'], model['center'], model['mean'], model['sd'], alt['mean'], alt['sd'],
                     'kmer', THR, 0.0)
    assert exp['thr_margin'] > 0.0                                            # no window sum within its gate of +-thr: the calls are the device's
    cs = (reads['strand'] == '-').astype(np.int32)
    key = np.array([_key(s, p) for s in (0, 1) for p in planted], np.int64)
    poff = P.pair_index_ref(key, 40)
    counts = P.counts_ref(cs, reads['start'], reads['off'], exp['llr_win'], key, poff, THR)
    sites = (np.array(['chrT'] * 6), np.array(['+'] * 3 + ['-'] * 3), np.array(list(planted) * 2))
    return dict(reads=reads, model=model, alt=alt, planted=planted, sites=sites, key=key, poff=poff, counts=counts,
                ref=P.pair_stats_ref(counts, 10, poff))


def test_end_to_end_through_cooccur_reads_llr(chain):
    from nanomod_amd import readllr
    A, B, C_ = chain['planted']
    lines = []
    pairs = readllr.cooccur_reads_llr(chain['reads'], chain['model'], chain['alt'], sites=chain['sites'], max_dist=40, thr=THR, min_reads=10,
                                      fdr='bh', log=lines.append)
    assert len(lines) == 1 and lines[0].startswith('readpairs: 160 read(s); 6 candidate site(s), 6 pair(s) at most 40 apart')
    assert pairs['pos_a'].tolist() == [A, A, B] * 2 and pairs['pos_b'].tolist() == [B, C_, C_] * 2 and pairs['strand'].tolist() == ['+'] * 3 + ['-'] * 3
    assert pairs['dist'].tolist() == [20, 40, 20] * 2 and set(pairs['chrom'].tolist()) == {'chrT'}
    got = np.stack([pairs[f] for f in ('n00', 'n01', 'n10', 'n11')], 1).astype(np.int32).ravel()
    assert same(got, chain['counts'])
    res = dict(pairs, first=chain['ref']['first'], second=chain['ref']['second'])
    ref = _check_stats(res, chain['counts'], 10, chain['poff'])
    # the restatement's own verdict, at the 5 % level over the six pairs: (A, B) go together on both strands, (A, C) do not
    for ab, ac in ((0, 1), (3, 4)):
        assert ref['log_or'][ab] > 0.0 and ref['p_fisher'][ab] < 0.05 / 6 < ref['p_fisher'][ac]
        assert pairs['log_or'][ab] > 0.0 and pairs['p_fisher'][ab] < 0.05 / 6 < pairs['p_fisher'][ac]
    want_q, _ = _engine().fdr_adjust_host(pairs['p_fisher'], 'bh')
    assert same(pairs['q'], want_q[0])
    # the default choice of sites, K14's estimates at q <= site_alpha, finds the planted bases among its candidates: their pairs are
    # the same rows whatever else is a candidate
    auto = readllr.cooccur_reads_llr(chain['reads'], chain['model'], chain['alt'], max_dist=40, thr=THR, min_reads=10, log=lambda *a: None)
    for i in range(6):
        hit = np.flatnonzero((auto['pos_a'] == pairs['pos_a'][i]) & (auto['pos_b'] == pairs['pos_b'][i]) & (auto['strand'] == pairs['strand'][i]))
        assert len(hit) == 1, i
        for f in ('n11', 'n10', 'n01', 'n00', 'log_or', 'se', 'phi', 'p_fisher', 'status'):
            assert same(auto[f][hit[0]], pairs[f][i]), (i, f)


def test_the_command_line_writes_the_same_rows(chain):
    from nanomod_amd import cli, container, kmermodel, readllr
    reads = chain['reads']
    with tempfile.TemporaryDirectory() as tmp:
        r_path, m_path, a_path, s_path, out = (os.path.join(tmp, n) for n in ('reads.npz', 'model.npz', 'alt.npz', 'sites.txt', 'cli'))
        container.save_reads(r_path, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
        zeros = np.zeros(64, np.int64)
        for path, m in ((m_path, chain['model']), (a_path, chain['alt'])):
            kmermodel.save_kmer_model(path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                                 n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
        open(s_path, 'w').writelines('%s %s %d\n' % (c, s, p + 1) for c, s, p in zip(*chain['sites']))
        argv = ['readpairs', '--wrkBase1', r_path, '--kmerModel', m_path, '--altModel', a_path, '--sites', s_path, '--maxDist', '40', '--fdr', 'by',
                '--outFolder', out, '--FileID', 'run', '--outLevel', '3']
        assert cli.main(argv) == 0
        pairs = readllr.cooccur_reads_llr(reads, kmermodel.load_kmer_model(m_path), kmermodel.load_kmer_model(a_path), sites=chain['sites'], max_dist=40,
                                          fdr='by', log=lambda *a: None)
        readllr.write_site_pairs(os.path.join(tmp, 'want.txt'), pairs)
        text = open(os.path.join(out, 'run_site_pairs.txt')).read()
        assert text == open(os.path.join(tmp, 'want.txt')).read()
        rows = [ln.split() for ln in text.splitlines()]
        assert len(rows) == 6 and all(len(r) == 15 for r in rows)
        assert [[int(v) for v in r[5:9]] for r in rows] == chain['counts'].reshape(-1, 4)[:, ::-1].tolist()
        assert [int(r[2]) for r in rows] == (pairs['pos_a'] + 1).tolist() and [r[12] for r in rows] == ['%.3E' % p for p in chain['ref']['p_fisher']]
