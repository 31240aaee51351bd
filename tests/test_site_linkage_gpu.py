"""-m gpu: nmod_pair_rows_count / nmod_pair_rows_fill / nmod_pair_linkage (K18) on the device against the restatement
(tests/linkage_ref.py): the rows as exact bytes on constructed reads, the margins as nmod_site_stoich's bits, the linkage within gates
built from stoich_ref's constants with test_site_stoich_gpu's helper (the restatement's stage 2 at the device's margins, which the
bit-equality with K14 ties to K14's own gates), every status bit on planted rows, the independence of a pair's bits from everything
but its row, batches larger than the persistent grids, the stream contract, and the chain through readllr.cooccur_reads_llr and
`cli readpairs --soft 1`."""
import os
import tempfile

import numpy as np
import pytest

import grid_cases as G
import linkage_ref as K
import pairs_ref as P
import stoich_ref as F
import stream_cases as S
from nanomod_amd import _lib as L
from test_engine_device_args_gpu import same
from test_site_pairs import _key
from test_site_pairs_gpu import _case
from test_site_stoich_gpu import _share

pytestmark = pytest.mark.gpu

THR = 2.5
ROW_FIELDS = ('prow_off', 'sa', 'sb', 'read')
ALL = K.FIELDS + ('n_valid', 'iters', 'status')


def _engine():
    from nanomod_amd import engine
    return engine


@pytest.fixture(scope='module')
def det():
    return _engine().DeviceDetector(0)


def _rows_ref(c):
    return K.pair_rows_ref(c['cs'], c['start'], c['roff'], c['score'], c['key'], c['poff'])


def _rows_device(det, c):
    import torch
    t = {f: torch.from_numpy(c[f]).cuda() for f in ('cs', 'start', 'roff', 'score', 'key', 'poff')}
    res = det.pair_rows(t['cs'], t['start'], t['roff'], t['score'], t['key'], t['poff'], int(c['poff'][-1]))
    return {f: v.cpu().numpy() for f, v in res.items()}


def _same_rows(got, want):
    for f in ROW_FIELDS:
        assert got[f].dtype == want[f].dtype and same(got[f], want[f]), f


# ------------------------------------------------------------------------------------------------------------ the rows
@pytest.fixture(scope='module')
def mixed():
    """test_site_pairs_gpu's `mixed` in its manner: three (chrom, strand) ids with the same site positions, reads of 1 .. 60 events with
    scores beyond and inside +-thr, NaN and infinities, reads that cover no site, one site, and two sites at their first and last event"""
    rng = np.random.default_rng(1811)
    pos = np.unique(np.concatenate((rng.choice(200, 70, replace=False), [100, 110, 111, 150, 160])))
    pos = pos[(pos < 151) | (pos > 159)]
    key = np.array([_key(cs, p) for cs in (0, 1, 2) for p in pos], np.int64)
    values = np.array([3.0, -3.0, THR, -THR, 1.25, -0.5, np.nan, 0.0, -0.0, np.inf, -np.inf, 40.0, -7.5, 1e300])
    reads = []
    for _ in range(400):
        n = int(rng.integers(1, 61))
        reads.append((int(rng.integers(0, 3)), int(rng.integers(0, 215 - n)), values[rng.integers(0, len(values), n)]))
    reads.append((0, 300, np.full(30, 3.0)))                                  # covers no site
    reads.append((1, 152, np.full(9, 3.0)))                                   # 152 .. 160: one site only
    reads.append((0, 150, np.array([1.0] + [0.0] * 9 + [-2.0])))              # 150 .. 160: two sites, at the first and the last event
    reads.append((1, 150, np.array([1.0] + [0.0] * 9 + [-2.0])))              # the same on '-': event 0 lies at 160
    reads.append((2, 150, np.array([np.nan] + [0.0] * 9 + [-2.0])))           # an invalid score at one of the two: no row
    c = _case(reads, key, 10)
    c['want'] = _rows_ref(c)
    return c


def test_rows_on_constructed_reads(det, mixed):
    want = mixed['want']
    got = _rows_device(det, mixed)
    _same_rows(got, want)
    assert want['prow_off'][-1] > 2000 and (np.diff(want['prow_off']) == 0).any()
    j = int(np.flatnonzero((mixed['key'] == _key(0, 150)))[0])
    idx = int(mixed['poff'][j])                                               # (150, 160) on cs 0: 160 is 150's next site
    sl = slice(int(want['prow_off'][idx]), int(want['prow_off'][idx + 1]))
    n = len(mixed['cs'])
    assert (n - 3) in want['read'][sl].tolist() and want['sa'][sl][want['read'][sl] == n - 3].tolist() == [1.0]
    j1 = int(mixed['poff'][int(np.flatnonzero((mixed['key'] == _key(1, 150)))[0])])
    sl1 = slice(int(want['prow_off'][j1]), int(want['prow_off'][j1 + 1]))
    assert want['sa'][sl1][want['read'][sl1] == n - 2].tolist() == [-2.0]     # '-': event 0 lies at 160, the last event at 150
    j2 = int(mixed['poff'][int(np.flatnonzero((mixed['key'] == _key(2, 150)))[0])])
    assert (n - 1) not in want['read'][int(want['prow_off'][j2]):int(want['prow_off'][j2 + 1])].tolist()
    for j in range(len(want['prow_off']) - 1):                                # within a pair the rows are in ascending read index
        r = got['read'][int(got['prow_off'][j]):int(got['prow_off'][j + 1])]
        assert np.all(np.diff(r) > 0), j
    assert np.all(np.abs(got['sa']) <= K.DBL_MAX) and np.all(np.abs(got['sb']) <= K.DBL_MAX)


def test_rows_two_runs_and_both_memspaces_give_identical_bytes(det, mixed):
    first, second = _rows_device(det, mixed), _rows_device(det, mixed)
    host = _engine().pair_rows_host(*[mixed[f] for f in ('cs', 'start', 'roff', 'score', 'key', 'poff')])
    for f in ROW_FIELDS:
        assert same(first[f], second[f]) and same(first[f], host[f]), f


def test_rows_beyond_thr_are_k16s_table(det, mixed):
    """for every pair the rows whose two scores are both beyond +-thr are the reads K16 counts: N, and the four cells.  (K16 calls an
    infinite score, which is no VALID one here: its table is taken over the scores with the infinities set to NaN.)"""
    import torch
    got = _rows_device(det, mixed)
    t = {f: torch.from_numpy(mixed[f]).cuda() for f in ('cs', 'start', 'roff', 'score', 'key', 'poff')}
    t['score'] = torch.from_numpy(np.where(np.isinf(mixed['score']), np.nan, mixed['score'])).cuda()
    counts = det.site_pairs(t['cs'], t['start'], t['roff'], t['score'], t['key'], t['poff'], int(mixed['poff'][-1]), thr=THR,
                            want=('counts',))['counts'].cpu().numpy().reshape(-1, 4)
    called = (np.abs(got['sa']) >= THR) & (np.abs(got['sb']) >= THR)
    pair_of = np.repeat(np.arange(len(got['prow_off']) - 1), np.diff(got['prow_off']))
    assert same(np.bincount(pair_of[called], minlength=len(counts)).astype(np.int64), counts.sum(1).astype(np.int64)) and counts.sum() > 1000
    cell = 2 * (got['sa'] >= THR) + (got['sb'] >= THR)
    assert same(np.bincount(4 * pair_of[called] + cell[called], minlength=counts.size).astype(np.int32), counts.ravel())


def test_rows_of_a_workgroup_class_read_with_partners_across_windows(det):
    """reads beyond NMOD_CALLS_WAVE_MAX events, '+' and '-', every position a candidate site (far more than the 256 of a staged
    window) and max_dist beyond a window: a site's partners lie in the next window and the one after"""
    rng = np.random.default_rng(1814)
    n = L.CALLS_WAVE_MAX + 150
    key = np.array([_key(cs, p) for cs in (0, 1) for p in range(n + 40)], np.int64)
    reads = [(0, 7, np.where(rng.random(n) < 0.1, rng.normal(size=n), np.nan)),
             (1, 33, np.where(rng.random(n) < 0.1, rng.normal(size=n), np.inf)),
             (1, 0, np.where(rng.random(500) < 0.3, 1.5, np.nan))]              # a read of the wave class over the same pairs
    c = _case(reads, key, 300)
    want = _rows_ref(c)
    got = _rows_device(det, c)
    _same_rows(got, want)
    pair_of = np.repeat(np.arange(len(got['prow_off']) - 1), np.diff(got['prow_off']))
    far = pair_of - np.repeat(c['poff'][:-1], np.diff(c['poff']))[pair_of] >= 256
    assert c['poff'][-1] > 10 ** 6 and far.sum() > 500 and (np.diff(got['prow_off']) == 2).any()


def test_rows_of_more_short_reads_than_the_grid_has_waves(det):
    rng = np.random.default_rng(1815)
    key = np.array([_key(cs, p) for cs in (0, 1) for p in range(0, 400, 2)], np.int64)
    reads = [(int(rng.integers(0, 2)), int(rng.integers(0, 380)), rng.choice([3.0, -1.0, 0.5, np.nan], int(rng.integers(15, 26)))) for _ in range(20000)]
    c = _case(reads, key, 6)
    want = _rows_ref(c)
    got = _rows_device(det, c)
    _same_rows(got, want)
    assert want['prow_off'][-1] > 200000 and np.diff(want['prow_off']).max() > 100


# ------------------------------------------------------------------------------------------------------------ the row kernel
def _stoich_margins(sa, sb, off, **iteration):
    """nmod_site_stoich's pi over the two rows of every pair under the same max_iter and tol, a read that is not valid at both sites
    masked out of both"""
    both = (np.abs(sa) <= K.DBL_MAX) & (np.abs(sb) <= K.DBL_MAX)
    eng = _engine()
    return [eng.site_stoich_host(np.where(both, s, np.nan), off, min_valid=1, **iteration)['pi'] for s in (sa, sb)]


def _check_pairs(got, sa, sb, off, converged=True, **opts):
    """status and n_valid exactly, the NaN pattern, iters 0 wherever no root of D is searched for; pa and pb: nmod_site_stoich's
    bits on the same rows; the other doubles within the restatement's gates at those margins (exactly where the gate is 0)"""
    pa, pb = _stoich_margins(sa, sb, off, **{k: v for k, v in opts.items() if k in ('max_iter', 'tol')})
    exp = K.pair_linkage(sa, sb, off, margins=(got['pa'], got['pb']), **opts)
    worst = {}
    for i, e in enumerate(exp):
        assert int(got['status'][i]) == e['status'] and int(got['n_valid'][i]) == e['n_valid'], (i, got['status'][i], e['status'], got['n_valid'][i], e['n_valid'])
        if e['status'] & (K.TOO_FEW | K.FLAT | K.TOO_LARGE):
            assert all(np.isnan(got[f][i]) for f in K.FIELDS) and got['iters'][i] == 0, i
            continue
        assert same(got['pa'][i], pa[i]) and same(got['pb'][i], pb[i]), (i, got['pa'][i], pa[i], got['pb'][i], pb[i])
        if e['status'] & K.DEGENERATE:
            assert [got[f][i] for f in ('d', 'd_lo', 'd_hi', 'stat', 'p_indep')] == [0.0, 0.0, 0.0, 0.0, 1.0] and np.isnan(got['r'][i]) and got['iters'][i] == 0, i
            continue
        assert not any(np.isnan(got[f][i]) for f in K.FIELDS), i
        assert got['d_lo'][i] <= got['d'][i] <= got['d_hi'][i], i
        if e['status'] & (K.AT_MIN | K.AT_MAX):
            assert got['iters'][i] == 0 and got['d'][i] == e['d'], i
        if not converged:
            continue
        g = e['gates']
        for f in ('d', 'd_lo', 'd_hi', 'r', 'stat'):
            _share(f, abs(got[f][i] - e[f]), g[f], worst)
        lo, hi = g['p_indep']
        assert lo <= got['p_indep'][i] <= hi, (i, lo, got['p_indep'][i], hi)
    print('worst deviation as a share of its gate: %s' % (', '.join('%s %.3g' % kv for kv in sorted(worst.items())) or 'none compared'))
    assert all(v <= 1.0 for v in worst.values()), worst
    return exp


def test_parity_over_the_row_lengths():
    """two pairs of each length: 1, min_reads - 1, min_reads, NMOD_LINK_SMALL - 1, NMOD_LINK_SMALL, NMOD_LINK_SMALL + 1, NMOD_LINK_WAVE,
    NMOD_LINK_WAVE + 1, and the staged limits of the workgroup form and one read past each"""
    sa, sb, off = K.parity_batch()
    lens = set(np.diff(off).tolist())
    assert {1, K.MIN_READS - 1, K.MIN_READS, L.LINK_SMALL - 1, L.LINK_SMALL, L.LINK_SMALL + 1, L.LINK_WAVE, L.LINK_WAVE + 1} <= lens
    assert (L.LINK_SMALL, L.LINK_WAVE) == (K.SMALL, K.WAVE) == (L.STOICH_SMALL, L.STOICH_WAVE)
    got = _engine().pair_linkage_host(sa, sb, off, min_reads=K.MIN_READS)
    exp = _check_pairs(got, sa, sb, off, min_reads=K.MIN_READS)
    assert [e['status'] for e in exp[:4]] == [K.TOO_FEW] * 4 and sum(e['status'] == 0 for e in exp) >= 16


def test_every_status_bit_on_planted_rows():
    sa, sb, off, names = K.planted_batch()
    got = _engine().pair_linkage_host(sa, sb, off)
    exp = _check_pairs(got, sa, sb, off)
    st = dict(zip(names, (e['status'] for e in exp)))
    assert st['too_few'] == st['invalid_mix'] == st['too_few_by_invalid'] == K.TOO_FEW and st['flat_a'] == st['flat_b'] == K.FLAT
    assert st['degenerate_a0'] == st['degenerate_b1'] == K.DEGENERATE and st['at_max'] == K.AT_MAX and st['at_min'] == K.AT_MIN
    assert st['plain'] == st['wave_invalid'] == st['block_invalid'] == st['perfect_calls'] == 0
    # max_iter = 1: every root that is searched for stops unconverged, and says so
    one = _engine().pair_linkage_host(sa, sb, off, max_iter=1)
    exp1 = _check_pairs(one, sa, sb, off, converged=False, max_iter=1)
    assert sum(bool(e['status'] & K.NOT_CONVERGED) for e in exp1) >= 5 and all(one['iters'][i] <= 1 for i in range(len(exp1)))
    # a row beyond NMOD_MAX_DEEP reads (by its offsets alone; device memory, where nothing of it is read)
    import torch
    det = _engine().DeviceDetector(0)
    big = det.pair_linkage(torch.zeros(8, dtype=torch.float64, device='cuda'), torch.zeros(8, dtype=torch.float64, device='cuda'),
                           torch.tensor([0, L.MAX_DEEP + 1], dtype=torch.int64, device='cuda'))
    assert int(big['status'][0]) == K.TOO_LARGE and int(big['n_valid'][0]) == 0 and bool(torch.isnan(big['d'][0]))


def _raw(sa, sb, off, fields, **opts):
    """nmod_pair_linkage through ctypes with the outputs named in `fields` alone"""
    import ctypes as C
    lib = L.load()
    o = dict(K.DEFAULTS, **opts)
    shapes = _engine()._link_shapes(len(off) - 1)
    res = {f: np.zeros(shapes[f][1], np.dtype(shapes[f][0])) for f in fields}
    out = L.make_link_out(**{f: a.ctypes.data for f, a in res.items()})
    prm = L.make_params(memspace=L.MEM_HOST, dtype=L.DTYPE_F64)
    assert lib.nmod_pair_linkage(C.byref(prm), len(off) - 1, sa.ctypes.data, sb.ctypes.data, off.ctypes.data,
                                 C.byref(L.make_link_opts(o['max_iter'], o['min_reads'], o['tol'], o['ci_drop'])), C.byref(out)) == 0
    return res


def _pool():
    sa, sb, off, _ = K.planted_batch()
    pa, pb, poff = K.parity_batch()
    rows = [(sa[off[i]:off[i + 1]], sb[off[i]:off[i + 1]]) for i in range(len(off) - 1)]
    rows += [(pa[poff[i]:poff[i + 1]], pb[poff[i]:poff[i + 1]]) for i in range(len(poff) - 1) if poff[i + 1] - poff[i] <= K.WAVE + 1]
    return rows


def test_a_pairs_bits_depend_on_its_row_alone(det):
    """the same rows in a permuted batch, from device memory, through the engine's two layers, and with fewer outputs: the same bits;
    without d_lo and d_hi the other outputs keep theirs"""
    import torch
    rows = _pool()
    sa, sb, off = K._csr(rows)
    full = _raw(sa, sb, off, ALL)
    perm = np.random.default_rng(1806).permutation(len(rows))
    sa2, sb2, off2 = K._csr([rows[j] for j in perm])
    shuf = _raw(sa2, sb2, off2, ALL)
    for f in ALL:
        assert same(shuf[f], full[f][perm]), f
    for fields in (('d',), ('d_lo', 'd_hi'), ('pa', 'pb', 'status'), ('stat', 'p_indep', 'r'), ('iters', 'n_valid'),
                   tuple(f for f in ALL if f not in ('d_lo', 'd_hi'))):
        part = _raw(sa, sb, off, fields)
        assert all(same(part[f], full[f]) for f in fields), fields
    host = _engine().pair_linkage_host(sa, sb, off)
    dev = det.pair_linkage(torch.from_numpy(sa).cuda(), torch.from_numpy(sb).cuda(), torch.from_numpy(off).cuda())
    no_ci = det.pair_linkage(torch.from_numpy(sa).cuda(), torch.from_numpy(sb).cuda(), torch.from_numpy(off).cuda(), interval=False)
    assert set(no_ci) == set(ALL) - {'d_lo', 'd_hi'}
    for f in ALL:
        assert same(host[f], full[f]) and same(dev[f].cpu().numpy(), full[f]), f
        assert f in ('d_lo', 'd_hi') or same(no_ci[f].cpu().numpy(), full[f]), f


def test_more_pairs_than_each_persistent_grid_has_groups():
    """every class on a batch beyond its grid (the counts as tests/test_persistent_grids_gpu.py takes them: grid_cases.stoich_units,
    K14's launches, which are this kernel's): every repeat of a pool row has the bits of its first copy, and the first copies are
    checked against the restatement"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(1807)
    pools = [[K.simulate_pair(rng, n, 2.0, 0.3, 0.4, 0.05) for _ in range(4)] for n in (30, 300, K.WAVE + 76)]
    rows, ident = [], []
    for c, (pool, units) in enumerate(zip(pools, G.stoich_units(cus))):
        for k in range(units + 37):
            rows.append(pool[k % 4])
            ident.append(4 * c + k % 4)
    order = rng.permutation(len(rows))
    rows, ident = [rows[j] for j in order], np.array(ident)[order]
    sa, sb, off = K._csr(rows)
    lens = np.diff(off)
    for n, units in zip((30, 300, K.WAVE + 76), G.stoich_units(cus)):
        assert (lens == n).sum() > units
    got = _engine().pair_linkage_host(sa, sb, off)
    firsts = np.array([int(np.flatnonzero(ident == v)[0]) for v in range(12)])
    for f in ALL:
        assert same(got[f], got[f][firsts][ident]), f
    sub = K._csr([rows[i] for i in firsts])
    _check_pairs({f: got[f][firsts] for f in ALL}, *sub)


def test_side_stream_and_no_wait_for_the_work_before_it(det):
    """tests/stream_cases.py's method: on a side stream the default stream's result; behind a stall on a fresh stream, the inputs put
    in place behind the stall and a decoy behind the call, the call returns while the stall runs and gives the real inputs' result"""
    import torch
    sa, sb, off = K._csr(_pool())
    want = _engine().pair_linkage_host(sa, sb, off)
    sw = S.Swapped(dict(sa=sa, sb=sb), dict(sa=-sb, sb=sa[::-1].copy()))
    d_off = torch.from_numpy(off).cuda()
    call = lambda out=None: det.pair_linkage(sw.t['sa'], sw.t['sb'], d_off, out=out)
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
    sites = (np.array(['chrT'] * 6), np.array(['+'] * 3 + ['-'] * 3), np.array(list(planted) * 2))
    return dict(reads=reads, model=model, alt=alt, planted=planted, sites=sites)


def test_end_to_end_through_cooccur_reads_llr(chain):
    from nanomod_amd import readllr
    hard_lines, soft_lines = [], []
    kw = dict(sites=chain['sites'], max_dist=40, thr=THR, min_reads=10, fdr='bh')
    hard = readllr.cooccur_reads_llr(chain['reads'], chain['model'], chain['alt'], log=hard_lines.append, **kw)
    soft = readllr.cooccur_reads_llr(chain['reads'], chain['model'], chain['alt'], log=soft_lines.append, soft=True, **kw)
    # without the option nothing changes: the same entries with the same bytes, the same line
    assert len(hard_lines) == 1 and soft_lines[0] == hard_lines[0] and len(soft_lines) == 2 and soft_lines[1].startswith('readpairs: soft linkage of 6 pair(s)')
    assert set(soft) - set(hard) == {'n_cov', 'pa', 'pb', 'd', 'd_lo', 'd_hi', 'r', 'pi11', 'pi10', 'pi01', 'pi00', 'stat', 'p_indep', 'link_status',
                                     'q_indep'}
    for f in hard:
        assert same(np.asarray(soft[f]), np.asarray(hard[f])), f
    # every read covers the planted sites with a finite sum: all of them take part, far more than K16's called reads
    n_called = soft['n11'] + soft['n10'] + soft['n01'] + soft['n00']
    assert np.all(soft['n_cov'] >= n_called) and np.all((soft['link_status'] & (L.LINK_NO_ESTIMATE | L.LINK_NOT_CONVERGED | L.LINK_DEGENERATE)) == 0)
    assert soft['n_cov'].min() >= 20
    cells = np.stack([soft[f] for f in ('pi11', 'pi10', 'pi01', 'pi00')])
    assert np.allclose(cells.sum(0), 1.0, atol=1e-12) and cells.min() > -1e-12
    assert np.all(soft['d_lo'] <= soft['d']) and np.all(soft['d'] <= soft['d_hi'])
    # the planted verdict of K16's chain: (A, B) go together on both strands, (A, C) do not
    for ab, ac in ((0, 1), (3, 4)):
        assert soft['d'][ab] > 0.0 and soft['r'][ab] > 0.3 and soft['p_indep'][ab] < 0.05 / 6 < soft['p_indep'][ac]
        assert soft['d_lo'][ab] > 0.0 and soft['d_lo'][ac] < 0.0 < soft['d_hi'][ac]
    want_q, _ = _engine().fdr_adjust_host(soft['p_indep'], 'bh')
    assert same(soft['q_indep'], want_q[0])


def test_the_command_line_writes_the_same_rows(chain):
    from nanomod_amd import cli, container, kmermodel, readllr
    reads = chain['reads']
    with tempfile.TemporaryDirectory() as tmp:
        r_path, m_path, a_path, s_path, out, out0 = (os.path.join(tmp, n) for n in ('reads.npz', 'model.npz', 'alt.npz', 'sites.txt', 'cli', 'cli0'))
        container.save_reads(r_path, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
        zeros = np.zeros(64, np.int64)
        for path, m in ((m_path, chain['model']), (a_path, chain['alt'])):
            kmermodel.save_kmer_model(path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                                 n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
        open(s_path, 'w').writelines('%s %s %d\n' % (c, s, p + 1) for c, s, p in zip(*chain['sites']))
        argv = ['readpairs', '--wrkBase1', r_path, '--kmerModel', m_path, '--altModel', a_path, '--sites', s_path, '--maxDist', '40', '--fdr', 'by',
                '--FileID', 'run', '--outLevel', '3']
        assert cli.main(argv + ['--outFolder', out, '--soft', '1', '--ciLevel', '0.9']) == 0
        assert cli.main(argv + ['--outFolder', out0]) == 0
        pairs = readllr.cooccur_reads_llr(reads, kmermodel.load_kmer_model(m_path), kmermodel.load_kmer_model(a_path), sites=chain['sites'], max_dist=40,
                                          fdr='by', soft=True, ci_level=0.9, log=lambda *a: None)
        readllr.write_site_linkage(os.path.join(tmp, 'want.txt'), pairs)
        text = open(os.path.join(out, 'run_site_linkage.txt')).read()
        assert text == open(os.path.join(tmp, 'want.txt')).read()
        rows = [ln.split() for ln in text.splitlines()]
        assert len(rows) == 6 and all(len(r) == 20 for r in rows) and [int(r[5]) for r in rows] == pairs['n_cov'].tolist()
        # without the option: no linkage file, and the pairs file of either run is the same
        assert os.listdir(out0) == ['run_site_pairs.txt']
        assert open(os.path.join(out0, 'run_site_pairs.txt')).read() == open(os.path.join(out, 'run_site_pairs.txt')).read()
