"""GPU: nmod_read_sites_count / nmod_read_hmm (K19) against tests/hmm_ref.py: the entries as exact integers, post, ll and ll_indep within
the derived gates, states, runs and site counts consistent with the device's own post and equal to the reference's wherever the reference
is clear of the thresholds; the seams of the scan; extremes against mpmath; invariances as identical bytes; the stream contract; the
refusals; the chain K13 -> K19 through readllr.smooth_reads_llr and `cli readhmm`."""
import ctypes as C
import math
import os
import tempfile

import numpy as np
import pytest

import hmm_ref as H
import read_batch_cases as RB
import readllr_ref as RF
import stream_cases as S
from nanomod_amd import _lib as L
from test_engine_device_args_gpu import same
from test_site_pairs import _key

pytestmark = pytest.mark.gpu

PI, LENGTH, CALL_POST = 0.3, 30.0, 0.9
ENTRY, READ, SITE = L.HMM_ENTRY_FIELDS, L.HMM_READ_FIELDS, L.HMM_SITE_FIELDS
ALL = ENTRY + READ + SITE
TILE_WAVE, TILE_GROUP = 64 * L.HMM_CHUNK, 256 * L.HMM_CHUNK


def _engine():
    from nanomod_amd import engine
    return engine


@pytest.fixture(scope='module')
def det():
    return _engine().DeviceDetector(0)


def _case(reads, key):
    """reads: (cs, start, scores) triples; the flat arrays of the entries"""
    cs = np.array([r[0] for r in reads], np.int32)
    start = np.array([r[1] for r in reads], np.int64)
    roff = np.zeros(len(reads) + 1, np.int64)
    roff[1:] = np.cumsum([len(r[2]) for r in reads])
    score = np.concatenate([np.asarray(r[2], np.float64) for r in reads]) if reads else np.zeros(0)
    return dict(cs=cs, start=start, roff=roff, score=score, key=np.asarray(key, np.int64))


def _device(det, c, pi=PI, length=LENGTH, call_post=CALL_POST, **kw):
    """read_sites and read_hmm on device tensors of case c -> the results as numpy, hoff among them"""
    import torch
    t = {f: torch.from_numpy(c[f]).cuda() for f in ('cs', 'start', 'roff', 'score', 'key')}
    hoff, nrows = det.read_sites(t['cs'], t['start'], t['roff'], t['score'], t['key'])
    res = det.read_hmm(t['cs'], t['start'], t['roff'], t['score'], t['key'], hoff, nrows, pi=pi, length=length, call_post=call_post, **kw)
    return dict({f: v.cpu().numpy() for f, v in res.items()}, hoff=hoff.cpu().numpy())


def _ref(c, pi=PI, length=LENGTH, call_post=CALL_POST):
    return H.read_hmm_ref(c['cs'], c['start'], c['roff'], c['score'], c['key'], pi, length, call_post)


def _check(res, ref, call_post=CALL_POST):
    """the device's results against the restatement's; returns the share of the entries whose reference posterior lies within its gate of
    a threshold (their states are the device's to decide) and the largest relative errors of post and ll"""
    assert same(res['hoff'], ref['hoff']) and same(res['site'], ref['site'])
    ok = H.post_within(res['post'], ref['post'], ref['gate'])
    assert np.all(ok), (np.flatnonzero(~ok)[:5], res['post'][~ok][:5], ref['post'][~ok][:5])
    g_read = np.array([H.gate(int(m)) if m else 0.0 for m in np.diff(ref['hoff'])])
    for f in ('ll', 'll_indep'):
        ok = H.ll_within(res[f], ref[f], g_read, ref['denom'])
        assert np.all(ok), (f, np.flatnonzero(~ok)[:5], res[f][~ok][:5], ref[f][~ok][:5])
    assert same(res['status'], ref['status']) and same(res['n_sites'], ref['n_sites'])
    # the hard outputs are those of the post that was written
    state = H.states(res['post'], call_post)
    assert same(res['state'], state)
    own = dict(H.per_read(res['hoff'], state), **H.per_site(res['site'], state, len(ref['site_n'])))
    for f in ('n_mod', 'n_can', 'n_runs') + SITE:
        assert same(res[f], own[f]), f
    clear = H.band_margin(ref['post'], call_post, ref['gate'])
    assert same(res['state'][clear], ref['state'][clear])
    if clear.all():
        for f in ('n_mod', 'n_can', 'n_runs') + SITE:
            assert same(res[f], ref[f]), f
    big = ref['post'] > 1e-280
    rel = float(np.max(np.abs(res['post'][big] - ref['post'][big]) / ref['post'][big])) if big.any() else 0.0
    rel_ll = float(np.max(np.abs(res['ll'] - ref['ll']) / (ref['denom'] + 1.0))) if len(ref['ll']) else 0.0
    print('largest relative error: post %.3g, ll %.3g (over %d entries)' % (rel, rel_ll, len(ref['post'])))
    return 1.0 - float(clear.mean()) if len(clear) else 0.0


# ------------------------------------------------------------------------------------------------------------ constructed reads
@pytest.fixture(scope='module')
def mixed():
    """Three (chrom, strand) ids with the same site positions, reads of 1 .. 60 events on all of them with scores at and around K13's
    threshold, 0, NaN and infinities; reads that cover no site, exactly one site, and sites at their first and last event on '+' and '-'"""
    rng = np.random.default_rng(1911)
    pos = np.unique(np.concatenate((rng.choice(200, 70, replace=False), [100, 110, 111, 150, 160])))
    pos = pos[(pos < 151) | (pos > 159)]
    key = np.array([_key(cs, p) for cs in (0, 1, 2) for p in pos], np.int64)
    values = np.array([3.0, -3.0, 2.5, -2.5, 1.0, -0.5, np.nan, 0.0, np.inf, -np.inf, 40.0, -7.5])
    reads = []
    for _ in range(400):
        n = int(rng.integers(1, 61))
        reads.append((int(rng.integers(0, 3)), int(rng.integers(0, 215 - n)), values[rng.integers(0, len(values), n)]))
    reads.append((0, 300, np.full(30, 3.0)))                                  # covers no site
    reads.append((1, 151, np.full(9, 3.0)))                                   # 151 .. 159: none either
    reads.append((1, 152, np.full(9, 3.0)))                                   # 152 .. 160: one site, at its first event ('-')
    reads.append((0, 152, np.full(9, -3.0)))                                  # the same on '+': at its last event
    reads.append((0, 150, np.array([3.0] + [0.0] * 9 + [-3.0])))              # 150 .. 160: two sites, at the first and the last event
    reads.append((1, 150, np.array([3.0] + [0.0] * 9 + [-3.0])))              # the same on '-': event 0 lies at 160
    reads.append((2, 100, np.array([2.5] + [np.nan] * 9 + [-2.5, np.nan])))   # 110 valid, 111 not: the chain ends at 110
    reads.append((2, 100, np.zeros(12)))                                      # every score 0: the likelihood is 1
    c = _case(reads, key)
    c['ref'] = _ref(c)
    return c


def test_entries_posteriors_and_counts_on_constructed_reads(det, mixed):
    res = _device(det, mixed)
    ref = mixed['ref']
    assert set(res) == set(ALL) | {'hoff'} and len(ref['post']) > 2000
    excluded = _check(res, ref)
    assert excluded == 0.0                                                    # call_post and the score grid leave no reference entry in the band
    m = np.diff(ref['hoff'])
    assert m[-8:-1].tolist() == [0, 0, 1, 1, 2, 2, 2] and m[-1] >= 3 and (m == 0).sum() > 8 and m.max() >= 20
    assert ref['status'][-8:].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and np.all(res['ll'][m == 0] == 0.0) and np.all(res['ll_indep'][m == 0] == 0.0)
    a, b = ref['hoff'][-5], ref['hoff'][-4]
    assert mixed['key'][res['site'][a:b]].tolist() == [_key(0, 150), _key(0, 160)] and res['post'][a] > 0.5 > res['post'][a + 1]
    a, b = ref['hoff'][-4], ref['hoff'][-3]                                   # '-': the score of event 0 belongs to 160
    assert mixed['key'][res['site'][a:b]].tolist() == [_key(1, 150), _key(1, 160)] and res['post'][a] < 0.5 < res['post'][a + 1]
    assert len(set(res['state'].tolist())) == 3 and res['n_runs'].max() >= 2 and res['site_n'].sum() == len(ref['post'])


def test_host_and_device_memspace_and_fewer_outputs_give_identical_bytes(det, mixed):
    dev = _device(det, mixed)
    eng = _engine()
    args = [mixed[f] for f in ('cs', 'start', 'roff', 'score', 'key')]
    hoff = eng.read_sites_host(*args)
    assert same(hoff, dev['hoff'])
    host = eng.read_hmm_host(*args, hoff, pi=PI, length=LENGTH, call_post=CALL_POST)
    for f in ALL:
        assert same(host[f], dev[f]), f
    for want in (('ll',), ('post',), ('ll', 'll_indep', 'n_sites', 'status'), ('state', 'site_mod'), ('n_runs', 'site_n', 'site'), ('n_mod', 'n_can', 'site_can')):
        part = _device(det, mixed, want=want)
        assert set(part) == set(want) | {'hoff'}
        for f in want:
            assert same(part[f], dev[f]), (want, f)


def _per_read_rows(res, order):
    """the per-entry tracks of `res` with the reads taken in `order`"""
    hoff = res['hoff']
    rows = np.concatenate([np.arange(hoff[r], hoff[r + 1]) for r in order]) if len(order) else np.zeros(0, np.int64)
    return {f: res[f][rows] for f in ENTRY}


def test_a_permutation_of_the_reads_and_a_read_alone_change_nothing(det, mixed):
    dev = _device(det, mixed)
    n = len(mixed['cs'])
    order = np.random.default_rng(1912).permutation(n)
    reads = [(mixed['cs'][r], mixed['start'][r], mixed['score'][mixed['roff'][r]:mixed['roff'][r + 1]]) for r in range(n)]
    perm = _device(det, _case([reads[r] for r in order], mixed['key']))
    want = _per_read_rows(dev, order)
    for f in ENTRY:
        assert same(perm[f], want[f]), f
    for f in READ:
        assert same(perm[f], dev[f][order]), f
    for f in SITE:
        assert same(perm[f], dev[f]), f
    longest = int(np.argmax(np.diff(dev['hoff'])))
    for r in (longest, n - 4, 7):
        alone = _device(det, _case([reads[r]], mixed['key']))
        for f in ENTRY:
            assert same(alone[f], dev[f][dev['hoff'][r]:dev['hoff'][r + 1]]), (r, f)
        for f in READ:
            assert same(alone[f], dev[f][r:r + 1]), (r, f)


# ------------------------------------------------------------------------------------------------------------ the seams of the scan
SEAM_M = sorted({1, 2, 63, 64, 65, 127, 128, 129, TILE_WAVE - 1, TILE_WAVE, TILE_WAVE + 1, L.HMM_WAVE_MAX - 1, L.HMM_WAVE_MAX, L.HMM_WAVE_MAX + 1,
                 2 * TILE_GROUP + 301})


def _seam_runs(m):
    """the planted run of a read of m entries, across the largest boundary of the scan it has — a tile of either form, a wave, a lane's
    chunk — as counted from the read's first entry (the forward pass) and from its last (the backward pass)"""
    if m < 8:
        return [(0, m - 1)]
    b = next(b for b in (TILE_GROUP, TILE_WAVE, 64, L.HMM_CHUNK) if b + 3 < m)
    return [(b - 3, b + 2), (m - 1 - (b + 2), m - 1 - (b - 3))]


def test_a_planted_run_across_every_seam_of_the_scan(det):
    """every position a candidate site, so a read of m events has m entries; scores -6 with one run of +6"""
    top = max(SEAM_M)
    key = np.array([_key(1, p) for p in range(top + 5)], np.int64)
    reads, planted = [], []
    for m in SEAM_M:
        for first, last in _seam_runs(m):
            reads.append((1, 3, H.planted_run(m, first, last)[::-1].copy()))   # '-': event i lies at start + m - 1 - i
            planted.append((first, last))
    c = _case(reads, key)
    res = _device(det, c, length=20.0)
    ref = _ref(c, length=20.0)
    assert np.diff(ref['hoff']).tolist() == [m for m in SEAM_M for _ in _seam_runs(m)]
    assert _check(res, ref) == 0.0
    assert np.all(res['n_runs'] == 1) and np.all(ref['n_runs'] == 1)
    for r, (first, last) in enumerate(planted):
        st = res['state'][res['hoff'][r]:res['hoff'][r + 1]]
        got = H.runs(st)
        assert (int(got[0][0]), int(got[1][0])) == (first, last) or len(st) < 8, (r, got, first, last)
        assert same(st, ref['state'][ref['hoff'][r]:ref['hoff'][r + 1]])


def test_more_reads_than_either_grid_has_units(det):
    """in read_batch_cases' manner: a batch whose reads are copies of a few distinct reads, more of them than the persistent grids of
    either form have waves (workgroups), has the distinct reads' outputs, gathered; the site counts are their sums"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(1913)
    top = L.HMM_WAVE_MAX + 77
    key = np.array([_key(0, p) for p in range(0, 2 * top, 2)], np.int64)      # every second position
    distinct = [(0, int(rng.integers(0, 40)), rng.normal(0.0, 3.0, int(rng.integers(5, 60)))) for _ in range(23)]
    single = _device(det, _case(distinct, key))
    idx = rng.integers(0, len(distinct), RB.short_units(cus) + 1500)
    batch = _device(det, _case([distinct[i] for i in idx], key))
    assert len(idx) > RB.short_units(cus)
    want = _per_read_rows(single, idx)
    for f in ENTRY:
        assert same(batch[f], want[f]), f
    for f in READ:
        assert same(batch[f], single[f][idx]), f
    for f in SITE:
        per = np.stack([H.per_site(single['site'][single['hoff'][r]:single['hoff'][r + 1]], single['state'][single['hoff'][r]:single['hoff'][r + 1]],
                                   len(key))[f] for r in range(len(distinct))])
        assert same(batch[f], (per * np.bincount(idx, minlength=len(distinct))[:, None]).sum(0).astype(np.int32)), f
    long_read = (0, 0, rng.normal(0.0, 3.0, 2 * top - 1))                      # top entries: the workgroup form
    one = _device(det, _case([long_read], key))
    assert one['n_sites'].tolist() == [top]
    many = RB.long_units(cus) + 50
    rep = _device(det, _case([long_read] * many, key), want=('post', 'state', 'n_runs', 'll', 'site_mod'))
    assert same(rep['post'], np.tile(one['post'], many)) and same(rep['state'], np.tile(one['state'], many))
    assert same(rep['ll'], np.repeat(one['ll'], many)) and same(rep['n_runs'], np.repeat(one['n_runs'], many)) and same(rep['site_mod'], one['site_mod'] * many)


# ------------------------------------------------------------------------------------------------------------ extremes
@pytest.mark.parametrize('pi,length', [(0.3, 1e6), (1e-9, 1e6), (1.0 - 1e-9, 200.0), (0.5, 1e-3), (1e-9, 1e9)])
def test_extremes_against_mpmath(det, pi, length):
    """+-800 next to each other at distance 1, the ends of pi's range, a gap of 60 000 bases (rho underflows to 0 at the shorter lengths)"""
    import mpmath as mp
    key = np.array([_key(0, p) for p in (10, 11, 12, 13, 60013, 60014, 60015)], np.int64)
    scores = np.full(60010, np.nan)
    scores[[0, 1, 2, 3, 60003, 60004, 60005]] = 800.0, -800.0, 800.0, -800.0, 5.0, -5.0, 40.0
    c = _case([(0, 10, scores), (0, 10, scores[:4]), (0, 11, -scores[1:6])], key)
    res = _device(det, c, pi=pi, length=length)
    ref = _ref(c, pi, length)
    assert same(res['hoff'], ref['hoff']) and ref['hoff'].tolist() == [0, 7, 11, 14] and same(res['site'], ref['site'])
    worst = 0.0
    for r in range(3):
        a, b = int(ref['hoff'][r]), int(ref['hoff'][r + 1])
        exact = H.hmm_mp(ref['x'][a:b], ref['s'][a:b], pi, length)
        g = H.gate(b - a)
        with mp.workdps(60):
            for j in range(b - a):
                got = float(res['post'][a + j])
                assert math.isfinite(got) and abs(mp.mpf(got) - exact['post'][j]) <= g * exact['post'][j] + mp.mpf(H.FLOOR), (r, j, got, float(exact['post'][j]))
                if exact['post'][j] > 1e-280:
                    worst = max(worst, float(abs(mp.mpf(got) - exact['post'][j]) / exact['post'][j]))
            for f in ('ll', 'll_indep'):
                got = float(res[f][r])
                assert math.isfinite(got) and abs(mp.mpf(got) - exact[f]) <= g * (exact['denom'] + 1), (r, f, got, float(exact[f]))
    print('largest relative error of post against mpmath: %.3g' % worst)
    assert same(res['state'], H.states(res['post'], CALL_POST))


# ------------------------------------------------------------------------------------------------------------ the stream
def test_side_stream_and_no_wait_for_the_work_before_it(det, mixed):
    """On a side stream the result is the default stream's; and behind a stall of stream_cases.T_MS on a fresh stream (the inputs put in
    place behind the stall, a decoy behind the call: tests/stream_cases.py) the call returns while the stall still runs, and its result
    is the one of the real inputs"""
    import torch
    want = _device(det, mixed)
    real = {f: mixed[f] for f in ('cs', 'start', 'roff', 'score', 'key')}
    decoy = dict(real, score=-mixed['score'])                                 # (the same entries: the offsets stay those of the call)
    sw = S.Swapped(real, decoy)
    hoff = torch.from_numpy(want['hoff']).cuda()
    nrows = int(want['hoff'][-1])
    call = lambda out=None: det.read_hmm(sw.t['cs'], sw.t['start'], sw.t['roff'], sw.t['score'], sw.t['key'], hoff, nrows, pi=PI, length=LENGTH,
                                         call_post=CALL_POST, out=out)
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


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(mixed):
    eng = _engine()
    lib = L.load()
    ptr = eng._np_ptr
    n = 6
    c = {f: mixed[f][:n + 1 if f == 'roff' else n].copy() for f in ('cs', 'start', 'roff')}
    c['score'] = mixed['score'][:int(c['roff'][-1])].copy()
    c['key'] = mixed['key']
    hoff = eng.read_sites_host(c['cs'], c['start'], c['roff'], c['score'], c['key'])
    nrows, ns = int(hoff[-1]), len(c['key'])
    assert nrows > 3
    host = L.make_params(device=0, memspace=L.MEM_HOST)
    shapes = eng._hmm_shapes(ALL, nrows, n, ns)
    res = {f: np.full(k, 77, np.dtype(kind)) for f, (kind, k) in shapes.items()}
    untouched = lambda: all(np.all(v == 77) for v in res.values())

    def hmm(prm=host, nreads=n, hoff=hoff, nrows=nrows, opts=None, out=None, **kw):
        a = dict(c, **kw)
        opts = opts if opts is not None else L.make_hmm_opts(PI, LENGTH, CALL_POST)
        out = out if out is not None else L.make_hmm_out(**eng._np_ptrs(res))
        return lib.nmod_read_hmm(C.byref(prm) if prm is not None else None, nreads, ptr(a['cs']), ptr(a['start']), ptr(a['roff']), ptr(a['score']),
                                 ns, ptr(a['key']), ptr(hoff), nrows, C.byref(opts), C.byref(out))
    assert hmm(None) == -1 and hmm(L.make_params(device=0, memspace=5)) == -1 and hmm(nreads=2 ** 31) == -1 and hmm(nreads=-1) == -1
    for missing in ('cs', 'start', 'roff', 'score', 'key'):
        assert hmm(**{missing: None}) == -1, missing
    assert hmm(roff=c['roff'][::-1].copy()) == -1 and hmm(key=c['key'][::-1].copy()) == -1
    for bad in (dict(pi=0.0), dict(pi=1e-10), dict(pi=1.0), dict(pi=float('nan')), dict(length=1e-4), dict(length=1.1e9), dict(length=float('inf')),
                dict(length=float('nan')), dict(call_post=0.5), dict(call_post=1.0), dict(call_post=float('nan')), dict(call_post=float('inf'))):
        assert hmm(opts=L.make_hmm_opts(**dict(dict(pi=PI, length=LENGTH, call_post=CALL_POST), **bad))) == -1, bad
    short = L.make_hmm_opts(PI, LENGTH, CALL_POST); short.struct_size -= 8
    wrong = L.make_hmm_out(**eng._np_ptrs(res)); wrong.struct_size += 8
    assert hmm(opts=short) == -1 and hmm(out=wrong) == -1
    assert lib.nmod_read_hmm(C.byref(host), n, ptr(c['cs']), ptr(c['start']), ptr(c['roff']), ptr(c['score']), ns, ptr(c['key']), ptr(hoff), nrows, None,
                             C.byref(L.make_hmm_out(**eng._np_ptrs(res)))) == -1
    assert hmm(hoff=None) == -1 and hmm(nrows=-1) == -1 and hmm(nrows=2 ** 31) == -1 and hmm(nrows=nrows + 1) == -1
    down = hoff.copy()
    down[n - 1] = down[n] + 1
    assert hmm(hoff=hoff + 1) == -1 and hmm(hoff=down) == -1
    assert untouched()
    got = np.zeros(n + 1, np.int64) + 77
    total = C.c_int64(77)

    def count(prm=host, nreads=n, out=got, tot=total, **kw):
        a = dict(c, **kw)
        return lib.nmod_read_sites_count(C.byref(prm) if prm is not None else None, nreads, ptr(a['cs']), ptr(a['start']), ptr(a['roff']), ptr(a['score']),
                                         ns, ptr(a['key']), ptr(out), C.byref(tot) if tot is not None else None)
    assert count(None) == -1 and count(nreads=2 ** 31) == -1 and count(out=None) == -1 and count(tot=None) == -1
    for missing in ('cs', 'start', 'roff', 'score', 'key'):
        assert count(**{missing: None}) == -1, missing
    assert count(roff=c['roff'][::-1].copy()) == -1 and count(key=c['key'][::-1].copy()) == -1
    assert np.all(got == 77) and total.value == 77
    # what is not refused: no reads, no rows — zeroed site counts
    assert count() == 0 and same(got, hoff) and total.value == nrows
    assert hmm() == 0 and not untouched()
    z = {f: np.full(ns, 77, np.int32) for f in SITE}
    none = np.zeros(1, np.int64)
    assert lib.nmod_read_hmm(C.byref(host), 0, None, None, None, None, ns, ptr(c['key']), ptr(none), 0, C.byref(L.make_hmm_opts(PI, LENGTH, CALL_POST)),
                             C.byref(L.make_hmm_out(**eng._np_ptrs(z)))) == 0
    assert all(np.all(v == 0) for v in z.values())
    far = _case([(0, 300, np.full(30, 3.0)), (1, 151, np.full(9, 3.0))], c['key'])     # reads, none of which covers a site
    out = eng.read_hmm_host(*[far[f] for f in ('cs', 'start', 'roff', 'score', 'key')], pi=PI, length=LENGTH, call_post=CALL_POST)
    assert out['hoff'].tolist() == [0, 0, 0] and out['status'].tolist() == [1, 1] and out['ll'].tolist() == [0.0, 0.0] and len(out['post']) == 0
    assert all(np.all(out[f] == 0) for f in SITE + ('n_sites', 'n_mod', 'n_can', 'n_runs'))


# ------------------------------------------------------------------------------------------------------------ end to end
GRID = [12.5, 25.0, 50.0, 100.0, 200.0, 400.0]
CHAIN_PI = 0.15


@pytest.fixture(scope='module')
def chain():
    reads, model, alt, sites, planted = H.chain_inputs()
    exp = RF.restate(reads['norm_mean'], reads['off'], reads['base'], model['k'], model['center'], model['mean'], model['sd'], alt['mean'], alt['sd'],
                     'kmer', H.CHAIN_THR, 0.0)
    cs = (reads['strand'] == '-').astype(np.int32)
    key = np.unique(np.array([_key(0 if s == '+' else 1, p) for s, p in zip(sites[1], sites[2])], np.int64))
    walk = (cs, reads['start'], reads['off'], exp['llr_win'], key)
    profile = [(v, math.fsum(H.read_hmm_ref(*walk, CHAIN_PI, v, CALL_POST)['ll'].tolist())) for v in GRID]
    best = max(profile, key=lambda p: p[1])[0]
    return dict(reads=reads, model=model, alt=alt, sites=sites, planted=planted, cs=cs, key=key, profile=profile, best=best,
                ref=H.read_hmm_ref(*walk, CHAIN_PI, best, CALL_POST))


def test_end_to_end_through_smooth_reads_llr(chain):
    from nanomod_amd import readllr
    lines = []
    res = readllr.smooth_reads_llr(chain['reads'], chain['model'], chain['alt'], sites=chain['sites'], pi=CHAIN_PI, fit_length=GRID, call_post=CALL_POST,
                                   thr=H.CHAIN_THR, log=lines.append)
    ref = chain['ref']
    assert len(lines) == 1 and lines[0].startswith('readhmm: 120 read(s), %d candidate site(s), %d entries' % (len(chain['key']), len(ref['post'])))
    assert res['length'] == chain['best'] and [v for v, _ in res['profile']] == GRID and GRID[0] < chain['best'] < GRID[-1]
    for (_, got), (_, want) in zip(res['profile'], chain['profile']):
        assert abs(got - want) <= 1e-12 * (ref['denom'].sum() + len(ref['ll']))
    flat = dict(res['entries'], **res['reads'], site_n=res['sites']['n'], site_mod=res['sites']['n_mod'], site_can=res['sites']['n_can'])
    assert _check(flat, ref) == 0.0
    want = H.result_of(ref, chain['reads'], chain['key'])
    for f in ('read', 'first', 'last', 'n_sites'):
        assert same(np.asarray(res['domains'][f], np.int64), np.asarray(want['domains'][f], np.int64)), f
    assert same(res['sites']['pos'], want['sites']['pos']) and res['sites']['strand'].tolist() == want['sites']['strand'].tolist()
    # the point of the chain: of the planted entries, more are called modified at posterior 0.9 than K13's own sums reach its threshold
    ns = chain['planted'].shape[1]
    read_of = np.searchsorted(ref['hoff'], np.arange(len(ref['site'])), 'right') - 1
    planted = chain['planted'][read_of, ref['site'] % ns] & ((ref['site'] // ns) == chain['cs'][read_of])
    by_hmm, by_k13 = int((planted & (res['entries']['state'] == 1)).sum()), int((planted & (ref['s'] >= H.CHAIN_THR)).sum())
    print('planted entries %d: %d called by the chain at posterior %g, %d by K13 at threshold %g' % (planted.sum(), by_hmm, CALL_POST, by_k13, H.CHAIN_THR))
    assert by_hmm > by_k13
    # pi=None: the mean of K14's estimates at the candidate sites that have one
    auto = readllr.smooth_reads_llr(chain['reads'], chain['model'], chain['alt'], sites=chain['sites'], length=chain['best'], log=lambda *a: None)
    assert 0.02 < auto['pi'] < 0.5 and same(auto['entries']['hoff'], ref['hoff'])


def test_the_command_line_writes_the_restatement_s_rows(chain):
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
        argv = ['readhmm', '--wrkBase1', r_path, '--model', m_path, '--altModel', a_path, '--sites', s_path, '--hmmPi', repr(CHAIN_PI),
                '--fitLength', ','.join(repr(v) for v in GRID), '--callPost', repr(CALL_POST), '--outFolder', out, '--FileID', 'run', '--outLevel', '3']
        assert cli.main(argv) == 0
        want = H.result_of(chain['ref'], reads, chain['key'])
        for suffix, write in (('_read_hmm.txt', readllr.write_read_hmm), ('_read_domains.txt', readllr.write_read_domains), ('_site_hmm.txt', readllr.write_site_hmm)):
            write(os.path.join(tmp, 'want.txt'), want)
            text = open(os.path.join(out, 'run' + suffix)).read()
            assert text == open(os.path.join(tmp, 'want.txt')).read(), suffix
            assert len(text.splitlines()) == {'_read_hmm.txt': 120, '_read_domains.txt': len(want['domains']['read']), '_site_hmm.txt': len(chain['key'])}[suffix]
