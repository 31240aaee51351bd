"""GPU: nmod_read_viterbi (K20) against tests/viterbi_ref.py: the device's own path scored by 60-digit mpmath within the derived gate of
the optimum, vit and delta within the gate, the path the reference's wherever the reference's margin exceeds the gate (nowhere excluded on
the constructed fixtures), the counts those of the device's own path; ties under the strict rule; a planted run across every seam of both
forms and the traceback's carry across tiles; batches larger than the grids; invariances as identical bytes; the stream contract; the
refusals; empty inputs; extremes; the chain K13 -> K19 -> K20 through readllr.smooth_reads_llr and `cli readhmm --decode`."""
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
import viterbi_ref as V
from nanomod_amd import _lib as L
from test_site_pairs import _key

pytestmark = pytest.mark.gpu

PI, LENGTH = 0.3, 30.0
ENTRY, READ, SITE = L.VIT_ENTRY_FIELDS, L.VIT_READ_FIELDS, L.VIT_SITE_FIELDS
ALL = ENTRY + READ + SITE
TILE_WAVE, TILE_GROUP = 64 * L.HMM_CHUNK, 256 * L.HMM_CHUNK
WALK = ('cs', 'start', 'roff', 'score', 'key')


def same(a, b):
    """identical bytes (a -0.0 is not a 0.0)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


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


def _device(det, c, pi=PI, length=LENGTH, **kw):
    """read_sites and read_viterbi on device tensors of case c -> the results as numpy, hoff among them"""
    import torch
    t = {f: torch.from_numpy(c[f]).cuda() for f in WALK}
    hoff, nrows = det.read_sites(*[t[f] for f in WALK])
    res = det.read_viterbi(*[t[f] for f in WALK], hoff, nrows, pi=pi, length=length, **kw)
    return dict({f: v.cpu().numpy() for f, v in res.items()}, hoff=hoff.cpu().numpy())


def _ref(c, pi=PI, length=LENGTH):
    return V.read_viterbi_ref(*[c[f] for f in WALK], pi, length, exact=True)


def _check(res, ref):
    """the device's results against the references (module docstring); returns the share of the entries that path equality leaves out"""
    assert same(res['hoff'], ref['hoff']) and same(res['site'], ref['site'])
    hoff = ref['hoff']
    worst = dict(opt=0.0, vit=0.0, delta=0.0)
    for r in range(len(hoff) - 1):
        a, b = int(hoff[r]), int(hoff[r + 1])
        if b == a:
            continue
        c, g = ref['mp'][r], float(ref['gate'][r])
        # 1. optimality: the device's own path, scored exactly; holds whatever the ties
        lost = float(c.opt - c.path_score_mp(res['path'][a:b]))
        assert -1e-50 <= lost <= g + ref['near_loss'][r], (r, lost, g, ref['near'][r])
        assert abs(res['vit'][r] - ref['opt'][r]) <= g, (r, res['vit'][r], ref['opt'][r], g)
        worst['opt'] = max(worst['opt'], lost / (ref['scale'][r] + 1.0))
        worst['vit'] = max(worst['vit'], abs(res['vit'][r] - ref['opt'][r]) / (ref['scale'][r] + 1.0))
    assert set(np.unique(res['path']).tolist()) <= {0, 1}
    # 2. the path is the reference's wherever the reference's margin is clear of the gate
    out = V.excluded(ref)
    assert same(res['path'][~out], ref['ref_path'][~out]), np.flatnonzero((res['path'] != ref['ref_path']) & ~out)[:5]
    # 3. delta, and the path against the device's own delta
    err = np.abs(res['delta'] - ref['ref_delta'])
    assert np.all(err <= ref['gate_row']), (np.flatnonzero(err > ref['gate_row'])[:5], err.max())
    clear = np.abs(res['delta']) > ref['gate_row']
    assert same(res['path'][clear], (res['delta'][clear] > 0).astype(np.uint8))
    if len(err):
        worst['delta'] = float(np.max(err / np.repeat(ref['scale'] + 1.0, np.diff(hoff))))
    # 4. the counts are those of the path that was written
    assert same(res['status'], ref['status']) and same(res['n_sites'], ref['n_sites'])
    own = dict(V.per_read(res['hoff'], res['path']), **V.per_site(res['site'], res['path'], len(ref['site_n'])))
    for f in ('n_mod', 'n_runs') + SITE:
        assert same(res[f], own[f]), f
    if not out.any():
        assert same(res['path'], ref['path'])                                  # (the float64 restatement agrees as well)
        for f in ('n_mod', 'n_runs') + SITE:
            assert same(res[f], ref[f]), f
    no_site = np.diff(hoff) == 0
    assert np.all(res['vit'][no_site] == 0.0) and np.all(res['n_mod'][no_site] == 0) and np.all(res['n_runs'][no_site] == 0)
    print('largest errors relative to D + 1: path score %.3g, vit %.3g, delta %.3g; largest gate %.3g (over %d entries)'
          % (worst['opt'], worst['vit'], worst['delta'], max([V.gate(int(m)) for m in np.diff(hoff) if m] or [0.0]), len(ref['path'])))
    return float(out.mean()) if len(out) else 0.0


# ------------------------------------------------------------------------------------------------------------ constructed reads
@pytest.fixture(scope='module')
def mixed():
    """test_read_hmm_gpu's `mixed` in construction: three (chrom, strand) ids with the same site positions, reads of 1 .. 60 events with
    scores of K19's grid, NaN and infinities; reads that cover no site, one site, and sites at their first and last event on '+' and '-'"""
    rng = np.random.default_rng(2011)
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
    c = _case(reads, key)
    c['ref'] = _ref(c)
    return c


def test_paths_margins_and_counts_on_constructed_reads(det, mixed):
    res = _device(det, mixed)
    ref = mixed['ref']
    assert set(res) == set(ALL) | {'hoff'} and len(ref['path']) > 2000
    assert _check(res, ref) == 0.0 and ref['near'].sum() == 0               # pi = 0.3 and the score grid leave no tie and no near decision
    m = np.diff(ref['hoff'])
    assert m[-7:].tolist() == [0, 0, 1, 1, 2, 2, 2] and (m == 0).sum() > 8 and m.max() >= 20
    assert ref['status'][-7:].tolist() == [1, 1, 0, 0, 0, 0, 0]
    a = ref['hoff'][-4]                                                       # '+': the score of event 0 belongs to 150, on '-' to 160
    assert res['delta'][a] > 0 > res['delta'][a + 1] and res['delta'][a + 2] < 0 < res['delta'][a + 3]
    assert res['n_runs'].max() >= 2 and res['site_n'].sum() == len(ref['path']) and 0 < res['n_mod'].sum() == res['path'].sum() == res['site_mod'].sum()
    ll = H.read_hmm_ref(*[mixed[f] for f in WALK], PI, LENGTH, 0.9)
    assert np.all(res['vit'] <= ll['ll'] + ref['gate'] + 1e-12 * (ll['denom'] + 1.0))          # vit <= ll, each to its own gate


def test_host_and_device_memspace_and_fewer_outputs_give_identical_bytes(det, mixed):
    dev = _device(det, mixed)
    eng = _engine()
    args = [mixed[f] for f in WALK]
    hoff = eng.read_sites_host(*args)
    assert same(hoff, dev['hoff'])
    host = eng.read_viterbi_host(*args, hoff, pi=PI, length=LENGTH)
    for f in ALL:
        assert same(host[f], dev[f]), f
    for want in (('vit',), ('path',), ('delta',), ('path', 'site', 'n_mod'), ('vit', 'n_sites', 'status', 'site_n'), ('n_runs',), ('site_mod', 'delta')):
        part = _device(det, mixed, want=want)                                 # vit alone; path without delta; delta without path
        assert set(part) == set(want) | {'hoff'}
        for f in want:
            assert same(part[f], dev[f]), (want, f)


def _per_read_rows(res, order):
    hoff = res['hoff']
    rows = np.concatenate([np.arange(hoff[r], hoff[r + 1]) for r in order]) if len(order) else np.zeros(0, np.int64)
    return {f: res[f][rows] for f in ENTRY}


def test_a_permutation_of_the_reads_and_a_read_alone_change_nothing(det, mixed):
    dev = _device(det, mixed)
    n = len(mixed['cs'])
    order = np.random.default_rng(2012).permutation(n)
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
    for r in (longest, n - 3, 7):
        alone = _device(det, _case([reads[r]], mixed['key']))
        for f in ENTRY:
            assert same(alone[f], dev[f][dev['hoff'][r]:dev['hoff'][r + 1]]), (r, f)
        for f in READ:
            assert same(alone[f], dev[f][r:r + 1]), (r, f)


# ------------------------------------------------------------------------------------------------------------ ties
def test_ties_go_to_state_0(det):
    """pi = 0.5: with every score 0 the two constant paths tie and the path is all 0; with +s on one half and -s on the other, and the
    mirror image, the paths are the reference's under the strict comparison"""
    ms = (1, 2, 5, 9, 64, 300, TILE_WAVE + 1, L.HMM_WAVE_MAX + 9)
    top = max(ms)
    key = np.array([_key(0, 7 * p) for p in range(top)], np.int64)            # equal gaps
    zeros = _case([(0, 0, np.zeros(7 * (m - 1) + 1)) for m in ms], key)
    res = _device(det, zeros, pi=0.5)
    assert np.diff(res['hoff']).tolist() == list(ms)
    assert not res['path'].any() and not res['n_runs'].any() and not res['n_mod'].any() and not res['site_mod'].any()
    ref = _ref(zeros, pi=0.5)
    assert not ref['ref_path'].any() and V.excluded(ref).all() and _check(res, ref) == 1.0    # every entry an exact tie: optimality still holds
    reads, want = [], []
    for m in ms[1:]:
        for first in (True, False):
            s = np.zeros(7 * (m - 1) + 1)
            s[::7] = V.half_scores(m, 4.0, first)
            reads.append((0, 0, s))
            want.append(([1] * (m // 2) + [0] * (m - m // 2)) if first else ([0] * (m // 2) + [1] * (m - m // 2)))
    c = _case(reads, key)
    res = _device(det, c, pi=0.5)
    ref = _ref(c, pi=0.5)
    _check(res, ref)
    assert res['path'].tolist() == [z for w in want for z in w] == ref['ref_path'].tolist() and np.all(res['n_runs'] == 1)
    even = np.array([m % 2 == 0 for m in ms[1:]])                             # halves of equal size: the mirror image has the same best score
    assert even.sum() >= 3 and np.all(np.abs(res['vit'][0::2] - res['vit'][1::2])[even] <= ref['gate'][0::2][even])


# ------------------------------------------------------------------------------------------------------------ the seams of the scan
SEAM_M = [1, 2, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2 * 1024 * 2 + 3]
SEAMS = (L.HMM_CHUNK, TILE_WAVE, 2 * TILE_WAVE, 3 * TILE_WAVE, TILE_GROUP, L.HMM_WAVE_MAX, 2 * TILE_GROUP)
assert TILE_WAVE == 256 and TILE_GROUP == 1024 == L.HMM_WAVE_MAX


def _seam_reads(m):
    """the planted runs of the reads of m entries, (first, last) lists: one read whose runs have an end on either side of every seam the
    scan has below m — a thread's chunk, the wave tile, the wave boundaries of the workgroup form, the workgroup tile, the class step —
    counted from the read's first entry (the forward pass) and from its last (the traceback and the backward pass); and one read with a
    single run from its third entry to its third last, which starts in the last tile and ends in the first"""
    if m < 8:
        return [[(0, m - 1)]]
    marks = sorted({b for b in SEAMS if b + 3 < m} | {m - b for b in SEAMS if b + 3 < m})
    runs = []
    for b in marks:                                                           # entries b - 3 .. b + 2: an end on either side of b
        if runs and b - 3 <= runs[-1][1] + 1:
            runs[-1] = (runs[-1][0], b + 2)
        else:
            runs.append((b - 3, b + 2))
    return [runs, [(2, m - 3)]]


def test_planted_runs_across_every_seam_of_the_scan(det):
    """every position a candidate site, so a read of m events has m entries; scores -6 with runs of +6"""
    key = np.array([_key(1, p) for p in range(max(SEAM_M) + 5)], np.int64)
    reads, planted = [], []
    for m in SEAM_M:
        for runs in _seam_reads(m):
            s = np.full(m, -6.0)
            for first, last in runs:
                s[first:last + 1] = 6.0
            assert same(s, H.planted_run(m, *runs[0])) or len(runs) > 1
            reads.append((1, 3, s[::-1].copy()))                              # '-': event i lies at start + m - 1 - i
            planted.append(runs)
    c = _case(reads, key)
    res = _device(det, c, length=20.0)
    ref = _ref(c, length=20.0)
    assert np.diff(ref['hoff']).tolist() == [m for m in SEAM_M for _ in _seam_reads(m)]
    assert _check(res, ref) == 0.0 and ref['near'].sum() == 0
    for r, runs in enumerate(planted):
        got = H.runs(res['path'][res['hoff'][r]:res['hoff'][r + 1]])
        assert list(zip(got[0].tolist(), got[1].tolist())) == runs and res['n_runs'][r] == len(runs), (r, got, runs)
    assert max(len(runs) for runs in planted) >= 8


def test_more_reads_than_either_grid_has_units(det):
    """in read_batch_cases' manner: a batch whose reads are copies of a few distinct reads, more of them than the persistent grids of
    either form have waves (workgroups), has the distinct reads' outputs, gathered; the site counts are their sums"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(2013)
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
        per = np.stack([V.per_site(single['site'][single['hoff'][r]:single['hoff'][r + 1]], single['path'][single['hoff'][r]:single['hoff'][r + 1]],
                                   len(key))[f] for r in range(len(distinct))])
        assert same(batch[f], (per * np.bincount(idx, minlength=len(distinct))[:, None]).sum(0).astype(np.int32)), f
    long_read = (0, 0, rng.normal(0.0, 3.0, 2 * top - 1))                      # top entries: the workgroup form
    one = _device(det, _case([long_read], key))
    assert one['n_sites'].tolist() == [top] and 0 < one['n_mod'][0] < top
    many = RB.long_units(cus) + 50
    rep = _device(det, _case([long_read] * many, key), want=('path', 'delta', 'n_runs', 'vit', 'site_mod'))
    assert same(rep['path'], np.tile(one['path'], many)) and same(rep['delta'], np.tile(one['delta'], many))
    assert same(rep['vit'], np.repeat(one['vit'], many)) and same(rep['n_runs'], np.repeat(one['n_runs'], many)) and same(rep['site_mod'], one['site_mod'] * many)


# ------------------------------------------------------------------------------------------------------------ extremes
@pytest.mark.parametrize('pi,length', [(0.3, 1e6), (1e-9, 1e6), (1.0 - 1e-9, 200.0), (0.3, 1e-3), (1e-9, 1e9)])
def test_extremes_against_mpmath(det, pi, length):
    """+-800 next to each other at distance 1, the ends of pi's range, a gap of 60 000 bases (rho underflows to 0 at the shorter lengths),
    and 300 entries of K19's score grid at every parameter pair"""
    rng = np.random.default_rng(2014)
    pos = np.concatenate(([10, 11, 12, 13, 60013, 60014, 60015], 60100 + np.cumsum(rng.integers(1, 40, 300))))
    key = np.array([_key(0, p) for p in pos], np.int64)
    scores = np.full(60010, np.nan)
    scores[[0, 1, 2, 3, 60003, 60004, 60005]] = 800.0, -800.0, 800.0, -800.0, 5.0, -5.0, 40.0
    grid = np.full(int(pos[-1]) - 60100 + 1, np.nan)
    grid[pos[7:] - 60100] = rng.choice(np.array([3.0, -3.0, 2.5, -2.5, 1.0, -0.5, 0.0, 40.0, -7.5]), 300)
    c = _case([(0, 10, scores), (0, 10, scores[:4]), (0, 11, -scores[1:6]), (0, 60100, grid)], key)
    res = _device(det, c, pi=pi, length=length)
    ref = _ref(c, pi, length)
    assert ref['hoff'].tolist() == [0, 7, 11, 14, 314]
    assert _check(res, ref) == 0.0 and np.all(np.isfinite(res['delta'])) and np.all(np.isfinite(res['vit']))


# ------------------------------------------------------------------------------------------------------------ the stream
def test_side_stream_and_no_wait_for_the_work_before_it(det, mixed):
    """test_read_hmm_gpu's contract test for this entry: a side stream gives the default stream's result; behind a stall on a fresh
    stream the call returns while the stall still runs, and its result is the one of the inputs in place when it ran"""
    import torch
    want = _device(det, mixed)
    real = {f: mixed[f] for f in WALK}
    decoy = dict(real, score=-mixed['score'])                                 # (the same entries: the offsets stay those of the call)
    sw = S.Swapped(real, decoy)
    hoff = torch.from_numpy(want['hoff']).cuda()
    nrows = int(want['hoff'][-1])
    call = lambda out=None: det.read_viterbi(*[sw.t[f] for f in WALK], hoff, nrows, pi=PI, length=LENGTH, out=out)
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


# ------------------------------------------------------------------------------------------------------------ refusals, empty inputs
def test_refusals_write_nothing_and_empty_inputs(mixed):
    eng = _engine()
    lib = L.load()
    ptr = eng._np_ptr
    n = 6
    c = {f: mixed[f][:n + 1 if f == 'roff' else n].copy() for f in ('cs', 'start', 'roff')}
    c['score'] = mixed['score'][:int(c['roff'][-1])].copy()
    c['key'] = mixed['key']
    hoff = eng.read_sites_host(*[c[f] for f in WALK])
    nrows, ns = int(hoff[-1]), len(c['key'])
    assert nrows > 3
    host = L.make_params(device=0, memspace=L.MEM_HOST)
    shapes = eng._vit_shapes(ALL, nrows, n, ns)
    res = {f: np.full(k, 77, np.dtype(kind)) for f, (kind, k) in shapes.items()}
    untouched = lambda: all(np.all(v == 77) for v in res.values())

    def vit(prm=host, nreads=n, hoff=hoff, nrows=nrows, opts=None, out=None, **kw):
        a = dict(c, **kw)
        opts = opts if opts is not None else L.make_vit_opts(PI, LENGTH)
        out = out if out is not None else L.make_vit_out(**eng._np_ptrs(res))
        return lib.nmod_read_viterbi(C.byref(prm) if prm is not None else None, nreads, ptr(a['cs']), ptr(a['start']), ptr(a['roff']), ptr(a['score']),
                                     ns, ptr(a['key']), ptr(hoff), nrows, C.byref(opts), C.byref(out))
    assert vit(None) == -1 and vit(L.make_params(device=0, memspace=5)) == -1 and vit(nreads=2 ** 31) == -1 and vit(nreads=-1) == -1
    for missing in WALK:
        assert vit(**{missing: None}) == -1, missing
    assert vit(roff=c['roff'][::-1].copy()) == -1 and vit(key=c['key'][::-1].copy()) == -1
    for bad in (dict(pi=0.0), dict(pi=1e-10), dict(pi=1.0), dict(pi=float('nan')), dict(length=1e-4), dict(length=1.1e9), dict(length=float('inf')),
                dict(length=float('nan'))):
        assert vit(opts=L.make_vit_opts(**dict(dict(pi=PI, length=LENGTH), **bad))) == -1, bad
    short = L.make_vit_opts(PI, LENGTH); short.struct_size -= 8
    wrong = L.make_vit_out(**eng._np_ptrs(res)); wrong.struct_size += 8
    hmm_sized = L.make_vit_opts(PI, LENGTH); hmm_sized.struct_size = C.sizeof(L.NmodHmmOpts)
    assert vit(opts=short) == -1 and vit(out=wrong) == -1 and vit(opts=hmm_sized) == -1
    assert lib.nmod_read_viterbi(C.byref(host), n, ptr(c['cs']), ptr(c['start']), ptr(c['roff']), ptr(c['score']), ns, ptr(c['key']), ptr(hoff), nrows, None,
                                 C.byref(L.make_vit_out(**eng._np_ptrs(res)))) == -1
    assert vit(hoff=None) == -1 and vit(nrows=-1) == -1 and vit(nrows=2 ** 31) == -1 and vit(nrows=nrows + 1) == -1
    down = hoff.copy()
    down[n - 1] = down[n] + 1
    assert vit(hoff=hoff + 1) == -1 and vit(hoff=down) == -1
    assert untouched()
    assert vit() == 0 and not untouched()
    # what is not refused: no reads, no rows — zeroed site counts; reads without sites
    z = {f: np.full(ns, 77, np.int32) for f in SITE}
    none = np.zeros(1, np.int64)
    assert lib.nmod_read_viterbi(C.byref(host), 0, None, None, None, None, ns, ptr(c['key']), ptr(none), 0, C.byref(L.make_vit_opts(PI, LENGTH)),
                                 C.byref(L.make_vit_out(**eng._np_ptrs(z)))) == 0
    assert all(np.all(v == 0) for v in z.values())
    far = _case([(0, 300, np.full(30, 3.0)), (1, 151, np.full(9, 3.0))], c['key'])     # reads, none of which covers a site: nrows = 0
    out = eng.read_viterbi_host(*[far[f] for f in WALK], pi=PI, length=LENGTH)
    assert out['hoff'].tolist() == [0, 0, 0] and out['status'].tolist() == [L.HMM_NO_SITE] * 2 and out['vit'].tolist() == [0.0, 0.0]
    assert len(out['path']) == 0 and len(out['delta']) == 0 and all(np.all(out[f] == 0) for f in SITE + ('n_sites', 'n_mod', 'n_runs'))


# ------------------------------------------------------------------------------------------------------------ end to end
GRID = [12.5, 25.0, 50.0, 100.0, 200.0, 400.0]
CHAIN_PI, CALL_POST = 0.15, 0.9
POSTERIOR_KEYS = {'pi', 'length', 'profile', 'reads', 'entries', 'sites', 'domains'}


@pytest.fixture(scope='module')
def chain():
    """hmm_ref.chain_inputs and the smoothing of today on it (decode left at its default): what the length is chosen by"""
    from nanomod_amd import readllr
    reads, model, alt, sites, planted = H.chain_inputs()
    exp = RF.restate(reads['norm_mean'], reads['off'], reads['base'], model['k'], model['center'], model['mean'], model['sd'], alt['mean'], alt['sd'],
                     'kmer', H.CHAIN_THR, 0.0)
    cs = (reads['strand'] == '-').astype(np.int32)
    key = np.unique(np.array([_key(0 if s == '+' else 1, p) for s, p in zip(sites[1], sites[2])], np.int64))
    lines = []
    post = readllr.smooth_reads_llr(reads, model, alt, sites=sites, pi=CHAIN_PI, fit_length=GRID, call_post=CALL_POST, thr=H.CHAIN_THR, log=lines.append)
    walk = (cs, reads['start'], reads['off'], exp['llr_win'], key)
    return dict(reads=reads, model=model, alt=alt, sites=sites, planted=planted, cs=cs, key=key, post=post, lines=lines, walk=walk,
                ref=V.read_viterbi_ref(*walk, CHAIN_PI, post['length'], chain=V.viterbi_device_order, exact=True))


def _viterbi_result_of(ref, reads, key, post=None):
    """the restatement's results in the layout of smooth_reads_llr's `viterbi` entry"""
    from nanomod_amd import readllr
    with np.errstate(invalid='ignore', divide='ignore'):
        share = np.where(ref['site_n'] > 0, ref['site_mod'] / ref['site_n'].astype(np.float64), np.nan)
    sites = dict(chrom=np.array(['chrT'])[key >> 41], strand=np.where((key >> 40) & 1, '-', '+').astype('U1'), pos=key & H.POS_MASK, n=ref['site_n'],
                 n_mod=ref['site_mod'], share=share)
    table = dict(index=np.arange(len(ref['vit'])), chrom=np.asarray(reads['chrom']).astype(str), strand=np.asarray(reads['strand']).astype(str))
    return dict(reads=table, entries={f: ref[f] for f in ('hoff', 'site', 'path', 'delta')}, sites=sites,
                domains=readllr.read_domains(ref['hoff'], ref['site'], ref['path'], post, sites['pos'], delta=ref['delta']))


def test_end_to_end_through_smooth_reads_llr(chain):
    from nanomod_amd import readllr
    post, ref = chain['post'], chain['ref']
    assert set(post) == POSTERIOR_KEYS and len(chain['lines']) == 1           # the default: today's keys and one line
    lines = []
    res = readllr.smooth_reads_llr(chain['reads'], chain['model'], chain['alt'], sites=chain['sites'], pi=CHAIN_PI, fit_length=GRID, call_post=CALL_POST,
                                   thr=H.CHAIN_THR, log=lines.append, decode='both')
    assert set(res) == POSTERIOR_KEYS | {'viterbi'} and len(lines) == 2 and lines[0] == chain['lines'][0] and lines[1].startswith('readhmm: Viterbi paths at pi 0.15')
    assert res['length'] == post['length'] and res['profile'] == post['profile'] and GRID[0] < res['length'] < GRID[-1]
    for part in ('reads', 'entries', 'sites', 'domains'):                     # the posterior decoding's bytes are those of the default
        assert set(res[part]) == set(post[part])
        for f in post[part]:
            assert same(res[part][f], post[part][f]) or res[part][f].dtype.kind == 'U' and res[part][f].tolist() == post[part][f].tolist(), (part, f)
    v = res['viterbi']
    flat = dict(v['entries'], **v['reads'], site_n=v['sites']['n'], site_mod=v['sites']['n_mod'])
    assert _check(flat, ref) == 0.0
    # path_logpost = vit - ll is the log of a probability: at most 0, to the gates of its two terms
    ll = H.read_hmm_ref(*chain['walk'], CHAIN_PI, res['length'], CALL_POST)
    assert same(v['reads']['path_logpost'], v['reads']['vit'] - res['reads']['ll'])
    assert np.all(v['reads']['path_logpost'] <= ref['gate'] + np.array([H.gate(int(m)) if m else 0.0 for m in np.diff(ref['hoff'])]) * (ll['denom'] + 1.0))
    assert np.all(v['reads']['path_logpost'][ref['n_sites'] > 1] < 0)
    want = _viterbi_result_of(ref, chain['reads'], chain['key'], post['entries']['post'])
    for f in ('read', 'first', 'last', 'n_sites'):
        assert same(np.asarray(v['domains'][f], np.int64), np.asarray(want['domains'][f], np.int64)), f
    assert np.all(np.abs(v['domains']['min_delta'] - want['domains']['min_delta']) <= ref['gate'][want['domains']['read']]) and np.all(v['domains']['min_delta'] >= -ref['gate'][want['domains']['read']])
    # the planted stretches come back as domains: every planted read has a run on its path, and the path calls more planted entries than
    # K13's own sums reach its threshold
    ns = chain['planted'].shape[1]
    read_of = np.searchsorted(ref['hoff'], np.arange(len(ref['site'])), 'right') - 1
    planted = chain['planted'][read_of, ref['site'] % ns] & ((ref['site'] // ns) == chain['cs'][read_of])
    by_path, by_k13 = int((planted & (v['entries']['path'] == 1)).sum()), int((planted & (ref['s'] >= H.CHAIN_THR)).sum())
    inside = np.bincount(read_of[planted & (v['entries']['path'] == 1)], minlength=len(chain['cs']))
    has = np.bincount(read_of[planted], minlength=len(chain['cs'])) > 0
    print('planted entries %d on %d reads: %d on the Viterbi path, %d by K13 at threshold %g; %d planted reads with a domain inside the stretch'
          % (planted.sum(), has.sum(), by_path, by_k13, H.CHAIN_THR, (inside[has] > 0).sum()))
    assert by_path > by_k13 and np.all(inside[has] > 0)
    only = readllr.smooth_reads_llr(chain['reads'], chain['model'], chain['alt'], sites=chain['sites'], pi=CHAIN_PI, length=res['length'], thr=H.CHAIN_THR,
                                    log=lambda *a: None, decode='viterbi')
    assert set(only) == {'pi', 'length', 'profile', 'viterbi'} and 'path_logpost' not in only['viterbi']['reads']
    for f in ('path', 'delta', 'site', 'hoff'):
        assert same(only['viterbi']['entries'][f], v['entries'][f]), f
    assert np.all(np.isnan(only['viterbi']['domains']['mean_post'])) and same(only['viterbi']['domains']['min_delta'], v['domains']['min_delta'])


def test_the_command_line_writes_the_restatement_s_rows(chain):
    from nanomod_amd import cli, container, kmermodel, readllr
    reads = chain['reads']
    k19 = ('_read_hmm.txt', '_read_domains.txt', '_site_hmm.txt')
    k20 = (('_read_viterbi.txt', readllr.write_read_viterbi), ('_read_domains_viterbi.txt', readllr.write_read_domains), ('_site_viterbi.txt', readllr.write_site_viterbi))
    with tempfile.TemporaryDirectory() as tmp:
        r_path, m_path, a_path, s_path = (os.path.join(tmp, n) for n in ('reads.npz', 'model.npz', 'alt.npz', 'sites.txt'))
        container.save_reads(r_path, *[reads[f] for f in ('chrom', 'strand', 'start', 'off', 'norm_mean', 'base')])
        zeros = np.zeros(64, np.int64)
        for path, m in ((m_path, chain['model']), (a_path, chain['alt'])):
            kmermodel.save_kmer_model(path, dict(version=kmermodel.KMER_MODEL_VERSION, clip_sigma=0.0, k=3, center=0, mean=m['mean'], sd=m['sd'],
                                                 n_positions=m['n_positions'], n_samples=zeros + 10, n_clipped=zeros))
        open(s_path, 'w').writelines('%s %s %d\n' % (c, s, p + 1) for c, s, p in zip(*chain['sites']))
        argv = ['readhmm', '--wrkBase1', r_path, '--model', m_path, '--altModel', a_path, '--sites', s_path, '--hmmPi', repr(CHAIN_PI),
                '--fitLength', ','.join(repr(v) for v in GRID), '--callPost', repr(CALL_POST), '--FileID', 'run', '--outLevel', '3']
        outs = {d: os.path.join(tmp, d) for d in ('plain', 'posterior', 'both', 'viterbi')}
        assert cli.main(argv + ['--outFolder', outs['plain']]) == 0
        for d in ('posterior', 'both', 'viterbi'):
            assert cli.main(argv + ['--outFolder', outs[d], '--decode', d]) == 0
        assert sorted(os.listdir(outs['plain'])) == sorted(os.listdir(outs['posterior'])) == sorted('run' + s for s in k19)
        assert sorted(os.listdir(outs['viterbi'])) == sorted('run' + s for s, _ in k20) and len(os.listdir(outs['both'])) == 6
        for s in k19:                                                         # the three K19 files: byte-identical to a run without the option
            plain = open(os.path.join(outs['plain'], 'run' + s), 'rb').read()
            assert plain == open(os.path.join(outs['posterior'], 'run' + s), 'rb').read() == open(os.path.join(outs['both'], 'run' + s), 'rb').read() and plain, s
        want = _viterbi_result_of(chain['ref'], reads, chain['key'], chain['post']['entries']['post'])
        for s, write in k20:
            write(os.path.join(tmp, 'want.txt'), want)
            text = open(os.path.join(outs['both'], 'run' + s)).read()
            assert text == open(os.path.join(tmp, 'want.txt')).read(), s
            assert len(text.splitlines()) == {'_read_viterbi.txt': len(chain['ref']['path']), '_read_domains_viterbi.txt': len(want['domains']['read']),
                                              '_site_viterbi.txt': len(chain['key'])}[s]
            if s != '_read_domains_viterbi.txt':                              # (without posteriors the domains' mean_post column is nan)
                assert text == open(os.path.join(outs['viterbi'], 'run' + s)).read(), s
