"""The window ranking (nmod_region_rank, detect.region_rank, engine.region_rank_host) without a GPU: the plain restatement of
tests/region_ref.py against the reference's golden window orders, the conditions the constructed GPU cases are built to meet,
the Python front end over a recorder, and the C entry's refusals before any device work."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import region_ref as R
from nanomod_amd import _lib as L, detect as D, engine
from test_engine_marshal import rec, _snap, check_params, NO_SUCH_DEVICE, F32      # noqa: F401  (rec: the recording library)

G50_TAGS = ['w10_o0', 'w10_o1', 'w3_o1_A', 'w5_o0_ks', 'w4_o1_st']
RAGGED_TAGS = ['w2_o0', 'w2_o1', 'w3_o1_ks', 'w2_o1_st', 'w3_o1_A']


def _golden(fixture, tag):
    z = np.load(os.path.join(H.GOLDEN, '%s_regionrank_%s.npz' % (fixture, tag)))
    method, rank_use = str(z['method']), str(z['rankUse'])
    # (ragged has no KS-only table: the KS track and the records are those of its Stouffer table, the method only adds a track)
    exp, _ = H.load_expected('%s_%s' % (fixture, 'stouffer' if (fixture, method) == ('ragged', 'ks') else method))
    opts = (int(z['window']), int(z['WindOvlp']), float(z['percentile']), str(z['NA']))
    return z, exp, R.golden_value(exp, method, rank_use), opts


def _restated(exp, value, opts, **kw):
    kept, _ = R.ranked_windows(exp['chrom'], exp['strand'], exp['pos'], exp['base'], value, *opts, **kw)
    return [(c['seg'][0], c['seg'][1], c['pos'], str(exp['base'][c['index']])) for c in kept]


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize('tag', G50_TAGS)
def test_restatement_gives_the_g50_golden_orders(tag):
    z, exp, value, opts = _golden('g50', tag)
    got = _restated(exp, value, opts)
    assert [g[2] for g in got] == z['pos'].tolist()
    assert [g[3] for g in got] == z['base'].tolist()
    assert opts[0] + 1 == int(z['window_after'])


@pytest.mark.parametrize('tag', RAGGED_TAGS)
def test_restatement_gives_the_ragged_golden_orders(tag):
    """the reference's own ranking on four gapped (chrom, strand) segments inserted out of sorted order"""
    z, exp, value, opts = _golden('ragged', tag)
    want = list(zip(z['chrom'].tolist(), z['strand'].tolist(), z['pos'].tolist(), z['base'].tolist()))
    assert _restated(exp, value, opts) == want
    assert opts[0] + 1 == int(z['window_after'])
    assert len(set(zip(exp['chrom'].tolist(), exp['strand'].tolist()))) == 4
    if opts[3]:
        assert len(want) > 0
    else:
        assert len({(c, s) for c, s, _, _ in want}) >= 3
    if opts[1] == 1:
        assert len(want) < len(_restated(exp, value, opts, suppress=False))


def test_restatement_by_hand():
    """one strand, positions 10..21 and w = 3: pmax = 21, so the centres with all of pk - 3 .. pk + 3 tested and below it are
    13 .. 17; every number below was worked out on paper"""
    pos = np.arange(10, 22)
    val = np.array([.9, .8, .1, .7, .6, .5, .4, .1, .3, .2, .95, .0])
    a = (['c'] * 12, ['+'] * 12, pos, ['A'] * 12, val)
    ws = [c for c in R.walk(*a, 2, 1, 0.0, '') if not c['failed']]
    assert [c['pos'] for c in ws] == [13, 14, 15, 16, 17]
    # members of 13: .9 .8 .1 .7 .6 .5 .4 -> min .1 first at index 2 -> tb 1; of 14: .8 .1 .7 .6 .5 .4 .1 -> index 1 -> tb 2 (first of two)
    assert [(c['key'], c['tb']) for c in ws[:2]] == [(.1, 1), (.1, 2)]
    assert [(c['key'], c['tb']) for c in ws[2:]] == [(.1, 3), (.1, 1), (.1, 0)]          # 15: .1 at 0; 16: .1 at 4; 17: .1 at 3
    assert R.region_rank(*a, 2, 0, 0.0, '') == [3, 6]                                     # centres 10, 13, 16, 19: (.1, 1) twice, stable
    assert R.region_rank(*a, 2, 1, 0.0, '') == [7, 3]                  # 17 first; 13 (4 away) kept; 16, 14, 15 each closer than 3 to a kept one
    assert [c['key'] for c in R.walk(*a, 2, 1, 0.5, '') if not c['failed']][:2] == [.6, .5]
    assert [c['key'] for c in R.walk(*a, 2, 1, 1.0, '') if not c['failed']][:2] == [.9, .8]
    b = list('AAACAAAAAAAA')
    ws = [c for c in R.walk(a[0], a[1], pos, b, val, 2, 1, 0.0, 'A')]
    assert [(c['pos'], c['cnt'], c['tb']) for c in ws if c['cnt']][:2] == [(13, 6, 1), (14, 6, 2)] and ws[7]['cnt'] == 7


# ---------------------------------------------------------------------------------- what the constructed cases are built for
CASES = R.gpu_cases()


def _tallies(name):
    case, options = CASES[name]
    return [(o, R.tally(case['chrom'], case['strand'], case['pos'], case['base'], case['value'], o[0] - 1, *o[1:])) for o in options]


def _walks(name, opt):
    case, _ = CASES[name]
    a = (case['chrom'], case['strand'], case['pos'], case['base'], case['value'], opt[0] - 1) + tuple(opt[1:])
    return case, R.walk(*a), R.ranked_windows(*a)


@pytest.mark.parametrize('layout', ['inblock', 'at256'])
@pytest.mark.parametrize('w', [3, 4, 11, 22])
def test_segment_cases_meet_their_conditions(layout, w):
    name = 'segments_%s_w%d' % (layout, w)
    case, options = CASES[name]
    lo, hi = R.segment_bounds(case['chrom'], case['strand'])
    bounds = set(np.flatnonzero(np.diff(lo))[:] + 1)
    assert len(bounds) == 4
    assert (256 in bounds) == (layout == 'at256') and any(b % 256 for b in bounds)
    gaps = np.diff(case['pos'])[np.diff(lo) == 0]
    assert gaps.min() == 1 and gaps.max() == 5 and 0.04 < np.mean(gaps > 1) < 0.13
    assert {(o[1], o[2]) for o in options} == {(v, p) for v in (0, 1) for p in (0.0, 0.1, 0.5, 1.0)}
    for o, t in _tallies(name):
        assert t['valid'] > 0 and t['absent'] > 0, (o, t)                       # windows spanning a gap, and nothing else wrong with them
        assert (t['suppressed'] > 0) == (o[1] == 1), (o, t)
    _, walk, _ = _walks(name, options[-1])
    short = [k for k, n in zip(R.SEG_KEYS, np.bincount(np.cumsum(np.r_[0, np.diff(lo) != 0]))) if n < 2 * w + 1]
    assert len(short) >= (3 if w == 22 else 2)                                   # segments shorter than a window: 1, 6 (and 40) records
    assert all(c['failed'] for c in walk if c['seg'] in short) and any(c['seg'] in short for c in walk)


def test_shared_position_case_meets_its_conditions():
    case, options = CASES['shared_positions']
    n = len(case['pos']) // 3
    assert np.array_equal(case['pos'][:n], case['pos'][n:2 * n]) and np.array_equal(case['pos'][:n], case['pos'][2 * n:])
    assert len(set(zip(case['chrom'].tolist(), case['strand'].tolist()))) == 3
    assert len(set(case['chrom'].tolist())) == 2 and len(set(case['strand'].tolist())) == 2
    for o in options:
        assert o[1] == 1
        _, _, (kept, dropped) = _walks('shared_positions', o)
        assert len(kept) >= 9 and len(dropped) > 0 and len(kept) % 3 == 0
        for t in range(0, len(kept), 3):                                         # both strands and both chromosomes keep their window
            assert [c['seg'] for c in kept[t:t + 3]] == list(R.SEG_KEYS[:3])
            assert len({c['pos'] for c in kept[t:t + 3]}) == 1


@pytest.mark.parametrize('w', [3, 11])
def test_strand_end_cases_meet_their_conditions(w):
    name = 'strand_ends_w%d' % w
    for o in CASES[name][1]:
        _, walk, _ = _walks(name, o)
        by = lambda k: [c for c in walk if c['seg'] == R.SEG_KEYS[k]]
        assert not any(not c['failed'] for c in by(0))                           # 2w + 1 records: the only complete window ends at pmax
        assert [c['pos'] for c in by(0) if c['failed'] == {'at_pmax'}] == [500 + w]
        assert [c['pos'] for c in by(1) if not c['failed']] == [500 + w]          # 2w + 2 records: exactly that one
        assert [c['pos'] for c in by(2) if not c['failed']][0] == w               # from position 0: the first window's first member is 0
        assert [c['pos'] for c in by(3) if not c['failed']][0] in ((2 * w - 1,) if o[1] == 1 else (2 * w - 1, 3 * w - 1))
        neg = [c['pos'] for c in by(4) if c['failed'] == {'negative'}]            # complete windows with a member below 0
        assert neg == ([w - 3, w - 2, w - 1] if o[1] == 1 else [w - 3])
        assert any(not c['failed'] for c in by(4))


@pytest.mark.parametrize('w', [3, 4, 22])
def test_step_phase_cases_meet_their_conditions(w):
    name = 'step_phase_w%d' % w
    (o,) = CASES[name][1]
    assert o[1] == 0
    case, walk, _ = _walks(name, o)
    valid = [c['index'] for c in walk if not c['failed']]
    assert len(valid) >= 4 and all(i % w != 0 for i in valid)                     # no centre a walk stepping by index would visit
    assert all((int(case['pos'][i]) - int(case['pos'][0])) % w == 0 for i in valid)


@pytest.mark.parametrize('w', [3, 4])
def test_tie_cases_meet_their_conditions(w):
    name = 'ties_w%d' % w
    case, options = CASES[name]
    assert set(np.unique(case['value']).tolist()) <= set(R.TIE_VALUES) and np.signbit(case['value']).any()
    assert {(o[2], o[3]) for o in options} == {(0.0, ''), (0.5, ''), (0.0, 'A'), (0.5, 'A')}
    for o in options:
        _, walk, (kept, _) = _walks(name, o)
        valid = [c for c in walk if not c['failed']]
        runs = np.diff(np.flatnonzero(np.r_[True, [(a['key'], a['tb']) != (b['key'], b['tb']) for a, b in zip(valid, valid[1:])], True]))
        assert runs.max() >= (10 if o[1] == 1 else 3), o                          # neighbours with equal (key, tie-break): generation order decides
        parities = {c['cnt'] % 2 for c in valid}
        assert parities == ({0, 1} if o[3] else {1}), o
        # the minimum repeats inside a window, and not at its first member only: the first occurrence matters
        rep = 0
        for c in valid:
            i = c['index']
            m = [float(case['value'][j]) for j in range(i - w, i + w + 1) if not o[3] or case['base'][j] == o[3]]
            rep += m.count(min(m)) > 1 and m.index(min(m)) != len(m) - 1 - m[::-1].index(min(m))
        assert rep >= 10, o


@pytest.mark.parametrize('w', [3, 11])
def test_base_filter_cases_meet_their_conditions(w):
    name = 'base_filter_w%d' % w
    case, options = CASES[name]
    assert '' in case['base'].tolist() and b' ' in R.base_bytes(case['base'])
    for o in options:
        assert o[3] == 'A'
        _, walk, _ = _walks(name, o)
        cnts = {c['cnt'] for c in walk if c['cnt'] is not None}
        assert {5, 6, 2 * w + 1} <= cnts, o
        assert any(c['failed'] == {'few'} and c['cnt'] == 5 for c in walk) and any(not c['failed'] and c['cnt'] == 6 for c in walk)
        off = 0
        for c in walk:
            if not c['failed']:
                i = c['index']
                j = i - w + int(np.argmin(case['value'][i - w:i + w + 1]))
                off += case['base'][j] != 'A'
        assert off >= 5, o                                                        # the smallest member sits on a base that does not contribute


@pytest.mark.parametrize('w', [3, 4, 11])
def test_suppression_cases_meet_their_conditions(w):
    name = 'suppression_w%d' % w
    for o in CASES[name][1]:
        assert o[1] == 1
        _, _, (kept, dropped) = _walks(name, o)
        rank = _rank_key(kept, dropped)
        rk = lambda c: rank[(c['seg'], c['pos'])]
        better_kept = lambda c: [k for k in kept if k['seg'] == c['seg'] and rk(k) < rk(c)]        # (best first: kept is ranked)
        near = lambda c, pool: sorted(abs(k['pos'] - c['pos']) for k in pool)
        # dropped with its closest better kept window exactly w - 1 away; kept with a better kept window exactly w and w + 1 away
        assert any(near(c, better_kept(c))[0] == w - 1 for c in dropped), o
        assert any(w in near(c, better_kept(c)) for c in kept), o
        assert any(w + 1 in near(c, better_kept(c)) for c in kept), o
        # a chain: a dropped window whose only blocker is the best window of its segment, although the segment's second-best
        # kept window ranks above it too
        chain = 0
        for c in dropped:
            bk = better_kept(c)
            chain += len(bk) >= 2 and [k for k in bk if abs(k['pos'] - c['pos']) < w] == [bk[0]]
        assert chain >= 1 or o[2] != 0.5, o                                      # (built for the median: see case_suppression)
        # a kept window closer than w to a better-ranked window that was itself dropped: dropped windows block nothing
        assert any(any(k['seg'] == c['seg'] and abs(k['pos'] - c['pos']) < w and rk(k) < rk(c) for k in dropped) for c in kept), o


def _rank_key(kept, dropped):
    """(seg, pos) -> the window's place in the ranked list before the suppression: (key, tie-break), then generation order"""
    gen = sorted(kept + dropped, key=lambda c: (c['seg'], c['pos']))
    order = sorted(range(len(gen)), key=lambda g: (gen[g]['key'], gen[g]['tb']))
    return {(gen[g]['seg'], gen[g]['pos']): r for r, g in enumerate(order)}


# --------------------------------------------------------------------------------------------------- detect.region_rank
class HostRecorder:
    """stands in for engine.region_rank_host: records its arguments and answers from the restatement (segments named by strand_lo)"""

    def __init__(self):
        self.calls = []

    def __call__(self, lo, hi, pos, base, value, w, movesize, na, percentile, wind_ovlp, device=0):
        self.calls.append(dict(lo=np.array(lo), hi=np.array(hi), pos=np.array(pos), base=base, value=np.array(value), w=w, movesize=movesize,
                               na=na, percentile=percentile, wind_ovlp=wind_ovlp, device=device))
        chrom = ['s%09d' % v for v in np.asarray(lo).tolist()]
        return np.array(R.region_rank(chrom, ['+'] * len(chrom), pos, base, value, w - 1, wind_ovlp, percentile, na), dtype=np.int32)


@pytest.fixture
def host(monkeypatch):
    h = HostRecorder()
    monkeypatch.setattr(engine, 'region_rank_host', h)
    return h


def _records(case, rng=None):
    """sign_test records of a case: four (statistic, p-value) pairs each, the case's value at [sorted_ind][use_pind] = [3][1]
    and numbers that must not be picked everywhere else"""
    n = len(case['pos'])
    return [((str(case['chrom'][i]), str(case['strand'][i]), int(case['pos'][i]), str(case['base'][i]), 5, 5),
             [(100.0 + i, 200.0 + i), (300.0 + i, 400.0 + i), (float(case['value'][i]) + 7.0, 1.0 - float(case['value'][i])),
              (-float(case['value'][i]), float(case['value'][i]))]) for i in range(n)]


@pytest.mark.parametrize('sizes', [(30,), (12, 1), (9, 1, 14, 20, 1)])
@pytest.mark.parametrize('ovlp', [0, 1])
def test_front_end_builds_the_segment_arrays_and_options(host, sizes, ovlp):
    case = R.case_segments(np.random.default_rng(21), sizes)
    recs = _records(case)
    mo = {'sign_test': recs, 'window': 2, 'WindOvlp': ovlp, 'percentile': 0.1, 'NA': '', 'nmod_device': 3}
    got = D.region_rank(mo, 3, 1)
    assert mo['window'] == 3                                                     # incremented once, as the reference does in place
    (c,) = host.calls
    first = np.cumsum((0,) + sizes[:-1])
    assert c['lo'].tolist() == np.repeat(first, sizes).tolist()
    assert c['hi'].tolist() == np.repeat(first + np.array(sizes) - 1, sizes).tolist()
    assert (c['w'], c['movesize'], c['wind_ovlp'], c['percentile'], c['na'], c['device']) == (3, 1 if ovlp else 3, ovlp, 0.1, '', 3)
    assert c['pos'].tolist() == case['pos'].tolist() and c['value'].tolist() == case['value'].tolist()
    assert bytes(c['base']) == R.base_bytes(case['base'])
    want = R.region_rank(case['chrom'], case['strand'], case['pos'], case['base'], case['value'], 2, ovlp, 0.1, '')
    assert [r[0] for r in got] == [recs[i][0] for i in want] and all(g is recs[i] for g, i in zip(got, want))
    if sizes == (30,):
        assert len(want) > 0


@pytest.mark.parametrize('sorted_ind, use_pind, pick', [(3, 1, lambda v: v), (3, 0, lambda v: -v), (2, 1, lambda v: 1.0 - v), (2, 0, lambda v: v + 7.0),
                                                        (0, 0, None), (1, 1, None)])
def test_front_end_picks_the_ranked_number(host, sorted_ind, use_pind, pick):
    case = R.case_segments(np.random.default_rng(22), (25,))
    mo = {'sign_test': _records(case), 'window': 2, 'WindOvlp': 1, 'percentile': 0.5}          # (no 'NA' key: no filter)
    D.region_rank(mo, sorted_ind, use_pind)
    (c,) = host.calls
    n = np.arange(25)
    want = pick(case['value']) if pick else {(0, 0): 100.0 + n, (1, 1): 400.0 + n}[(sorted_ind, use_pind)]
    assert c['value'].tolist() == want.tolist() and c['na'] == '' and c['device'] == 0


def test_front_end_blanks_an_empty_base_and_passes_the_filter(host):
    case = R.case_base_filter(np.random.default_rng(23), 3)
    mo = {'sign_test': _records(case), 'window': 2, 'WindOvlp': 1, 'percentile': 0.1, 'NA': 'A'}
    got = D.region_rank(mo, 3, 1)
    (c,) = host.calls
    assert c['na'] == 'A' and len(c['base']) == len(case['pos'])
    assert [i for i, b in enumerate(bytes(c['base'])) if b == 32] == [70, 71, 150] and case['base'][70] == ''
    assert len(got) > 0


def test_front_end_returns_at_once_without_records(host):
    mo = {'sign_test': [], 'window': 2, 'WindOvlp': 1, 'percentile': 0.1}
    assert D.region_rank(mo, 3, 1) == [] and host.calls == [] and mo['window'] == 3


@pytest.mark.parametrize('damage', ['segments_swapped', 'strands_swapped', 'repeated_position', 'descending_position', 'segment_split'])
def test_front_end_refuses_records_out_of_order(host, damage):
    case = R.case_segments(np.random.default_rng(24), (10, 8, 12))
    recs = _records(case)
    if damage == 'segments_swapped':
        recs = recs[18:] + recs[:18]                                             # (chr2, +) before (chr1, +)
    elif damage == 'strands_swapped':
        recs = recs[10:18] + recs[:10] + recs[18:]                               # (chr1, -) before (chr1, +)
    elif damage == 'repeated_position':
        recs[4] = (recs[3][0], recs[4][1])
    elif damage == 'descending_position':
        recs[3], recs[4] = recs[4], recs[3]
    else:
        recs = recs[:5] + recs[10:18] + recs[5:10] + recs[18:]                   # (chr1, +) continues after (chr1, -)
    mo = {'sign_test': recs, 'window': 2, 'WindOvlp': 1, 'percentile': 0.1}
    with pytest.raises(ValueError, match='ordered by'):
        D.region_rank(mo, 3, 1)
    assert host.calls == []


# -------------------------------------------------------------------------------------------- engine.region_rank_host
@pytest.mark.parametrize('na', ['', 'A'])
def test_region_rank_host_marshalling(rec, na):
    n = 9
    seen = {}

    def region_rank(*args):                                                      # the recorder's entry, plus what a library would write back
        snap = [_snap(a) for a in args[:-1]]
        prm, npos, lo, hi, pos, base, value, w, movesize, na_, pct, ovlp, out = snap
        view = lambda addr, ct: np.ctypeslib.as_array((ct * n).from_address(addr)).copy()
        seen.update(prm=prm, npos=npos, lo=view(lo, C.c_int32), hi=view(hi, C.c_int32), pos=view(pos, C.c_int64),
                    value=view(value, C.c_double), base=base, scalars=(w, movesize, na_, pct, ovlp))
        np.ctypeslib.as_array((C.c_int32 * n).from_address(out))[:] = np.arange(n)[::-1]
        args[-1]._obj.value = 4
        rec.calls.append(('nmod_region_rank', snap))
        return 0
    rec.nmod_region_rank = region_rank
    big = np.arange(4 * n)
    lo = (big[::4] * 0).astype(np.int64)                                         # wrong dtypes and strided views: converted before the call
    hi = np.full(2 * n, n - 1, dtype=np.int16)[::2]
    pos = (big[::4] + 50).astype(np.int32)
    value = np.linspace(0, 1, 2 * n, dtype=np.float32)[::2]
    got = engine.region_rank_host(lo, hi, pos, bytearray(b'ACGT ACGT'), value, 3, 1, na, 0.25, 1, device=2)
    rec.only('nmod_region_rank')
    check_params(seen['prm'], dtype=F32, device=2)                               # memspace HOST
    assert seen['npos'] == n
    assert seen['lo'].tolist() == [0] * n and seen['hi'].tolist() == [n - 1] * n
    assert seen['pos'].tolist() == (np.arange(n) * 4 + 50).tolist() and seen['value'].tolist() == value.astype(np.float64).tolist()
    assert seen['base'] == b'ACGT ACGT'
    assert seen['scalars'] == (3, 1, b'A' if na else b'\0', 0.25, 1)
    assert got.dtype == np.int32 and got.tolist() == [8, 7, 6, 5]                # the first n_ranked entries


# ------------------------------------------------------------------------------------------- the C entry's refusals
def _entry(lib, npos=8, *, lo='x', hi='x', pos='x', base='x', value='x', out='x', cnt='x', w=3, movesize=1, na=b'\0', pct=0.1, ovlp=1,
           memspace=None, prm='x'):
    n = npos if 0 <= npos < 1000 else 8
    a = dict(lo=np.zeros(max(n, 1), np.int32), hi=np.full(max(n, 1), n - 1, np.int32), pos=np.arange(max(n, 1), dtype=np.int64),
             value=np.zeros(max(n, 1)), out=np.zeros(max(n, 1), np.int32))
    pick = lambda v, name: a[name].ctypes.data if isinstance(v, str) else None
    if isinstance(prm, str):
        prm = L.make_params(device=NO_SUCH_DEVICE, memspace=L.MEM_HOST if memspace is None else memspace)
    c = C.c_int64(-7)
    rc = lib.nmod_region_rank(C.byref(prm) if prm is not None else None, npos, pick(lo, 'lo'), pick(hi, 'hi'), pick(pos, 'pos'),
                              b'A' * max(n, 1) if base is not None else None, pick(value, 'value'), w, movesize, na, pct, ovlp, pick(out, 'out'),
                              C.byref(c) if cnt is not None else None)
    return rc, c.value


def test_region_rank_refuses_invalid_arguments_before_any_device_work():
    """every bad argument is NMOD_ERR_INVALID_ARG (-1) although the device does not exist, which alone is NMOD_ERR_NO_DEVICE (-5)"""
    lib = L.load()
    nan, inf = float('nan'), float('inf')
    call = lambda *a, **kw: _entry(lib, *a, **kw)[0]
    assert call() == -5 and call(pct=0.0) == -5 and call(pct=1.0) == -5 and call(w=0) == -5 and call(ovlp=0, movesize=3) == -5
    assert call(na=b'A') == -5
    assert _entry(lib, 0) == (0, 0)                                              # no records: no device needed, nothing ranked
    assert _entry(lib, 0, lo=None, hi=None, pos=None, base=None, value=None, out=None) == (0, 0)
    assert call(prm=None) == -1 and call(cnt=None) == -1 and call(0, cnt=None) == -1
    assert call(-1) == -1 and call(2 ** 31) == -1 and call(2 ** 40) == -1
    for name in ('lo', 'hi', 'pos', 'base', 'value', 'out'):
        assert call(**{name: None}) == -1, name
    assert call(w=-1) == -1 and call(movesize=0) == -1 and call(movesize=-3) == -1
    assert call(memspace=L.MEM_DEVICE) == -1 and call(memspace=2) == -1
    assert all(call(pct=v) == -1 for v in (-1e-300, -0.1, 1.0000000000000002, 1.5, nan, inf, -inf))
    bad = L.make_params(device=NO_SUCH_DEVICE); bad.struct_size -= 4
    assert call(prm=bad) == -1
    assert _entry(lib, w=-1)[1] == 0                                             # *n_ranked is cleared before the arrays are looked at
