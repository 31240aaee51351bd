"""CPU: the constructed cases of tests/chain_cases.py have the properties they are named for, from hmm_ref.entries_ref and numpy alone:
the reads with holes lie on both sides of the two class steps and their named tiles hold the per-wave counts that a wrong cross-wave
prefix of the fill would trip over; no reference posterior lies within its gate of a threshold; every site table selects the number of
sort passes it is meant for and carries rows where a pass too few, or a byte carry, would show."""
import numpy as np
import pytest

import chain_cases as CC
import classes_ref as K
import hmm_ref as H
from nanomod_amd import _lib as L


def _reads_of(c, pattern):
    return [(r, c['tags'][r][1]) for r in range(len(c['reads'])) if c['tags'][r][0] == pattern]


def test_the_constants_are_the_header_s():
    assert (CC.EVENTS_MAX, CC.ENTRIES_MAX) == (L.CALLS_WAVE_MAX, L.HMM_WAVE_MAX) == (2048, 1024)
    assert CC.TILE == 4 * CC.WAVE == 256 and CC.HOLE_EVENTS == (64, 65, 128, 129, 2048, 2049, 2304, 2305, 4100)
    assert {CC.EVENTS_MAX, CC.EVENTS_MAX + 1} <= set(CC.HOLE_EVENTS)              # the pair astride the by-events class step


def test_hole_reads_lie_on_both_sides_of_both_class_steps():
    c = CC.hole_reads()
    key = c['key']
    assert np.all(np.diff(key) > 0) and len(key) == 2 * (CC.TOP + 1) + CC.TOP // 7 + 1
    events, m = np.diff(c['roff']), np.diff(c['hoff'])
    covered = np.array([len(CC.covered_valid(rd, key)[1]) for rd in c['reads']])
    tags = c['tags']
    for p in CC.HOLE_PATTERNS:                                                     # every event count on '+' and on '-' in every pattern
        got = sorted((n, c['reads'][r][0]) for r, n in _reads_of(c, p))
        assert got == sorted((n, cs) for n in CC.HOLE_EVENTS for cs in (0, 1)), p
    assert sorted(n for _, n in _reads_of(c, 'sparse')) == list(CC.SPARSE_EVENTS) and len(_reads_of(c, 'mixed')) == 20
    assert all(events[r] == t[1] for r, t in enumerate(tags)) and len(tags) == 5 * 18 + 3 + 20
    holes = m < covered
    # the fill's form goes by the events, the chain's by the entries: all four combinations, with holes
    for long_fill, long_chain in ((True, True), (True, False), (False, True), (False, False)):
        sel = ((events > CC.EVENTS_MAX) == long_fill) & ((m > CC.ENTRIES_MAX) == long_chain) & holes & (m > 0)
        assert sel.sum() >= 2, (long_fill, long_chain)
    for r, n in _reads_of(c, 'sparse'):                                            # the workgroup form fills what a wave chains
        assert c['reads'][r][0] == 2 and n > CC.EVENTS_MAX and 0.7 * covered[r] < m[r] < 0.9 * covered[r] and covered[r] <= 858 < CC.ENTRIES_MAX
    a = {n: [m[r] for r, k in _reads_of(c, 'a') if k == n] for n in CC.HOLE_EVENTS}
    assert all(CC.ENTRIES_MAX < v < 0.75 * n for n in (2048, 2049) for v in a[n]) and all(0.6 * n < v for n in CC.HOLE_EVENTS if n >= 2048 for v in a[n])
    for v in (np.nan, np.inf, -np.inf):                                            # every kind of invalid score, in long reads too
        hit = [np.any(np.isnan(rd[2]) if v != v else rd[2] == v) for rd in c['reads']]
        assert sum(h and e > CC.EVENTS_MAX for h, e in zip(hit, events)) >= 20
    assert set(c['s'].tolist()) == set(CC.VALUES.tolist())
    # shuffled: the long reads are not in front, nor sorted by pattern
    first = [t[0] for t in tags[:30]]
    assert len(set(first)) >= 5 and [t[0] for t in tags] != sorted(t[0] for t in tags)
    assert len(c['site']) == m.sum() == 27341                                     # the entries of the case
    assert CC.longest_of_each_pattern(c) == [next(r for r, t in enumerate(tags) if t == (p, n)) for p, n in
                                             [(p, 4100) for p in CC.HOLE_PATTERNS] + [('sparse', 6000)]]


def test_the_named_tiles_hold_the_claimed_counts_per_wave():
    c = CC.hole_reads()
    key = c['key']
    m = np.diff(c['hoff'])
    checked = 0
    for r, n in _reads_of(c, 'b'):
        w = CC.wave_counts(c['reads'][r], key)
        ta, tb = CC.hole_tiles(n)
        assert w.sum() == m[r]
        if n < CC.TILE:                                                            # (one tile, not a full one: its wave 1 is empty all the same)
            assert w[0, 1] == 0 and w[0, 0] > 0
            continue
        assert (ta, tb) == (1, 3) and n > 4 * CC.TILE
        assert w[ta, 1] == 0 and w[ta, 0] > 0 and w[ta, 2] > 0 and w[ta, 3] > 0    # a word of 0 while later waves have entries
        assert w[tb, 0] == 0 == w[tb, 2] and w[tb, 1] > 0 and w[tb, 3] > 0
        full = w[:n // CC.TILE]
        assert 0 < full.max() < CC.WAVE and (full > 0).mean() > 0.85                # no wave is full: no word is the 64 of a read without holes
        checked += n > CC.EVENTS_MAX
    assert checked == 8                                                           # 2 049, 2 304, 2 305 and 4 100 events, both strands
    for r, n in _reads_of(c, 'c'):
        w = CC.wave_counts(c['reads'][r], key)
        assert np.all(w.sum(1) == 1) and m[r] == -(-n // CC.TILE)
        at = w[:n // CC.TILE].argmax(1)
        assert at.tolist() == [t % 4 for t in range(n // CC.TILE)]                # a different wave from tile to tile
    for r, n in _reads_of(c, 'd'):
        w = CC.wave_counts(c['reads'][r], key)
        assert m[r] == CC.WAVE == w.sum()
        if n >= CC.TILE:
            assert w[n // CC.TILE - 1, 3] == CC.WAVE
        else:
            assert w[0, n // CC.WAVE - 1] == CC.WAVE
    for r, n in _reads_of(c, 'e'):
        assert m[r] == 0 and not CC.wave_counts(c['reads'][r], key).any()
    for r, n in _reads_of(c, 'a'):
        if n >= CC.TILE:
            w = CC.wave_counts(c['reads'][r], key)[:n // CC.TILE]
            assert 25 < w.min() and w.max() < CC.WAVE and len(np.unique(w)) > 5
    # the wave form of the same counts: pattern (b) empties whole tiles of 64 there
    r = next(r for r, n in _reads_of(c, 'b') if n == CC.EVENTS_MAX)
    w = CC.wave_counts(c['reads'][r], key, CC.WAVE)
    assert w.shape == (32, 1) and not w[[5, 12, 14], 0].any() and w[[4, 6, 13, 15], 0].all()


def test_no_reference_posterior_of_the_hole_reads_lies_in_the_band():
    """hmm_ref.band_margin on the restatement alone: the states of every entry are the reference's to decide, the excluded share is 0"""
    c = CC.hole_reads()
    ref = H.read_hmm_ref(*[c[f] for f in CC.WALK], CC.PI, CC.LENGTH, CC.CALL_POST)
    assert np.array_equal(ref['hoff'], c['hoff']) and H.band_margin(ref['post'], CC.CALL_POST, ref['gate']).all()
    assert len(set(ref['state'].tolist())) == 3 and (ref['status'] == H.NO_SITE).sum() >= 18


PASSES = dict(zip(CC.SORT_NSITES, (1, 2, 2, 3, 3, 4)))


def test_the_site_tables_stand_on_both_sides_of_every_pass_step():
    assert CC.SORT_NSITES == (255, 256, 65535, 65536, 70000, 2 ** 24 + 3)
    for nsites, want in PASSES.items():                                           # the selector of nmod_read_class_rows, as written there
        assert CC.sort_passes(nsites) == want == (1 if nsites < 256 else 2 if nsites < 65536 else 3 if nsites < 16777216 else 4)
    assert {255, 256, 65535, 65536} <= set(CC.SORT_NSITES) and max(CC.SORT_NSITES) > 1 << 24
    assert [CC.byte_pair(n) for n in CC.SORT_NSITES] == [None] * 4 + [(1, 65537), (1, 2 ** 24 + 1)]


@pytest.mark.parametrize('nsites', CC.SORT_NSITES)
def test_the_reads_of_a_site_table_carry_rows_where_a_wrong_sort_would_show(nsites):
    n, reads, key = CC.sort_pass_case(nsites)
    assert n == nsites == len(key) and key[0] == 0 and np.all(np.diff(key[:1000]) == 3) and key[-1] == 3 * (nsites - 1)
    assert 60 <= len(reads) <= 120 and all(3 <= len(r[2]) <= 40 and r[0] == 0 for r in reads)
    c = CC.case_arrays(reads, key)
    rows = K.rows_ref(*[c[f] for f in CC.WALK])
    site = rows['site'].astype(np.int64)
    per = np.diff(rows['soff'])
    assert per[0] > 0 and per[-1] > 0                                             # the lowest and the highest site index
    for carry in CC.CARRIES:
        if carry < nsites:
            assert per[carry - 1] > 0 and per[carry] > 0, carry
    assert [carry for carry in CC.CARRIES if carry < nsites] == {255: [], 256: [], 65535: [256], 65536: [256], 70000: [256, 65536]}.get(nsites, [256, 65536, 2 ** 24])
    multi = np.array([len(set(rows['rread'][rows['srow'][rows['soff'][j]:rows['soff'][j + 1]]].tolist())) for j in np.flatnonzero(per >= 3)])
    assert (multi >= 3).sum() >= 10
    assert site[0] > site[-1] and (np.diff(site) < 0).sum() >= 30                 # row order is not site order: later reads start lower
    assert 200 < len(site) < 1500
    pair = CC.byte_pair(nsites)
    if PASSES[nsites] >= 3 and nsites > 65536:
        lo, hi = pair
        top = 8 * (PASSES[nsites] - 1)
        assert (lo ^ hi) == 1 << top and per[lo] > 0 and per[hi] > 0
        assert np.flatnonzero(site == hi).max() < np.flatnonzero(site == lo).min()   # a sort one pass short leaves hi in front of lo
        short = np.argsort(site & ((1 << top) - 1), kind='stable')
        assert not np.array_equal(short, rows['srow']) and np.array_equal(np.argsort(site, kind='stable'), rows['srow'])
    else:
        assert pair is None
