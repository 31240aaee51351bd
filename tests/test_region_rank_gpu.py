"""nmod_region_rank on the device against the plain restatement of tests/region_ref.py, on constructed records where each of
the entry's conditions takes both branches (tests/test_region_rank.py checks, without a GPU, that the cases do what they are
built for).  Ranks are exact: every comparison is equality of the index list."""
import os

import numpy as np
import pytest

import helpers as H
import region_ref as R
from nanomod_amd import detect as D, engine

pytestmark = pytest.mark.gpu

CASES = R.gpu_cases()


def _device(case, w, ovlp, pct, na):
    lo, hi = R.segment_bounds(case['chrom'], case['strand'])
    return engine.region_rank_host(lo, hi, case['pos'], R.base_bytes(case['base']), case['value'], w, 1 if ovlp == 1 else w, na, pct,
                                   ovlp).tolist()


def _restated(case, w, ovlp, pct, na):
    return R.region_rank(case['chrom'], case['strand'], case['pos'], case['base'], case['value'], w - 1, ovlp, pct, na)


def _check(name, nonempty=True):
    case, options = CASES[name]
    for o in options:
        want = _restated(case, *o)
        got = _device(case, *o)
        assert got == want, (name, o, len(got), len(want), next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), None))
        assert len(want) > 0 or not nonempty, (name, o)


@pytest.mark.parametrize('layout', ['inblock', 'at256'])
@pytest.mark.parametrize('w', [3, 4, 11, 22])
def test_segments_and_gaps(layout, w):
    """five segments of 1 to 700 records with gaps of 1-4 positions, both WindOvlp values, percentiles 0, 0.1, 0.5 and 1: windows
    that span a gap or a segment boundary (inside a 256-thread block, and on the block boundary at index 256) are no windows"""
    _check('segments_%s_w%d' % (layout, w))


def test_same_positions_on_two_strands_and_two_chromosomes():
    """the suppression never crosses a (chrom, strand): the three copies of one segment keep the same windows, ranked adjacent and
    in segment order"""
    _check('shared_positions')
    case, options = CASES['shared_positions']
    n = len(case['pos']) // 3
    for o in options:
        got = _device(case, *o)
        assert len(got) % 3 == 0 and len(got) >= 9
        for t in range(0, len(got), 3):
            assert got[t + 1] == got[t] + n and got[t + 2] == got[t] + 2 * n and got[t] < n


@pytest.mark.parametrize('w', [3, 11])
def test_strand_ends(w):
    """segments of 2w + 1 records (no window) and 2w + 2 records (one); starts at 0, at w - 1 and below 0"""
    _check('strand_ends_w%d' % w)
    case, options = CASES['strand_ends_w%d' % w]
    lo, _ = R.segment_bounds(case['chrom'], case['strand'])
    for o in options:
        seg = np.searchsorted(np.unique(lo), lo[_device(case, *o)], side='left')
        assert (seg == 0).sum() == 0 and (seg == 1).sum() == 1 and (seg == 4).sum() >= 1


@pytest.mark.parametrize('w', [3, 4, 22])
def test_step_phase_follows_positions_not_indices(w):
    _check('step_phase_w%d' % w)


@pytest.mark.parametrize('w', [3, 4])
def test_ties(w):
    """values from {0.0, -0.0, 1e-300, 0.25, 0.5, 1.0}: the first occurrence of a repeated minimum, equal (key, tie-break) pairs in
    generation order, percentile 0 and 0.5 on odd and (with the base filter) even member counts"""
    _check('ties_w%d' % w)


@pytest.mark.parametrize('w', [3, 11])
def test_base_filter(w):
    """na = 'A': windows with exactly 5 (dropped), 6 and 2w + 1 contributing members, minima on bases that do not contribute,
    blanks for empty bases"""
    _check('base_filter_w%d' % w)


@pytest.mark.parametrize('w', [3, 4, 11])
def test_suppression(w):
    """WindOvlp = 1 with the best windows w - 1, w and w + 1 apart and a window blocked by the best one only: the library's
    per-position flags against the quadratic scan of the definition"""
    _check('suppression_w%d' % w)


@pytest.mark.parametrize('tag', ['w2_o1', 'w3_o1_A'])
def test_chain_on_a_ragged_golden(tag):
    """detect.region_rank on the reference's records of the four-segment ragged input gives the reference's ranked centres"""
    z = np.load(os.path.join(H.GOLDEN, 'ragged_regionrank_%s.npz' % tag))
    method = str(z['method'])
    exp, _ = H.load_expected('ragged_' + method)
    mo = {'sign_test': R.golden_records(exp, method), 'window': int(z['window']), 'WindOvlp': int(z['WindOvlp']),
          'percentile': float(z['percentile']), 'NA': str(z['NA'])}
    ranked = D.region_rank(mo, 3, 1 if str(z['rankUse']) == 'pv' else 0)
    assert mo['window'] == int(z['window_after'])
    assert [r[0][:4] for r in ranked] == list(zip(z['chrom'].tolist(), z['strand'].tolist(), z['pos'].tolist(), z['base'].tolist()))
    assert len(ranked) > 0
