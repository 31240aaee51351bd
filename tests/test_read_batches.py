"""The batches of tests/test_read_batches_gpu.py without a GPU (tests/read_batch_cases.py): the gather that stands in for running the
restatements over a whole batch is proved against them on a small tiled batch, and the distinct reads meet the conditions the GPU
gates need — every status, every content, margins from alpha and from the clip boundaries, a well-conditioned restated fit."""
import numpy as np
import pytest

import read_batch_cases as B
import readcalls_ref as Q
import rescale_ref as R

P_GATE = 1e-9                                     # tests/test_read_calls_gpu.py's gate
RESCALE_CASES = [(3, 1, 'int16'), (6, 2, 'float32'), (3, 1, 'float64')]                  # the cases of the GPU file
CALLS_CASES = [(3, 1, nb, 'int16') for nb in (0, 2, 64)] + [(6, 2, nb, 'float32') for nb in (0, 2, 64)]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _tiled(d, seed):
    D = len(d['off']) - 1
    idx = np.random.default_rng(seed).permutation(np.tile(np.arange(D), 3))
    return B.tile_batch(d['val'], d['off'], d['base'], idx)


def test_tile_batch_by_hand():
    val, off, base = np.array([10, 11, 12, 20, 30, 31], np.int16), np.array([0, 3, 3, 4, 6]), np.frombuffer(b'ACGTNA', np.uint8)
    b = B.tile_batch(val, off, base, [2, 0, 1, 3, 0])
    assert b['off'].tolist() == [0, 1, 4, 4, 6, 9] and b['ev'].tolist() == [3, 0, 1, 2, 4, 5, 0, 1, 2]
    assert b['val'].tolist() == [20, 10, 11, 12, 30, 31, 10, 11, 12] and b['val'].dtype == np.int16 and bytes(b['base']) == b'TACGNAACG'
    e = B.tile_batch(val, off, base, np.zeros(0, np.int64))
    assert e['off'].tolist() == [0] and len(e['ev']) == 0 and len(e['val']) == 0
    g = B.gather(dict(r=np.array([1, 2, 3, 4]), e=np.arange(6) * 10, margin=0.5), b['idx'], b['ev'], ('r',), ('e', 'absent'))
    assert g['r'].tolist() == [3, 1, 2, 4, 1] and g['e'].tolist() == [30, 0, 10, 20, 40, 50, 0, 10, 20] and g['margin'] == 0.5


@pytest.mark.parametrize('k,center,dtype', RESCALE_CASES[:2])
def test_rescale_restatement_agrees_with_the_gather(k, center, dtype):
    """K11's restatement run over 3 D reads in a permuted order is, bit for bit, its outputs on the D distinct reads gathered"""
    d = B.rescale_distinct(k, center, dtype)
    b = _tiled(d, 11)
    small = B.rescale_expected(k, center, dtype)
    exp = B.rescale_gather(small, b['idx'], b['ev'])
    direct = R.rescale(b['val'], b['off'], b['base'], k, center, d['mean'], d['sd'], min_events=B.RESCALE_MIN_EVENTS)
    assert len(b['idx']) == 3 * len(d['names']) and exp['clip_margin'] == direct['clip_margin']
    for f in B.RESCALE_FIELDS + ('val', 't1000'):
        assert direct[f].dtype == exp[f].dtype and _bits(direct[f]) == _bits(exp[f]), f


@pytest.mark.parametrize('k,center,nb,dtype', [(3, 1, 2, 'int16'), (6, 2, 64, 'float32')])
def test_calls_restatement_agrees_with_the_gather(k, center, nb, dtype):
    d = B.calls_distinct(k, center, nb, dtype)
    b = _tiled(d, 12)
    exp = B.calls_gather(B.calls_expected(k, center, nb, dtype), b['idx'], b['ev'])
    direct = Q.read_calls(b['val'], b['off'], b['base'], k, center, d['mean'], d['sd'], nb, B.CALLS_ALPHA)
    assert exp['alpha_margin'] == direct['alpha_margin']
    for f in B.CALLS_READ_FIELDS + B.CALLS_EVENT_FIELDS + ('W',):
        assert direct[f].dtype == exp[f].dtype and _bits(direct[f]) == _bits(exp[f]), f


@pytest.mark.parametrize('k,center,dtype', RESCALE_CASES)
def test_rescale_distinct_reads_meet_the_conditions_of_the_gpu_gates(k, center, dtype):
    """Both classes hold every failing status reachable without a huge read (int16: CLAMPED too) next to fitted reads whose shifts and
    scales differ clearly; no event lies within 1e-8 of a clip boundary; the restated fit agrees with the exact-rational one to 1e-13,
    far inside the GPU gates of 1e-11 / 1e-12; no rescaled int16 event equals the sentinel the GPU tests fill their outputs with."""
    d = B.rescale_distinct(k, center, dtype)
    exp = B.rescale_expected(k, center, dtype)
    lens = np.diff(d['off'])
    assert set(B.short_lengths(k)) <= set(lens.tolist()) and {B.WAVE_MAX + 1, B.WAVE_MAX + 1 + 512, 5000} <= set(lens.tolist())
    want = {0, R.TOO_FEW, R.DEGENERATE, R.OUT_OF_RANGE} | ({R.CLAMPED} if dtype == 'int16' else set())
    for cls in (lens <= B.WAVE_MAX, lens > B.WAVE_MAX):
        assert want <= set(exp['status'][cls].tolist()), (want, exp['status'][cls])
        ok = cls & (exp['status'] == 0)
        assert np.ptp(exp['shift'][ok]) > 0.4 and exp['scale'][ok].max() / exp['scale'][ok].min() > 1.4
    st = dict(zip(d['names'], exp['status'].tolist()))
    for tag in ('short_', 'long_'):
        assert (st[tag + 'too_few'], st[tag + 'homopolymer'], st[tag + 'negative_slope'], st[tag + 'out_of_range'], st[tag + 'clamped']) == \
            (R.TOO_FEW, R.DEGENERATE, R.DEGENERATE, R.OUT_OF_RANGE, R.CLAMPED if dtype == 'int16' else 0), st
    assert (lens[lens > B.WAVE_MAX] == B.WAVE_MAX + 1).mean() > 0.7                      # long reads are kept short
    assert 1e-8 < exp['clip_margin'] < np.inf
    fitted = 0
    for i in np.flatnonzero((exp['status'] & (R.TOO_FEW | R.DEGENERATE | R.OUT_OF_RANGE)) == 0):
        b, e = d['off'][i], d['off'][i + 1]
        x = R.to_double(d['val'][b:e])
        f = R.fit_read(x, R.read_codes(d['base'][b:e], k, center), d['mean'], d['sd'], min_events=B.RESCALE_MIN_EVENTS)
        assert f['status'] == 0 and f['scale'] == exp['scale'][i] and f['shift'] == exp['shift'][i]
        K = f['kept']
        a, s = R.exact_fit(x[K], f['mu'][K], f['w'][K])
        assert abs(f['scale'] / float(s) - 1.0) <= 1e-13 and abs(f['shift'] - float(a)) <= 1e-13, (i, f['scale'], float(s), f['shift'], float(a))
        fitted += 1
    assert fitted >= 15
    if dtype == 'int16':
        assert not (exp['val'] == np.array([0xA5A5], np.uint16).view(np.int16)[0]).any()


@pytest.mark.parametrize('k,center,nb,dtype', CALLS_CASES)
def test_calls_distinct_reads_meet_the_conditions_of_the_gpu_gates(k, center, nb, dtype):
    """No restated P lies within the p-value gate of alpha, so the counts are exact; the set holds the lengths around this nb's tile,
    reads with no eligible event, with model holes and 'N' bytes, and reads whose called fractions lie far apart"""
    d = B.calls_distinct(k, center, nb, dtype)
    exp = B.calls_expected(k, center, nb, dtype)
    assert exp['alpha_margin'] > P_GATE
    lens = np.diff(d['off'])
    inner = B.calls_inner(nb)
    assert inner == {0: 512, 2: 496, 64: 384}[nb]
    assert set(B.short_lengths(k)) | {inner - 1, inner, inner + 1} <= set(lens.tolist())
    assert {B.WAVE_MAX + 1, B.WAVE_MAX + 1 + inner, 5000} <= set(lens.tolist()) and (lens[lens > B.WAVE_MAX] == B.WAVE_MAX + 1).mean() > 0.6
    at = {n: i for i, n in enumerate(d['names'])}
    for tag in ('short_', 'long_'):
        none, clean, shifted, holes = (at[tag + n] for n in ('none_eligible', 'clean', 'shifted', 'holes'))
        assert lens[none] > 0 and exp['n_sites'][none] == 0 == exp['n_called'][none]
        assert exp['n_called'][clean] < 0.1 * exp['n_sites'][clean] and exp['n_called'][shifted] > 0.8 * exp['n_sites'][shifted] > 400
        b, e = d['off'][holes], d['off'][holes + 1]
        codes = R.read_codes(d['base'][b:e], k, center)
        assert (d['base'][b:e] == ord('N')).sum() == 3 and (codes < 0).sum() >= 3 and 0 < exp['n_sites'][holes] <= (codes >= 0).sum()
        if k == 3:                                                             # the tile runs through codes 3, 6 and 12 of the model's holes
            assert np.isin(codes, (3, 6, 9, 12)).sum() > 100 and exp['n_sites'][holes] == (~np.isin(codes, (-1, 3, 6, 9, 12))).sum()
    assert (exp['p'][~np.isnan(exp['p'])] == Q.DBL_MIN).any()                   # contaminated values reach the clamp
    assert not exp['status'].any()


@pytest.mark.parametrize('cus', [8, 256, 304])
def test_index_vectors_exceed_the_grids(cus):
    """for any CU count the batches hold more than twice as many reads of a class as the largest grid has units for it, every distinct
    read of the class is in them, and the second-pass batch puts its long reads beyond the classify grid's first stride"""
    d = B.rescale_distinct(3, 1, 'int16')
    lens = np.diff(d['off'])
    short, long_ = np.flatnonzero(lens <= B.WAVE_MAX), np.flatnonzero(lens > B.WAVE_MAX)
    for kind, ns, nl in (('short', 1, 0), ('long', 0, 1), ('mixed', 1, 1)):
        idx = B.batch_index(d['off'], kind, cus)
        is_long = lens[idx] > B.WAVE_MAX
        assert ((~is_long).sum() > 2 * B.short_units(cus)) == bool(ns) and (is_long.sum() > 2 * B.long_units(cus)) == bool(nl)
        assert set(np.unique(idx).tolist()) == set((short if ns else short[:0]).tolist()) | set((long_ if nl else long_[:0]).tolist())
        assert np.array_equal(idx, B.batch_index(d['off'], kind, cus))                  # seeded
        if kind == 'mixed':                                                     # interleaved: nearly every wave of 64 reads holds both classes
            full = is_long[:len(idx) // 64 * 64].reshape(-1, 64)
            assert (full.any(1) & ~full.all(1)).mean() > 0.95
    assert (B.short_units(256), B.long_units(256)) == (8192, 2048)
    if cus == 8:
        return
    idx = B.classify_index(d['off'], cus)
    n = len(idx)
    first_stride = B.CLASSIFY_READS_PER_CU * cus
    assert n == first_stride + B.CLASSIFY_BEYOND and B.CLASSIFY_READS_PER_CU == 4096
    where_long = np.flatnonzero(lens[idx] > B.WAVE_MAX)
    assert len(where_long) == 7 and where_long.min() >= first_stride
    assert 0.94 < (lens[idx] <= 3).mean() < 0.96 and set(short.tolist()) <= set(np.unique(idx).tolist())
    assert 2e6 < lens[idx].sum() < 8e6
