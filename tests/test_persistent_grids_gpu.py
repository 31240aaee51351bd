"""-m gpu: K8 (nmod_mix_fraction), K9 (nmod_one_sample) and K10 (nmod_kmer_model) on batches larger than their persistent grids, and the
classify kernels of K8, K9 and K14 (nmod_site_stoich) past one stride of their grid.  Every persistent loop of these entries takes its
second and third turn here: LDS words reused from one position to the next, the barrier or fence between the last read of one position
and the first store of the next, a group with no row left beside groups that have one, a short position after a long one.

The batches and what they must give are tests/grid_cases.py's (checked without a GPU in tests/test_grid_cases.py): every repeat of a pool
position has the bits of its first copy, the first copies match the numpy restatements within the gates of the entries' own GPU tests
(test_mix_gpu._check, test_one_sample_gpu._compare, test_site_stoich_gpu._check_rows, test_kmer_model_gpu._check, imported as they
are), and K10's int16 sums are exact integers.  No tolerance is new.  The sizes come from the device's CU count."""
import numpy as np
import pytest

import grid_cases as G
import kmer_ref as KR
import mix_ref as M
import one_ref as O
import stoich_ref as F
from test_kmer_model_gpu import _check as kmer_check
from test_mix_gpu import _check as mix_check
from test_one_sample_gpu import _compare as one_compare
from test_site_stoich_gpu import _check_rows as stoich_check_rows

pytestmark = pytest.mark.gpu


def _engine():
    from nanomod_amd import engine
    return engine


@pytest.fixture(scope='module')
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _sizes(what, names, counts, units):
    """print the batch sizes against the units, and assert that every class holds more than twice its units"""
    print('%s: %s' % (what, ', '.join('%s %d positions on %d units (%.2f turns)' % (n, c, u, c / u) for n, c, u in zip(names, counts, units))))
    assert all(c > 2 * u for c, u in zip(counts, units)), (what, counts, units)


def _same_as_first(what, a, rep, label=None):
    """a[i] has the bits of a[rep[i]] for every i"""
    a = np.ascontiguousarray(a)
    u = a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    bad = np.flatnonzero(u != u[rep])
    assert len(bad) == 0, '%s: %d of %d differ from their first copy; the first at %d (%r against %r at %d)%s' % (
        what, len(bad), len(a), bad[0], a[bad[0]], a[rep[bad[0]]], rep[bad[0]], '' if label is None else ', class %r' % (label[bad[0]],))


def _print_shares(what, shares):
    print('%s: worst deviation as a share of its gate: %s' % (what, ', '.join('%s %.3g' % kv for kv in sorted(shares.items())) or 'none compared'))


# --------------------------------------------------------------------------------------------------------------------------- K8

def _mix_run(b, model, **kw):
    return _engine().mix_fraction_host(b['ref'], b['roff'], b['mix'], b['moff'], mix_group=1, model=model, max_iter=G.MIX_MAX_ITER, tol=G.MIX_TOL,
                                       want_resp=True, **kw)


def _mix_verify(res, b, model, what):
    """the repeats against their first copies (resp included), the first copies against mix_ref.em through test_mix_gpu._check"""
    computed = b['cls'] >= 0
    rep = G.first_copies(np.where(computed, b['idx'], -1 - np.arange(len(computed))))
    for f in G.MIX_OUT_FIELDS:
        _same_as_first('%s %s' % (what, f), res[f], rep, b['cls'])
    _same_as_first(what + ' resp', res['resp'], G.sample_copies(b['moff'], rep))
    firsts = np.unique(rep[computed])
    x = [b['ref'][b['roff'][i]:b['roff'][i + 1]] for i in firsts]
    y = [b['mix'][b['moff'][i]:b['moff'][i + 1]] for i in firsts]
    sub = {f: res[f][firsts] for f in G.MIX_OUT_FIELDS}
    sub['resp_rows'] = [res['resp'][b['moff'][i]:b['moff'][i + 1]] for i in firsts]
    assert len(firsts) == len(np.unique(b['idx'][computed]))
    mix_check(sub, x, y, model, G.MIX_MAX_ITER, G.MIX_TOL, what)
    assert (sub['status'] == M.DEGENERATE).any() and (sub['status'] & M.NOT_CONVERGED).any() and (sub['status'] == 0).any()
    assert len(set(sub['iters'].tolist())) >= 5                                         # positions of one wave stop at different iterations
    shares = {}
    for n, (xi, yi) in enumerate(zip(x, y)):
        if sub['status'][n] & M.DEGENERATE:
            continue
        o = M.em(xi, yi, model, int(sub['iters'][n]))
        dev = dict(pi=abs(sub['pi'][n] - o['pi']) / min(1e-9 * o['pi'], 1e-12) if o['pi'] > 0.0 else 0.0,
                   sd_mod=abs(sub['sd_mod'][n] - o['sd_mod']) / (1e-9 * o['sd_mod']), mu_mod=abs(sub['mu_mod'][n] - o['mu_mod']) / (1e-9 * o['s']),
                   resp=np.abs(sub['resp_rows'][n].astype(np.float64) - o['resp']).max() / 2.0 ** -23)
        if not np.isnan(o['llr']):
            dev['llr'] = abs(sub['llr'][n] - o['llr']) / (1e-9 * abs(o['llr']) + 1e-9)
        for k, v in dev.items():
            shares[k] = max(shares.get(k, 0.0), float(v))
    _print_shares(what, shares)


@pytest.mark.parametrize('dtype,model', [('i16', M.FREE), ('f64', M.EQUAL)])
def test_mix_fraction_on_a_batch_larger_than_its_grids(cus, dtype, model):
    """2 units + 5 positions of each class, interleaved: every group of mix_em_kernel<16>, every wave of mix_em_kernel<64> and every
    workgroup of mix_stream_kernel takes a second and a third position (the sweep code is shared by the six template instances)"""
    b = G.mix_grid_batch(dtype, cus)
    _sizes('K8 %s' % dtype, ('16 lanes', 'wave', 'streaming'), [int((b['cls'] == k).sum()) for k in range(3)], G.mix_units(cus))
    res = _mix_run(b, model)
    _mix_verify(res, b, model, 'K8 grid %s model %d' % (dtype, model))


def test_mix_classify_past_one_stride(cus):
    """16 * 256 CUs + 100 000 positions, about 95 % of them left out by pos_classify_kernel<MixRule> — degenerate by size, gated off, a NaN gate —
    and the pool's positions of every class on both sides of the stride"""
    b = G.mix_classify_batch('f32', cus)
    npos, stride = len(b['idx']), G.classify_stride(cus)
    print('K8 classify: %d positions on a stride of %d (%.2f turns), %d computed' % (npos, stride, npos / stride, int((b['cls'] >= 0).sum())))
    assert npos > stride and all((b['cls'][:stride] == k).any() and (b['cls'][stride:] == k).any() for k in range(3))
    res = _mix_run(b, M.FREE, gate=b['gate'], gate_max=G.MIX_GATE_MAX)
    left = b['cls'] < 0
    assert np.array_equal(res['status'][left], np.where(b['skipped'], M.SKIPPED, M.DEGENERATE)[left].astype(np.uint8))
    assert not res['iters'][left].any() and all(np.isnan(res[f][left]).all() for f in M.FIELDS)
    ny, nr = np.diff(b['moff']), np.diff(b['roff'])
    per_sample = np.repeat(left, ny)
    assert np.isnan(res['resp'][per_sample]).all() and (res['status'][~left] & M.SKIPPED == 0).all()
    _mix_verify(res, b, M.FREE, 'K8 classify')
    # the work lists implied by the outputs: every position is left out or in the list of its size class
    out_left = ((res['status'] & M.SKIPPED) != 0) | ((res['status'] == M.DEGENERATE) & (res['iters'] == 0) & ((ny < 2) | (nr < 2)))
    lists = [int((~out_left & (G.mix_class_of(ny) == k)).sum()) for k in range(3)]
    print('K8 classify: lists of %r, %d left out' % (lists, int(out_left.sum())))
    assert lists == [int((b['cls'] == k).sum()) for k in range(3)] and sum(lists) + int(out_left.sum()) == npos


# --------------------------------------------------------------------------------------------------------------------------- K9

_one_ref_cache = {}


def _one_ref(dtype, with_n):
    """one_ref.batch over the pool of a dtype: computed once, never changed"""
    if (dtype, with_n) not in _one_ref_cache:
        pool = G.one_pool(dtype)
        _one_ref_cache[dtype, with_n] = O.batch(O.as_doubles(pool['rows']), pool['mu'], pool['sd'], pool['nr'] if with_n else None,
                                                O.MAX_ONE_F64 if dtype == 'f64' else O.MAX_ONE)
    return _one_ref_cache[dtype, with_n]


def _one_verify(res, b, dtype, with_n, what):
    rep = G.first_copies(b['idx'])
    for f in G.ONE_OUT_FIELDS:
        _same_as_first('%s %s' % (what, f), res[f], rep, b['cls'])
    firsts = np.unique(rep)
    ref = _one_ref(dtype, with_n)
    sub = {f: res[f][firsts] for f in G.ONE_OUT_FIELDS}
    exp = {f: ref[f][b['idx'][firsts]] for f in G.ONE_OUT_FIELDS}
    one_compare(sub, exp, what)
    st = exp['status']
    assert (st == O.T_NAN).any() and (st & O.BAD_REFERENCE).any() and (st == 0).sum() >= 10 and (dtype == 'i16' or (st == O.NONFINITE).any())
    ok = ~np.isnan(exp['ks_d'])
    shares = dict(ks_d=float(np.abs(sub['ks_d'][ok] - exp['ks_d'][ok]).max() / 1e-13))
    for f in ('ks_p', 't_p'):
        m = ~np.isnan(exp[f])
        shares[f] = float((np.abs(sub[f][m] - exp[f][m]) / (1e-9 * np.abs(exp[f][m]) + 1e-300)).max())
    for f in ('t_t', 'shift', 'mean', 'std'):
        m = ~np.isnan(exp[f])
        shares[f] = float((np.abs(sub[f][m] - exp[f][m]) / (1e-11 * np.abs(exp[f][m]) + 1e-12)).max())
    _print_shares(what, shares)


def _one_run(b, with_n):
    return _engine().one_sample_host(b['sig'], b['off'], b['mu'], b['sd'], b['nr'] if with_n else None, method='ks')


@pytest.mark.parametrize('with_n', [True, False])
@pytest.mark.parametrize('dtype', ['f32', 'i16', 'f64'])
def test_one_sample_on_a_batch_larger_than_its_grids(cus, dtype, with_n):
    """2 units + 5 positions of each class (float64: of the workgroup class, which takes them all), row lengths mixed within a class:
    a wave's LDS keys are stored again while its neighbours still hold theirs, and one_block_kernel's 64 KiB serve the reduction words and
    the sort keys of one position after the other, paddings of 4 096 and 8 192 (float64: 64 .. 512 and 4 096) in turn"""
    b = G.one_grid_batch(dtype, cus, with_n)
    names, units = ('16 lanes', 'wave x 16', 'wave x 32', 'workgroup'), G.one_units(cus)
    counts = [int((b['cls'] == k).sum()) for k in range(4)]
    if dtype == 'f64':
        assert counts[:3] == [0, 0, 0]
        names, units, counts = names[3:], units[3:], counts[3:]
    _sizes('K9 %s' % dtype, names, counts, units)
    res = _one_run(b, with_n)
    _one_verify(res, b, dtype, with_n, 'K9 grid %s %s' % (dtype, 'control' if with_n else 'model'))


def test_one_sample_classify_past_one_stride(cus):
    b = G.one_classify_batch('f32', cus, True)
    npos, stride = len(b['idx']), G.classify_stride(cus)
    print('K9 classify: %d positions on a stride of %d (%.2f turns), %d computed' % (npos, stride, npos / stride, int((b['cls'] >= 0).sum())))
    assert npos > stride and all((b['cls'][:stride] == k).any() and (b['cls'][stride:] == k).any() for k in range(4))
    res = _one_run(b, True)
    left = b['cls'] < 0
    lens = np.diff(b['off'])
    want = (np.where(lens == 0, O.EMPTY, 0) | np.where(~(b['sd'] > 0.0) | (b['nr'] < 2), O.BAD_REFERENCE, 0)).astype(np.uint8)
    assert want[left].all() and np.array_equal(res['status'][left], want[left]) and all(np.isnan(res[f][left]).all() for f in O.FIELDS)
    _one_verify(res, b, 'f32', True, 'K9 classify')
    out_left = (res['status'] & (O.EMPTY | O.TOO_LARGE | O.BAD_REFERENCE)) != 0
    lists = [int((~out_left & (G.one_class_of(lens, 'f32') == k)).sum()) for k in range(4)]
    print('K9 classify: lists of %r, %d left out' % (lists, int(out_left.sum())))
    assert lists == [int((b['cls'] == k).sum()) for k in range(4)] and sum(lists) + int(out_left.sum()) == npos


# -------------------------------------------------------------------------------------------------------------------------- K14

def test_site_stoich_classify_past_one_stride(cus):
    """about 95 % rows of 0 .. 2 scores (TOO_FEW at once), the pool's rows of every class on both sides of the stride"""
    b = G.stoich_classify_batch(cus)
    pool = G.stoich_pool()
    npos, stride = len(b['idx']), G.classify_stride(cus)
    print('K14 classify: %d rows on a stride of %d (%.2f turns), %d of more than 2 scores' % (npos, stride, npos / stride, int((b['cls'] >= 0).sum())))
    assert npos > stride and all((b['cls'][:stride] == k).any() and (b['cls'][stride:] == k).any() for k in range(3))
    got = _engine().site_stoich_host(b['score'], b['off'], min_valid=G.STOICH_MIN_VALID, resp=True)
    left = b['cls'] < 0
    n_valid = np.array([int(np.isfinite(r).sum()) for r in pool['rows']])
    assert (got['status'][left] == F.TOO_FEW).all() and not got['iters'][left].any() and np.array_equal(got['n_valid'][left], n_valid[b['idx']][left])
    assert all(np.isnan(got[f][left]).all() for f in F.FIELDS) and np.isnan(got['resp'][np.repeat(left, np.diff(b['off']))]).all()
    rep = G.first_copies(b['idx'])
    for f in G.STOICH_OUT_FIELDS:
        _same_as_first('K14 classify ' + f, got[f], rep, b['cls'])
    _same_as_first('K14 classify resp', got['resp'], G.sample_copies(b['off'], rep))
    firsts = np.unique(rep).tolist()
    assert len(firsts) == len(pool['rows'])
    exp = {i: F.row(b['score'][b['off'][i]:b['off'][i + 1]], min_valid=G.STOICH_MIN_VALID) for i in firsts}
    stoich_check_rows(got, exp, b['off'], rows=firsts)
    lens = np.diff(b['off'])
    by_len = np.where(lens <= F.SMALL, 0, np.where(lens <= F.WAVE, 1, 2))
    lists = [int((by_len == k).sum()) for k in range(3)]                                # (no row here is TOO_LARGE: every row is in a list)
    few = int((got['status'] == F.TOO_FEW).sum())
    print('K14 classify: lists of %r, %d rows with too few scores' % (lists, few))
    assert not (got['status'] & F.TOO_LARGE).any() and sum(lists) == npos and few == int(left.sum())
    assert lists[1:] == [int((b['cls'] == k).sum()) for k in (1, 2)] and lists[0] == int((b['cls'] <= 0).sum())


# -------------------------------------------------------------------------------------------------------------------------- K10

def _kmer_shares(what, got, exp, gate):
    shares = {}
    for f in ('mean', 'sd'):
        m = ~np.isnan(exp[f])
        err, g = np.abs(got[f][m] - exp[f][m]), gate(np.abs(exp[f][m]))
        share = np.where(g > 0.0, err / np.where(g > 0.0, g, 1.0), np.where(err > 0.0, np.inf, 0.0))      # (an sd of 0 is matched as it is)
        shares[f] = float(share.max()) if m.any() else 0.0
    _print_shares(what, shares)


@pytest.mark.parametrize('ncodes,bounds,stride', [(64, False, 0), (65536, False, 0), (4096, True, 0), (64, False, 5)],
                         ids=['lds-table', 'global-table', 'clip-4096', 'stride'])
def test_kmer_model_i16_on_a_batch_larger_than_its_grid(cus, ncodes, bounds, stride):
    """more than two tiles of 64 positions for every wave of km_i16_kernel: its per-wave LDS words are stored again after the tile's last
    km_wave_sync, and the LDS table gathers several tiles per wave before its flush.  Counts and pos_status exact, mean and sd within
    1e-14 relative of the exact rational values"""
    units = G.km_i16_positions(cus, ncodes)
    npos = G.kmer_grid_npos(cus, ncodes)
    b = G.kmer_batch(npos, ncodes, 10000 + ncodes + stride, stride=stride, bounds=bounds)
    _sizes('K10 int16 ncodes %d' % ncodes, ('positions',), (npos,), (units,))
    assert npos % G.KM_TILE != 0 and len(b['sig']) < 2 ** 33
    got = _engine().kmer_model_host(b['sig'], b['off'], b['code'], ncodes, b['keep_lo'], b['keep_hi'], stride=stride)
    exp = G.kmer_expected_i16(b['sig'], b['lens'], b['code'], ncodes, b['keep_lo'], b['keep_hi'])
    assert exp['n_samples'].sum() > 0.9 * len(b['sig']) * (0.5 if bounds else 1.0) and (not bounds or exp['n_clipped'].sum() > 0)
    kmer_check(got, exp, np.int16, 'K10 grid int16 ncodes=%d' % ncodes)
    _kmer_shares('K10 int16 ncodes %d' % ncodes, got, exp, lambda e: 1e-14 * e)


@pytest.mark.parametrize('ncodes', [64, 4096])
@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_kmer_model_float_on_a_batch_larger_than_its_grid(cus, dt, ncodes):
    """more than two positions for every wave of km_moments_kernel, against kmer_ref.kmer_model directly"""
    dtype = G.NP_DTYPE[dt]
    npos = G.kmer_float_npos(cus)
    _sizes('K10 %s ncodes %d' % (dt, ncodes), ('positions',), (npos,), (G.km_moments_units(cus),))
    rows, code = G.kmer_float_rows(npos, ncodes, dtype, 20000 + ncodes)
    sig, off = KR.csr(rows, dtype)
    got = _engine().kmer_model_host(sig, off, code, ncodes)
    exp = KR.kmer_model(rows, code, ncodes, dtype)
    assert (exp['pos_status'] == KR.NONFINITE).sum() >= 2
    kmer_check(got, exp, dtype, 'K10 grid %s ncodes=%d' % (dt, ncodes))
    _kmer_shares('K10 %s ncodes %d' % (dt, ncodes), got, exp, lambda e: 1e-11 * e + 1e-12)
