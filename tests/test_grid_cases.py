"""The batches of tests/test_persistent_grids_gpu.py without a GPU (tests/grid_cases.py): the builders exceed the grids for any CU count,
the repeat builder round-trips, the vectorised K10 expectation is kmer_ref.kmer_model's bit for bit, and the pools meet the conditions
the GPU gates need — checked on the restatements alone."""
import numpy as np
import pytest

import grid_cases as G
import kmer_ref as KR
import mix_ref as M
import one_ref as O
import stoich_ref as F


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _odd_count(n, units):
    return n > 2 * units and n % 4 != 0 and n % 16 != 0


def test_tile_rows_by_hand():
    val, off = np.array([10, 11, 12, 20, 30, 31], np.int16), np.array([0, 3, 3, 4, 6])
    b = G.tile_rows(val, off, [2, 0, 1, 3, 0])
    assert b['off'].tolist() == [0, 1, 4, 4, 6, 9] and b['ev'].tolist() == [3, 0, 1, 2, 4, 5, 0, 1, 2]
    assert b['val'].tolist() == [20, 10, 11, 12, 30, 31, 10, 11, 12] and b['val'].dtype == np.int16
    e = G.tile_rows(val, off, np.zeros(0, np.int64))
    assert e['off'].tolist() == [0] and len(e['ev']) == 0 and len(e['val']) == 0
    rep = G.first_copies(b['idx'])
    assert rep.tolist() == [0, 1, 2, 3, 1]
    assert G.sample_copies(b['off'], rep).tolist() == [0, 1, 2, 3, 4, 5, 1, 2, 3]
    assert G.first_copies(np.array([5, -1, 5, -1, 7])).tolist() == [0, 1, 0, 1, 4]


@pytest.mark.parametrize('dtype', ['i16', 'f32', 'f64'])
def test_tiling_round_trips(dtype):
    """every row of a tiled batch is its pool row, for both inputs of K8 and for K9's rows and reference; the first copies are the first"""
    pool = G.mix_pool(dtype)
    idx = np.random.default_rng(3).permutation(np.tile(np.arange(len(pool['cls'])), 3))
    b = G.mix_tile(pool, idx)
    for i, j in enumerate(idx.tolist()):
        assert _bits(b['ref'][b['roff'][i]:b['roff'][i + 1]]) == _bits(pool['ref_rows'][j]) and b['ref'].dtype == pool['ref_rows'][j].dtype
        assert _bits(b['mix'][b['moff'][i]:b['moff'][i + 1]]) == _bits(pool['mix_rows'][j])
    rep = G.first_copies(idx)
    assert np.array_equal(idx[rep], idx) and (rep <= np.arange(len(idx))).all() and len(np.unique(rep)) == len(pool['cls'])
    assert all(rep[i] == idx.tolist().index(j) for i, j in enumerate(idx.tolist()))
    ev = G.sample_copies(b['moff'], rep)
    assert _bits(b['mix'][ev]) == _bits(b['mix']) and (ev <= np.arange(len(ev))).all()
    one = G.one_pool(dtype)
    idx = np.random.default_rng(4).permutation(np.tile(np.arange(len(one['lens'])), 2))
    t = G.one_tile(one, idx)
    for i, j in enumerate(idx.tolist()):
        assert _bits(t['sig'][t['off'][i]:t['off'][i + 1]]) == _bits(one['rows'][j])
    assert _bits(t['mu']) == _bits(one['mu'][idx]) and _bits(t['sd']) == _bits(one['sd'][idx]) and _bits(t['nr']) == _bits(one['nr'][idx])
    assert t['nr'].dtype == np.int32 and t['sig'].dtype == G.NP_DTYPE[dtype]


@pytest.mark.parametrize('cus', [1, 2])
def test_every_builder_exceeds_the_grids(cus):
    """more than twice the units of every class, counts that are no multiple of 4 or 16, every pool position of a class present, the
    classes interleaved; the classify batches reach past one stride with every class on both sides of it"""
    assert G.mix_units(256) == (32768, 8192, 512) and G.one_units(256) == (32768, 8192, 8192, 512) and G.stoich_units(256) == (32768, 8192, 512)
    assert (G.km_i16_positions(256, 64), G.km_i16_positions(256, 65536), G.km_moments_units(256)) == (262144, 524288, 8192)
    assert G.classify_stride(256) == 1048576
    for dtype in ('i16', 'f64'):
        pool, b = G.mix_pool(dtype), G.mix_grid_batch(dtype, cus)
        ny = np.diff(b['moff'])
        assert np.array_equal(G.mix_class_of(ny), b['cls']) and np.array_equal(b['cls'], pool['cls'][b['idx']])
        for k, u in enumerate(G.mix_units(cus)):
            assert _odd_count(int((b['cls'] == k).sum()), u), (dtype, k)
            have, want = set(b['idx'][b['cls'] == k].tolist()), set(np.flatnonzero(pool['cls'] == k).tolist())
            assert have == want or (have < want and len(have) == 2 * u + 5)             # (fewer than 16 where the grid is that small)
        lo, hi = zip(*G.MIX_Y_LENGTHS)
        assert (ny >= np.array(lo)[b['cls']]).all() and (ny <= np.array(hi)[b['cls']]).all()
        nr = np.diff(b['roff'])
        assert nr.min() == 5 and nr.max() == 60
        head = b['cls'][:len(b['cls']) // 64 * 64].reshape(-1, 64)
        assert ((head == 0).any(1) & (head == 1).any(1)).mean() > 0.9                  # interleaved
    for dtype in ('f32', 'i16', 'f64'):
        for with_n in (True, False):
            pool, b = G.one_pool(dtype), G.one_grid_batch(dtype, cus, with_n)
            lens = np.diff(b['off'])
            cls = G.one_pool_class(pool, dtype, with_n)
            computed = b['cls'] >= 0
            assert np.array_equal(G.one_class_of(lens, dtype)[computed], b['cls'][computed]) and (~computed).sum() >= 9
            for k, u in enumerate(G.one_units(cus)):
                n = int((b['cls'] == k).sum())
                assert (n == 0 and dtype == 'f64' and k < 3) or _odd_count(n, u), (dtype, k, n)
                have, want = set(b['idx'][b['cls'] == k].tolist()), set(np.flatnonzero(cls == k).tolist())
                assert have == want or (have < want and len(have) == n)
    for ncodes in (64, 4096, 65536):
        n = G.kmer_grid_npos(cus, ncodes)
        assert n > 2 * G.km_i16_positions(cus, ncodes) and n % G.KM_TILE != 0
    assert G.km_i16_positions(cus, 4096) == 1024 * cus and G.km_i16_positions(cus, 4097) == 2048 * cus
    assert _odd_count(G.kmer_float_npos(cus), G.km_moments_units(cus))
    # the classify batches
    stride, n = G.classify_stride(cus), G.classify_stride(cus) + G.CLASSIFY_BEYOND
    m = G.mix_classify_batch('f32', cus)
    o = G.one_classify_batch('f32', cus, True)
    s = G.stoich_classify_batch(cus)
    for b, cls, nclass in ((m, m['cls'], 3), (o, o['cls'], 4), (s, s['cls'], 3)):
        assert len(cls) == n == len(b['idx'])
        assert 0.93 < (cls < 0).mean() < 0.96
        for k in range(nclass):
            assert (cls[:stride] == k).any() and (cls[stride:] == k).any(), k
    assert np.array_equal(m['skipped'] | m['by_size'], m['cls'] < 0) and not (m['skipped'] & m['by_size']).any()
    assert not (m['gate'][m['skipped']] <= G.MIX_GATE_MAX).any() and np.isnan(m['gate'][m['skipped']]).mean() > 0.3
    assert (m['gate'][~m['skipped']] <= G.MIX_GATE_MAX).all() and (m['gate'][m['cls'] >= 0] == G.MIX_GATE_MAX).any()
    ny, nr = np.diff(m['moff']), np.diff(m['roff'])
    assert ((ny < 2) | (nr < 2))[m['by_size']].all() and not ((ny < 2) | (nr < 2))[m['cls'] >= 0].any() and (m['skipped'] & (ny >= 2) & (nr >= 2)).any()
    assert (o['left'] == (o['cls'] < 0)).all() and (s['left'] == (s['cls'] < 0)).all()
    lens = np.diff(o['off'])
    assert ((lens == 0) | ~(o['sd'] > 0.0) | (o['nr'] < 2))[o['cls'] < 0].all() and (lens[o['cls'] < 0] == 0).any() and (o['sd'][o['cls'] < 0] == 0.0).any()
    assert (np.diff(s['off'])[s['cls'] < 0] <= 2).all() and set(np.diff(s['off'])[s['cls'] < 0].tolist()) == {0, 1, 2}


def test_one_sample_rows_share_their_units_as_intended():
    """with the work lists in position order (the order the classifier gives but for the interleaving of its waves): in the workgroup class
    a padding of 4 096 follows one of 8 192 on the same workgroup and the reverse, each on more than a tenth of the workgroups; in the
    16-lane class a 3-sample row shares a wave with a 256-sample one on many waves.  At 32 CUs: enough rows for the shares to show"""
    cus = 32
    b = G.one_grid_batch('f32', cus, True)
    lens = np.diff(b['off'])
    units = G.one_units(cus)
    rows = lens[b['cls'] == 3]
    P = np.array([G.block_padding(int(n)) for n in rows])
    assert set(P.tolist()) == {4096, 8192}
    a, c = P[:len(P) - units[3]], P[units[3]:]                                          # turn t and turn t + 1 of the same workgroup
    assert ((a == 8192) & (c == 4096)).sum() > 0.1 * units[3] and ((a == 4096) & (c == 8192)).sum() > 0.1 * units[3]
    small = lens[b['cls'] == 0]
    w = small[:len(small) // 4 * 4].reshape(-1, 4)
    both = ((w == 3).any(1) & (w == 256).any(1)).sum()
    assert both >= 20, both
    assert small.min() == 1 and small.max() == 256 and lens[b['cls'] == 1].min() == 257 and lens[b['cls'] == 1].max() == 400
    assert lens[b['cls'] == 2].min() == 1025 and lens[b['cls'] == 2].max() == 1100 and set(rows.tolist()) >= {2049, 2200, 5000}
    f = G.one_grid_batch('f64', cus, True)
    fl = np.diff(f['off'])[f['cls'] == 3]
    Pf = np.array([G.block_padding(int(n)) for n in fl])
    a, c = Pf[:len(Pf) - units[3]], Pf[units[3]:]
    assert {2, 300, 3000} <= set(fl.tolist()) and ((a == 4096) & (c < 4096)).any() and ((a < 4096) & (c == 4096)).any()


@pytest.mark.parametrize('ncodes,bounds,stride', [(64, False, 0), (4096, True, 0), (5000, False, 0), (64, True, 5), (64, False, 7)])
def test_the_vectorised_kmer_expectation_is_the_restatements(ncodes, bounds, stride):
    """a few thousand positions with every kind of row the big batches hold: 1 .. 11 samples, empty rows, codes of -1, absent codes, rows of
    513 and 4 097 samples, samples exactly on a keep bound, a NaN bound, a one-sided bound, a single kept value"""
    b = G.kmer_batch(3001, ncodes, 77 + ncodes, stride=stride, bounds=bounds)
    lens = b['lens']
    off = np.r_[0, np.cumsum(lens)]
    if not stride:
        assert (lens == 0).sum() > 10 and sorted(lens[lens > 11].tolist()) == sorted(G.KM_LONG_ROWS) and set(range(1, 12)) <= set(lens.tolist())
        assert np.array_equal(off, b['off'])
    assert (b['code'] == -1).sum() > 10 and np.abs(b['sig'].astype(np.int64)).max() == 32767 and not (b['code'] == 7).any()
    rows = [b['sig'][off[i]:off[i + 1]] for i in range(len(lens))]
    got = G.kmer_expected_i16(b['sig'], lens, b['code'], ncodes, b['keep_lo'], b['keep_hi'])
    exp = KR.kmer_model(rows, b['code'], ncodes, np.int16, b['keep_lo'], b['keep_hi'])
    for f in exp:
        assert got[f].dtype == exp[f].dtype and _bits(got[f]) == _bits(exp[f]), f
    assert (exp['pos_status'] == KR.EMPTY).any() == (not stride) and (exp['pos_status'] & KR.NO_CODE).any()
    if bounds:
        lo, hi = b['keep_lo'], b['keep_hi']
        d = b['sig'].astype(np.float64) / 1000.0
        c = np.repeat(b['code'], lens)
        assert exp['n_clipped'].sum() > 0 and ((c >= 0) & (d == lo[np.maximum(c, 0)])).any() and ((c >= 0) & (d == hi[np.maximum(c, 0)])).any()
        assert exp['n_samples'][3] == 0 and exp['n_clipped'][3] > 0 and np.isnan(exp['mean'][3]) and exp['n_positions'][3] == 0
        assert lo[6] == hi[6] and (exp['n_samples'][6] == 0 or exp['sd'][6] == 0.0)


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_the_float_kmer_rows(dtype):
    rows, code = G.kmer_float_rows(G.kmer_float_npos(2), 64, G.NP_DTYPE[dtype], 5)
    st = np.array([KR.position_status(r, int(c), 64, G.NP_DTYPE[dtype]) for r, c in zip(rows, code)])
    assert (st == KR.NONFINITE).sum() >= 2 and (st == KR.EMPTY).any() and (st & KR.NO_CODE).any() and (st == 0).mean() > 0.9
    assert all(r.dtype == G.NP_DTYPE[dtype] for r in rows[:5])


@pytest.mark.parametrize('dtype,model', [('i16', M.FREE), ('f64', M.EQUAL)])
def test_the_mix_pool_meets_the_conditions_of_the_gpu_gates(dtype, model):
    """The cases of the GPU file.  Every class holds its shortest and longest |Y|, the planted fractions, a constant reference group and
    (float) a NaN; the other positions are computed by the restatement, stop at different iterations within a class, and NO delta of
    any iteration up to the stop lies in _check's band of 1e-6 tol around tol: the device, which follows the restatement to 1e-9, stops
    where it does, and none of the first copies needs _check's 1 % allowance.  fp64 numpy and 40-digit mpmath agree to 1e-11 at equal
    iteration counts on the 16-lane class and on two positions of each other class (the pin of tests/test_mix.py, on these shapes)."""
    import mpmath as mp
    pool = G.mix_pool(dtype)
    kinds = np.array(pool['kind'])
    worst = 0.0
    for k, (lo, hi) in enumerate(G.MIX_Y_LENGTHS):
        ids = np.flatnonzero(pool['cls'] == k)
        ny = np.array([len(pool['mix_rows'][i]) for i in ids])
        assert len(ids) == G.MIX_PER_CLASS and ny.min() == lo and ny.max() == hi
        assert (kinds[ids] == 'constant_ref').sum() == 1 and (kinds[ids] == 'nan').sum() == (dtype != 'i16')
        iters = []
        for n, i in enumerate(ids.tolist()):
            x, y = pool['ref_rows'][i], pool['mix_rows'][i]
            assert 5 <= len(x) <= 60
            if kinds[i] != 'planted':
                assert M.degenerate_by_input(x, y) and len(x) >= 2 and len(y) >= 2
                continue
            assert not M.degenerate_by_input(x, y)
            own = M.run(x, y, model, max_iter=G.MIX_MAX_ITER, tol=G.MIX_TOL)
            assert own['status'] & M.DEGENERATE == 0 and 1 <= own['iters'] <= G.MIX_MAX_ITER
            for it in range(1, own['iters'] + 1):
                dl = M.em(x, y, model, it)['delta']
                assert abs(dl - G.MIX_TOL) > 1e-6 * G.MIX_TOL, (k, i, it, dl)
            iters.append(own['iters'])
            if k == 0 or n < 2:
                a, b = M.em(x, y, model, own['iters']), M.em_mp(x, y, model, own['iters'])
                with mp.workdps(40):
                    dev = [abs(a['pi'] - b['pi']) / b['pi'] if b['pi'] > 0 else abs(a['pi']), abs(a['sd_mod'] - b['sd_mod']) / b['sd_mod'],
                           abs(a['mu_mod'] - b['mu_mod']) / b['s']]
                    if np.isfinite(a['llr']):
                        dev.append(abs(a['llr'] - b['llr']) / (abs(b['llr']) + 1))
                    worst = max(worst, max(float(v) for v in dev))
        assert len(set(iters)) >= 3 and max(iters) == G.MIX_MAX_ITER, iters            # the null positions run into max_iter
    print('numpy against 40-digit mpmath on the pool, %s model %d: %.3g' % (dtype, model, worst))
    assert worst <= 1e-11
    tiny = np.flatnonzero(pool['cls'] < 0)
    assert all(min(len(pool['ref_rows'][i]), len(pool['mix_rows'][i])) < 2 for i in tiny) and len(tiny) == len(G.MIX_TINY)


@pytest.mark.parametrize('dtype', ['f32', 'i16', 'f64'])
def test_the_one_sample_pool_holds_every_kind(dtype):
    pool = G.one_pool(dtype)
    cap = O.MAX_ONE_F64 if dtype == 'f64' else O.MAX_ONE
    dbl = O.as_doubles(pool['rows'])
    at = {}
    for i, name in enumerate(pool['kind']):
        at.setdefault(name, []).append(i)
    for with_n in (True, False):
        ref = O.batch(dbl, pool['mu'], pool['sd'], pool['nr'] if with_n else None, cap)
        st = ref['status']
        assert (st[at['plain']] == 0).all() and (st[at['one_sample']] == O.T_NAN).all()
        assert (st[at['nonfinite']] == (0 if dtype == 'i16' else O.NONFINITE)).all()
        assert (st[at['sd_zero'] + at['sd_nan']] == O.BAD_REFERENCE).all() and st[at['empty'][0]] == O.EMPTY
        assert st[at['ref_n_one'][0]] == (O.BAD_REFERENCE if with_n else 0)
        left = G.one_pool_class(pool, dtype, with_n) < 0
        assert np.array_equal(left, (st & (O.BAD_REFERENCE | O.EMPTY | O.TOO_LARGE)) != 0)
        assert (np.abs(ref['shift'][st == 0]) > 0.5).any() and (np.abs(ref['shift'][st == 0]) < 0.2).any()
    want = set(G.ONE_LENGTHS_F64) if dtype == 'f64' else {n for v in G.ONE_LENGTHS.values() for n in v}
    assert want <= set(pool['lens'].tolist())


def test_the_stoich_pool_holds_every_class_and_rows_that_are_too_few():
    pool = G.stoich_pool()
    exp = [F.row(r, min_valid=G.STOICH_MIN_VALID) for r in pool['rows']]
    for i, e in enumerate(exp):
        assert (e['status'] == F.TOO_FEW) == (pool['cls'][i] < 0), i
    assert [e['n_valid'] for e, c in zip(exp, pool['cls']) if c < 0] == [0, 1, 1, 2, 2, 1]
    for k, n in enumerate(G.STOICH_LENGTHS):
        rows = [e for e, c in zip(exp, pool['cls']) if c == k]
        assert len(rows) == G.STOICH_PER_CLASS and all(e['gates'] is not None for e in rows) and sum(e['status'] == 0 for e in rows) >= 8
    assert np.array_equal(np.where(pool['lens'] <= F.SMALL, 0, np.where(pool['lens'] <= F.WAVE, 1, 2))[pool['cls'] >= 0], pool['cls'][pool['cls'] >= 0])
