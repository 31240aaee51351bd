"""CPU: every constructed position of hist_cases.py has the property its family is named for (by the numpy model of the kernels,
hist_model.py), the batches pack them as promised, and on all of them both oracles give mwu_u, ks_d and the status that the
exact integers of k1_ints.exact_ints imply — the reference of test_rank_hist_constructed_gpu.py, validated without a device."""
import numpy as np
import pytest

import hist_cases as HC
import hist_model as M
import k1_ints as K
import nanomod_oracle as orc
import oracle_c


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def test_instance_rule():
    assert M.instance_of(1, 1) == ('rank_hist', 8, 8) and M.instance_of(64, 64) == ('rank_hist', 8, 8)
    assert M.instance_of(1, 128) == ('rank_hist', 16, 8) and M.instance_of(200, 200) == ('rank_hist', 16, 16)
    assert M.instance_of(64, 256) == ('wide',) and M.instance_of(65, 256) == ('rank_hist', 16, 16)
    assert M.instance_of(512, 257) == ('rank_hist', 16, 32) and M.instance_of(1024, 1024) == ('rank_hist', 16, 64)
    assert M.instance_of(256, 1024) == ('wide',) and M.instance_of(2048, 257) == ('rank_pair', 32, 8)
    assert M.instance_of(1025, 1024) == ('rank_pair', 32, 16) and M.instance_of(2048, 2048) == ('rank_pair', 32, 32)
    assert M.instance_of(2049, 10) == ('big',)


def test_exact_ints_small():
    # a = {1, 2, 2}, b = {2, 3}: pooled 1 | 2 2 2 | 3.  |c0 n1 - c1 n0| at v = 1: |1*2 - 0| = 2, at v = 2: |3*2 - 1*3| = 3, at v = 3: 0;
    # each 2 of a has no b below it and one b equal to it; one pooled tie group of three
    assert K.exact_ints([2, 1, 2], [3, 2]) == (3, 2, 24)
    assert K.exact_ints([0.0, -0.0], [-0.0]) == (0, 2, 24) and K.mwu_u_of(2, 2, 1) == 1.0
    assert K.exact_ints([5], [7]) == (1, 0, 0) and K.exact_ints([7], [5]) == (1, 2, 0)


def _check_claim(c, d, R):
    fam, name = c['family'], c['name']
    m, q = d['m'], d['q']
    a, b = _f64(c['a']), _f64(c['b'])
    S, Q, _ = M.split(a, b)
    if fam == 'end_bin_hi':
        assert d['cntL'][m] == q == d['maxc'] and M.has_triple(Q) == ('equal' in name)
    elif fam == 'end_bin_lo':
        assert d['cntL'][0] == q == d['maxc'] and d['eq'].sum() == 0
    elif fam == 'one_bin_mid':
        k = int(np.argmax(d['cntL']))
        assert d['cntL'][k] == q and 0 < k < m and d['eq'].sum() == 0 and len(np.unique(Q)) == q
        assert (k % R == 0) == ('boundary' in name)
    elif fam == 'pairs_only':
        assert not d['general_s'] and not d['general_q']
        for x, st in ((S, d['straddle_s']), (Q, d['straddle_q'])):
            assert sum(e - s == 2 for s, e, _ in M.runs_of(x)) >= (len(x) - 2) // 2
            assert [bnd for bnd, l, r in st if (l, r) == ((R - 1,), (0,))] == list(range(R, 2 * ((len(x) - 1) // 2) + 1, R)), name
        assert (d['ab1'] > 0) == ('shared' in name)
    elif fam == 'one_triple':
        g = 'q' if '/q_' in name else 's'
        assert d['general_' + g] and not d['general_' + ('s' if g == 'q' else 'q')]
        x = Q if g == 'q' else S
        three = [(s, e) for s, e, _ in M.runs_of(x) if e - s >= 3]
        assert len(three) == 1 and three[0][1] - three[0][0] == 3
        offs = tuple(i % R for i in range(*three[0]))
        want = {'Rm2_Rm1_0': (R - 2, R - 1, 0), 'Rm1_0_1': (R - 1, 0, 1), 'midlane': (R // 2 - 1, R // 2, R // 2 + 1)}
        assert offs == [v for k, v in want.items() if k in name][0], (name, offs)
    elif fam == 'long_runs':
        if 'whole_q' in name:
            assert len(np.unique(Q)) == 1 and d['maxc'] == q and 0 < int(np.argmax(d['cntL'])) < m
        elif 'whole_s' in name:
            assert len(np.unique(S)) == 1 and d['ab1'] == m
        else:
            L, o = [int(t) for t in name.split('/')[1].replace('len', '').split('_at')]
            long = [(s, e) for s, e, _ in M.runs_of(Q) if e - s > 1]
            assert long == [(R + o, R + o + L)] and d['general_q'] and L in (R, R + 1, 2 * R + 1) and o in (0, 1, R - 1)
    elif fam == 's_runs_with_q':
        assert d['ab1'] > 0 and d['ab3'] > 0
        if 'first_key' in name or 'first_and_last' in name:
            assert d['eq'][0] > 0
        if 'last_key' in name or 'first_and_last' in name:
            assert np.sort(S)[-1] in Q
        if 'aR_bR1' in name:
            assert d['ab1'] >= R * (R + 1)
        if 'all_but_one' in name:
            assert d['ab1'] == (m - 1) * (q - 1)
    elif fam == 'all_equal':
        assert len(np.unique(np.concatenate([a, b]))) == 1 and d['ab1'] == m * q and d['ab3'] == m * q * (m + q)
    elif fam == 'all_equal_but_one':
        v, n = np.unique(np.concatenate([a, b]), return_counts=True)
        assert len(v) == 2 and min(n) == 1
        odd = v[np.argmin(n)]
        assert (odd in (S if '/s_' in name else Q)) and (odd == v[0]) == ('first' in name)
    elif fam == 'signed_zero':
        for x in (a, b):
            assert np.any((x == 0) & np.signbit(x)) and np.any((x == 0) & ~np.signbit(x)) and np.any(x > 0) and np.any(x < 0)
    elif fam == 'flt_max':
        fm = float(HC.FLT_MAX)
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
        assert np.any(np.abs(np.concatenate([a, b])) == fm)
        if 'both' in name:
            assert (S == fm).sum() == 2 and (Q == fm).sum() == 3 and (S == -fm).sum() == 1 and (Q == -fm).sum() == 2
    elif fam == 'row_neighbours':
        assert m == q == R * 8 and d['pad_s'] == 0 and d['pad_q'] == 0
    else:
        assert fam in ('size_matrix', 'full_vs_padded'), fam


def _check_reference(cases, dtype):
    """both oracles against the exact integers: U = min(u1, n0 n1 - u1), D within 4.5e-16 of the rational (and the two oracles'
    float forms equal), status MWU_ALL_IDENTICAL exactly where tie == n^3 - n"""
    idx = list(range(len(cases)))
    s0, o0, s1, o1 = HC.concat(cases, idx, dtype)
    rid = np.zeros(len(idx), np.int32)
    ec = oracle_c.detect_batch(s0, o0, s1, o1, rid, 2, 2.0, 'stouffer', tests=7)
    sc = 1e-3 if dtype == 'i16' else 1.0
    ep = orc.detect_batch(_f64(s0) * sc, o0, _f64(s1) * sc, o1, rid, 2, 2.0, orc.METHOD_STOUFFER)
    for i, c in enumerate(cases):
        a, b = HC.values(c, dtype)
        n0, n1 = len(a), len(b)
        ks_num, mwu_s, tie = K.exact_ints(a, b)
        n = n0 + n1
        ident = tie == n ** 3 - n
        for e in (ec, ep):
            assert bool(e['status'][i] & 1) == ident, c['name']
            if ident:
                assert np.isnan(e['mwu_u'][i]) and e['ks_d'][i] == 0.0
            else:
                assert e['mwu_u'][i] == K.mwu_u_of(mwu_s, n0, n1), c['name']
            assert abs(e['ks_d'][i] - ks_num / (n0 * n1)) <= K.KS_D_FLOAT_FORM_ABS, c['name']
        assert ec['ks_d'][i] == ep['ks_d'][i] and ec['status'][i] == ep['status'][i], c['name']
        if c['family'] == 'all_equal':
            assert ident and ks_num == 0 and mwu_s == n0 * n1
            if n0 == n1 == 1024:
                assert n0 * n1 * (n0 + n1) == 2 ** 31


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('inst', HC.HIST_INSTANCES, ids=lambda t: 'R%d_LG%d' % t)
def test_rank_hist_cases(inst, dtype):
    R, LG = inst
    PW = 64 // LG
    cases = HC.hist_cases(R, LG, dtype)
    fams = {c['family'] for c in cases}
    want = {'size_matrix', 'end_bin_hi', 'end_bin_lo', 'one_bin_mid', 'pairs_only', 'one_triple', 'long_runs', 's_runs_with_q',
            'all_equal', 'all_equal_but_one'} | ({'signed_zero', 'flt_max'} if dtype == 'f32' else set())
    assert fams == want
    assert len({c['name'] for c in cases}) == len(cases)
    for c in cases:
        a, b = HC.values(c, dtype)
        assert M.instance_of(len(a), len(b)) == ('rank_hist', R, LG)
        if dtype == 'f32':                                                   # exact multiples of 2^-11 (or the special values)
            for x in (a, b):
                fin = np.abs(x) < 1e30
                assert np.array_equal(np.rint(_f64(x[fin]) * 2048) / 2048, _f64(x[fin]))
        _check_claim(c, M.describe(a, b, R, LG), R)
    # the size matrix reaches both ends of the instance and both group orders
    sizes = {(len(c['a']), len(c['b'])) for c in cases if c['family'] == 'size_matrix'}
    cap = R * LG
    lo = 1 if cap <= 128 else cap // 4 + 1
    assert {(cap, cap), (cap - 1, cap), (cap, cap - 1), (lo, cap), (cap, lo), (cap // 2 + 1, cap // 2 + 1)} <= sizes
    # packing: every case at every slot of a wave; wave-mates of more than one family
    for batch in HC.split_batches(cases, PW, 400 if cap < 1024 else 100):
        assert len(batch) % PW == 0 and len(batch) <= max(400, PW * PW)
        slots = {}
        for p, i in enumerate(batch):
            slots.setdefault(i, set()).add(p % PW)
        assert all(s == set(range(PW)) for s in slots.values())
        if PW > 1:
            for w in range(0, len(batch), PW):
                assert len({cases[i]['family'] for i in batch[w:w + PW]}) > 1
    covered = set().union(*[set(bt) for bt in HC.split_batches(cases, PW, 400 if cap < 1024 else 100)])
    assert covered == set(range(len(cases)))
    if PW > 1:
        tw, without = HC.triple_waves(cases, PW)
        assert len(tw) == len(without) == 6 * PW * PW
        assert all((x == y) != (cases[x]['family'] == 'one_triple') and cases[y]['family'] == 'pairs_only' for x, y in zip(tw, without))
        for w in range(0, len(tw), PW):
            fam = [cases[i]['family'] for i in tw[w:w + PW]]
            assert fam.count('one_triple') == 1 and fam.count('pairs_only') == PW - 1
            assert len({(len(cases[i]['a']), len(cases[i]['b'])) for i in tw[w:w + PW]}) == 1
        assert {(tw[w:w + PW].index(t)) for w in range(0, len(tw), PW) for t in tw[w:w + PW] if cases[t]['family'] == 'one_triple'} == set(range(PW))
    assert (cap, cap) in HC.uniform_groups(cases) and (cap - 1, cap // 2 + 1) in HC.uniform_groups(cases)
    _check_reference(cases, dtype)


@pytest.mark.parametrize('R', [8, 16])
def test_row_neighbour_cases(R):
    cases = HC.row_neighbour_cases(R, 8)
    assert len(cases) == 16
    for c in cases:
        _check_claim(c, M.describe(c['a'], c['b'], R, 8), R)
    for x, y in zip(cases[:-1], cases[1:]):                                  # A ends in the value B begins with, in both groups
        assert x['a'].max() == x['b'].max() == y['a'].min() == y['b'].min()
        assert (x['a'] == x['a'].max()).sum() == 3 and (y['b'] == y['b'].min()).sum() == 2
    for dtype in ('f32', 'i16'):
        _check_reference(cases, dtype)


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('cls', HC.PAIR_CLASSES, ids=lambda t: 'c%d_c%d' % t)
def test_rank_pair_cases(cls, dtype):
    c0, c1 = cls
    cases = HC.pair_cases(c0, c1, dtype)
    assert len(cases) < 100 and len({c['name'] for c in cases}) == len(cases)
    C0, C1 = 64 << c0, 64 << c1
    pads = set()
    for c in cases:
        a, b = HC.values(c, dtype)
        assert M.instance_of(len(a), len(b)) == ('rank_pair', 1 << c0, 1 << c1)
        d = M.describe_pair(a, b, 1 << c0, 1 << c1)
        pads.add((d['pad0'], d['pad1']))
        if c['family'] == 'full_vs_padded':
            assert (d['pad0'], d['pad1']) in ((0, C1 - (C1 // 2 + 1)), (C0 - (C0 // 2 + 1), 0))
    # one group full and the other padded, the reverse, both full, both padded
    assert {(0, C1 // 2 - 1), (C0 // 2 - 1, 0), (0, 0), (37, 212)} == pads
    assert sum(c['family'] == 'full_vs_padded' for c in cases) == 6
    assert {'all_equal', 'all_equal_but_one', 's_runs_with_q', 'long_runs', 'pairs_only', 'one_triple'} <= {c['family'] for c in cases}
    assert M.pad_run_pp(1) == 0 and M.pad_run_pp(2) == 2 and M.pad_run_pp(4) == 0 + 2 + 6 + 12
    _check_reference(cases, dtype)


@pytest.mark.parametrize('cls', HC.PAIR_CLASSES, ids=lambda t: 'c%d_c%d' % t)
def test_rank_pair_narrow_cases(cls):
    """the int16 positions that hand rank_pair_kernel's classes to their counting forms: the probe lets every one of them in, so
    the class's gate opens whichever 64 it samples"""
    c0, c1 = cls
    cases = HC.pair_narrow_cases(c0, c1)
    assert len(cases) < 100 and len({c['name'] for c in cases}) == len(cases)
    assert {(len(c['a']), len(c['b'])) for c in cases} == set(HC.pair_sizes(c0, c1))
    far = tot = 0
    for c in cases:
        a, b = HC.values(c, 'i16')
        assert M.instance_of(len(a), len(b)) == ('rank_pair', 1 << c0, 1 << c1)
        tails = M.count_window_tails(a, b)
        assert tails <= 32 and (tails > 0) == (c['family'] == 'narrow_outliers'), (c['name'], tails)
        far += tails; tot += len(a) + len(b)
    assert far > 0 and far * 1000 <= tot * 20
    out = [c for c in cases if c['family'] == 'narrow_outliers']
    assert len(out) == 4 and all(min(c['a'].min(), c['b'].min()) == -32768 and max(c['a'].max(), c['b'].max()) == 32767 for c in out)
    _check_reference(cases, 'i16')
