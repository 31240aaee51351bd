"""CPU: every constructed position of big_cases.py has the property its family is named for, routes to the form it is meant for
(big_cases.form_of restates classify_position), the persistent-loop batches are ordered as promised, and on every case the C
oracle gives the mwu_u, ks_d and status that the exact integers of k1_ints.exact_ints imply — the reference of
test_big_forms_constructed_gpu.py, validated without a device."""
import numpy as np
import pytest

import big_cases as B
import hist_cases as HC
import hist_model as M
import k1_ints as K
import nanomod_oracle as orc
import oracle_c


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _counts(x, v):
    return int(np.count_nonzero(_f64(x) == v))


def _check_claim(c, dtype):
    fam, name = c['family'], c['name'].split('/')[1]
    a, b = HC.values(c, dtype)
    S, Q = (_f64(b), _f64(a)) if c['order'] else (_f64(a), _f64(b))          # the roles the generator gave the groups
    assert len(S) <= len(Q)
    S = np.sort(S); m, q = len(S), len(Q)
    L, U = np.searchsorted(S, Q, 'left'), np.searchsorted(S, Q, 'right')
    pooled, cnt = np.unique(np.concatenate([S, Q]), return_counts=True)
    if fam == 'end_bin_hi':
        assert np.all(L == m) and (len(np.unique(Q)) == 1) == ('equal' in name)
    elif fam == 'end_bin_lo':
        assert np.all(U == 0) and (len(np.unique(Q)) == 1) == ('equal' in name)
    elif fam == 'two_halves':
        assert len(np.unique(S)) == len(np.unique(Q)) == 1 and S[0] != Q[0]
    elif fam == 'one_bin':
        k = int(name.split('_k')[1])
        assert np.all(L == k) and np.all(U == k) and len(np.unique(Q)) == q and 0 < k < m
        assert name.startswith('first') == (k == 1) and (k in (1, m // 2, m - 1))
    elif fam == 'pairs_only':
        for x in (S, Q):
            assert sum(e - s == 2 for s, e, _ in M.runs_of(x)) >= (len(x) - 2) // 2 and not M.has_triple(x)
        assert bool(np.any(L != U)) == ('shared' in name)
    elif fam == 'one_run':
        if name == 'whole_q':
            assert len(np.unique(Q)) == 1 and (m < 2 or (0 < L[0] < m)) and len(np.unique(S)) == m
        else:
            assert len(np.unique(S)) == 1 and len(np.unique(Q)) == q and np.count_nonzero(L != U) == 1
    elif fam == 'all_equal':
        assert len(pooled) == 1
    elif fam == 'signed_zero':
        z = np.concatenate([_f64(a), _f64(b)])
        assert np.any((z == 0) & np.signbit(z)) and np.any((z == 0) & ~np.signbit(z))
        if m >= 8:
            for x in (_f64(a), _f64(b)):
                assert np.any((x == 0) & np.signbit(x)) and np.any((x == 0) & ~np.signbit(x)) and np.any(x > 0) and np.any(x < 0)
    elif fam == 'flt_max':
        assert np.all(np.isfinite(pooled)) and np.any(np.abs(pooled) == float(HC.FLT_MAX))
    elif fam == 'stride_runs':
        Ln, where, kinds = name.split('_')
        Ln, kinds = int(Ln[1:]), kinds.split('+')
        assert Ln in (255, 256, 257, 513)
        tied = pooled[cnt > 1] if Ln > 1 else pooled
        tiles = [(_counts(S, v), _counts(Q, v)) for v in tied]
        want = [B.stride_tile(k, Ln) for k in kinds]
        if where == 'first':                                                 # tile 0 holds the smallest values of both groups
            assert tiles == [t for t in want if sum(t) > 1] and (_counts(S, pooled[0]), _counts(Q, pooled[0])) == want[0]
        else:                                                                # the last tile ends both groups
            assert tiles == [t for t in want if sum(t) > 1] and (_counts(S, pooled[-1]), _counts(Q, pooled[-1])) == want[-1]
    elif fam == 'search_fixup':
        assert len(np.unique(S)) == m
        key = S[-1] if name.startswith('last') else S[0]
        unit = S[1] - S[0]
        d = {'equal': [0], 'below': [-1], 'above': [1], 'mixed': [-1, 0, 1]}[name.split('_')[1]]
        for dd in d:
            assert _counts(Q, key + dd * unit / 4) >= q // (2 if len(d) == 1 else 4)
        if name == 'last_above':
            assert np.count_nonzero((L == m) & (U == m)) >= q // 2
        if name == 'last_equal':
            assert np.count_nonzero((L == m - 1) & (U == m)) >= q // 2
    elif fam == 'hash_table':
        assert q == 4096 and len(np.unique(Q)) == (q if 'distinct' in name else 1)
    elif fam in ('hash_chain', 'hash_wrap'):
        units = B.chain_units(dtype, fam[5:])
        keys = B.key_of(units, dtype)
        slots = B.hash_slot(keys)
        reps = [_counts(Q, float(k)) for k in keys]
        assert (reps == [1] * len(keys)) if name == 'once' else (set(reps) == {2, 3, 4, 5} and reps[0] == 2)
        if fam == 'hash_chain':
            assert len(set(slots.tolist())) == 1 and len(keys) >= 12 and len(np.unique(keys)) == len(keys)
        else:
            n0, n1 = int(np.count_nonzero(slots == B.HASH_SLOTS - 2)), int(np.count_nonzero(slots == B.HASH_SLOTS - 1))
            assert n0 + n1 == len(keys) >= 3 and n1 >= 2                     # slot 8 191 overflows into slot 0 whatever else is there
    elif fam == 'packed_bins':
        assert len(np.unique(L)) == 1 and len(np.unique(U)) == 1
        assert (L[0] != U[0]) == ('tied_run' in name) and (q == 4096 or q in (2049, 4095))
        if 'tied_run' in name:
            assert U[0] - L[0] == 7 and len(np.unique(Q)) == 1
    elif fam.startswith('redo_'):
        per = max(64, B.pow2_ceil(q)) // B.THREADS
        runs = M.runs_of(Q)
        assert not np.any(L != U)                                            # S never ties with Q
        if fam == 'redo_runs':
            Ln, t = int(name.split('_')[0][3:]), int(name.split('_at')[1])
            long = [(s, e) for s, e, _ in runs if e - s > 2 or (e - s == Ln and s == t)]
            assert (t, t + Ln) in long and all(e - s <= 2 for s, e in long if s != t) and Ln in (per, per + 1, 3 * per + 1)
            assert t % per == {'chunk_first': 0, 'chunk_last': per - 1, 'mid_chunk': per // 2}[name.split('_', 1)[1].rsplit('_at', 1)[0]]
        elif fam == 'redo_one_run':
            assert len(runs) == 1
        elif fam == 'redo_two_runs':
            assert len(runs) == 2
        elif fam == 'redo_no_ties':
            assert len(runs) == q
        assert B.redo_certain(c) == (q >= 352 and fam != 'redo_no_ties'), c['name']
    else:
        assert fam in ('random_ties', 'size_matrix'), fam


def _check_reference(cases, dtype):
    """the C oracle against the exact integers: U = min(u1, n0 n1 - u1), D within 4.5e-16 of the rational, status
    MWU_ALL_IDENTICAL exactly where tie == n^3 - n"""
    idx = list(range(len(cases)))
    s0, o0, s1, o1 = HC.concat(cases, idx, dtype)
    ec = oracle_c.detect_batch(s0, o0, s1, o1, np.zeros(len(idx), np.int32), 2, 2.0, 'stouffer', tests=7)
    for i, c in enumerate(cases):
        a, b = HC.values(c, dtype)
        n0, n1 = len(a), len(b)
        memo = c.setdefault('exact_ints', {})
        if dtype not in memo:
            memo[dtype] = K.exact_ints(a, b)
        ks_num, mwu_s, tie = memo[dtype]
        n = n0 + n1
        ident = tie == n ** 3 - n
        assert bool(ec['status'][i] & 1) == ident, c['name']
        if ident:
            assert np.isnan(ec['mwu_u'][i]) and ec['ks_d'][i] == 0.0
        else:
            assert ec['mwu_u'][i] == K.mwu_u_of(mwu_s, n0, n1), c['name']
        assert abs(ec['ks_d'][i] - ks_num / (n0 * n1)) <= K.KS_D_FLOAT_FORM_ABS, c['name']
        assert 0 <= mwu_s <= 2 * n0 * n1 and (ks_num == n0 * n1) == bool(a.max() < b.min() or b.max() < a.min())


def test_form_rule():
    assert B.form_of(2048, 2048) is None and B.form_of(2049, 1) == ('wide_big', 0) and B.form_of(256, 4096) == ('wide_big', 2)
    assert B.form_of(257, 2049) == B.form_of(4096, 1024) == 'big_hist' and B.form_of(1025, 2049) == B.form_of(1, 4097) == 'big_rank'
    assert B.form_of(2049, 2048, True) is None and B.form_of(2049, 2049, True) == 'big_rank' and B.form_of(65535, 65535) == 'big_rank'


GENERIC = {'random_ties', 'end_bin_hi', 'end_bin_lo', 'two_halves', 'pairs_only', 'one_run', 'all_equal'}


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('ks_only', [False, True], ids=['all', 'ks'])
def test_big_rank_cases(dtype, ks_only):
    batches = B.big_rank_batches(dtype, ks_only)
    want = B.BIG_RANK_KS_SIZES if ks_only else B.BIG_RANK_SIZES
    assert {s for s, _ in batches} == set(want) | {(b, a) for a, b in want}
    total = 0
    for (n0, n1), cases in batches:
        assert len({c['name'] for c in cases}) == len(cases)
        fams = {c['family'] for c in cases}
        small = n0 + n1 <= 10000
        assert {'random_ties', 'end_bin_hi', 'end_bin_lo', 'two_halves', 'one_run', 'all_equal'} <= fams
        assert ('stride_runs' in fams) == (dtype == 'f32' or max(n0, n1) < 32768)   # (the int16 domain holds no 2 x 65 535 untied values)
        if small:
            assert GENERIC <= fams and (min(n0, n1) < 2 or 'one_bin' in fams) and (dtype != 'f32' or {'signed_zero', 'flt_max'} <= fams)
            lengths = {int(c['name'].split('/')[1].split('_')[0][1:]) for c in cases if c['family'] == 'stride_runs'}
            assert lengths == {255, 256, 257, 513}
            kinds = set('+'.join(c['name'].split('/')[1].split('_')[2] for c in cases if c['family'] == 'stride_runs').split('+'))
            assert kinds == ({'1xL', 'Lx1', 'LxL', 'Lx0', '0xL'} if min(n0, n1) >= 513 else {'1xL', '0xL'})
        for c in cases:
            assert B.sizes_of(c) == (n0, n1) and B.form_of(n0, n1, ks_only) == 'big_rank'
            _check_claim(c, dtype)
        _check_reference(cases, dtype)
        total += len(cases)
    # the top of the range: ks_num beyond 2^31, mwu_s at 2 * 65 535^2, the largest tie sum
    top = dict(batches)[(65535, 65535)]
    ints = [c['exact_ints'][dtype] for c in top]
    assert max(i[0] for i in ints) == 65535 ** 2 > 2 ** 31 and max(i[1] for i in ints) == 2 * 65535 ** 2 and max(i[2] for i in ints) == 131070 ** 3 - 131070
    mixed = B.mixed_batch(batches)
    assert len(mixed) == len(batches) and len({B.sizes_of(c) for c in mixed}) == len(batches)
    print('big_rank %s %s: %d cases' % (dtype, 'ks' if ks_only else 'all', total))


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_big_hist_cases(dtype):
    """The hash chain: float32 has slots with 16 and more colliding keys among |units| < 2^19; the int16 domain's fullest home slot
    holds 12 keys (float)k — the chain asked for, and the longest there is."""
    cases = B.big_hist_cases(dtype)
    assert len({c['name'] for c in cases}) == len(cases)
    for c in cases:
        assert B.form_of(*B.sizes_of(c)) == 'big_hist', c['name']
        _check_claim(c, dtype)
    matrix = {B.sizes_of(c) for c in cases if c['family'] == 'size_matrix'}
    assert matrix == {(m, q) for m in B.BH_M for q in B.BH_Q} | {(q, m) for m in B.BH_M for q in B.BH_Q}
    assert len(B.chain_units(dtype, 'chain')) == (16 if dtype == 'f32' else 12)
    slot = B.hash_slot(B.key_of(np.arange(-32768, 32768), 'i16')).astype(np.int64)
    assert np.bincount(slot).max() == 12                                     # int16: no longer chain exists
    for m, q in B.BH_SIZES:
        fams = {c['family'] for c in cases if B.sizes_of(c) in ((m, q), (q, m))}
        assert GENERIC | {'one_bin', 'stride_runs', 'hash_chain', 'hash_wrap', 'packed_bins', 'search_fixup', 'size_matrix'} <= fams
        assert ('hash_table' in fams) == (q == 4096) and (dtype != 'f32' or {'signed_zero', 'flt_max'} <= fams)
        lengths = {int(c['name'].split('/')[1].split('_')[0][1:]) for c in cases if c['family'] == 'stride_runs' and B.sizes_of(c) in ((m, q), (q, m))}
        assert lengths == {255, 256, 257, 513}
    fix = {min(B.sizes_of(c)) for c in cases if c['family'] == 'search_fixup'}
    assert fix == {512, 1024, 511, 1023, 257, 513}                           # m == P, P - 1, P / 2 + 1
    assert {B.sizes_of(c)[0] < B.sizes_of(c)[1] for c in cases if c['family'] != 'size_matrix'} == {True, False}   # the swap
    _check_reference(cases, dtype)
    print('big_hist %s: %d cases' % (dtype, len(cases)))


@pytest.mark.parametrize('dtype', ['f32', 'g32', 'i16'])
def test_wide_big_cases(dtype):
    cases = B.wide_big_cases(dtype)
    assert len({c['name'] for c in cases}) == len(cases)
    assert {(min(B.sizes_of(c)), max(B.sizes_of(c))) for c in cases} == {(m, q) for m in B.WIDE_S for q in B.WIDE_Q}
    assert {B.sizes_of(c)[0] < B.sizes_of(c)[1] for c in cases} == {True, False}
    for c in cases:
        n0, n1 = B.sizes_of(c)
        assert B.form_of(n0, n1) == ('wide_big', M.size_class_of(min(n0, n1))), c['name']
        _check_claim(c, dtype)
        if dtype == 'g32':                                                   # on the milli-unit grid, as rank_hist.hpp's grid_key has it
            for x in HC.values(c, dtype):
                k = np.rint(x.astype(np.float64) * 1000)
                assert np.array_equal(k.astype(np.float32) / np.float32(1000.0), x) and np.abs(k).max() <= 32767
    for m in B.WIDE_S:
        assert GENERIC <= {c['family'] for c in cases if min(B.sizes_of(c)) == m}
    _check_reference(cases, dtype)
    print('wide_big %s: %d cases' % (dtype, len(cases)))


def test_wide_redo_cases():
    """What the CPU can show of the redo list: a position whose Q has 351 samples more than distinct values, with S off the grid, is
    certainly on it (big_cases.redo_certain) — every case of 2 048 samples and more but the untied one; a Q of 300 samples never
    is (the WIDE form finishes it itself) and is in the list as the issue of the kernel's sizes has it."""
    cases = B.wide_redo_cases()
    assert {(min(B.sizes_of(c)), max(B.sizes_of(c))) for c in cases} == set(B.REDO_SIZES)
    for c in cases:
        assert B.form_of(*B.sizes_of(c)) in (None, ('wide_big', M.size_class_of(min(B.sizes_of(c))))) and M.instance_of(*B.sizes_of(c)) in (('wide',), ('big',))
        _check_claim(c, 'f32')
    for m, q in B.REDO_SIZES:
        names = [c['name'].split('/')[1] for c in cases if max(B.sizes_of(c)) == q]
        per = max(64, B.pow2_ceil(q)) // 256
        for L in (per, per + 1, 3 * per + 1):
            for where in ('chunk_first', 'chunk_last') + (('mid_chunk',) if per > 2 else ()):
                assert any(n.startswith('len%d_%s_at' % (L, where)) for n in names), (q, L, where)
        assert {'whole_q', 'distinct', 'halves'} <= set(names)
    _check_reference(cases, 'f32')
    for pool in B.redo_loop_pools():
        assert len({c['family'] for c in pool}) >= 3 and all(B.redo_certain(c) and M.instance_of(*B.sizes_of(c)) == ('wide',) for c in pool)
        _check_reference(pool, 'f32')
    print('wide_redo: %d cases' % len(cases))


@pytest.mark.filterwarnings('ignore:Degrees of freedom')              # (the Python oracle's variance of a group of one sample)
def test_f64_cases():
    cases = B.f64_cases()
    redo = [c for c in cases if c['kind'] == 'redo']
    pairs = {B.sizes_of(c) for c in redo}
    assert pairs == {(x, y) for x in B.F64_SIZES for y in B.F64_SIZES} | {(x, 5) for x in B.F64_SIZES} | {(5, x) for x in B.F64_SIZES} | {B.F64_LARGE}
    assert B.form_of(*B.F64_LARGE) == 'big_rank'
    assert len([c for c in cases if c['kind'] == 'exact']) >= 5 and len([c for c in cases if c['kind'] == 'grid']) >= 5
    ties = 0
    for c in cases + B.f64_loop_pool():
        a, b = HC.values(c, 'f64')
        z = np.concatenate([a, b])
        f32_exact = np.array_equal(z.astype(np.float32).astype(np.float64), z)
        on_grid = np.array_equal(np.rint(z * 1000) / 1000.0, z)
        if c['kind'] == 'redo':                                              # class 3, every float32 image 1.0, order and ties of the units
            assert not f32_exact and not on_grid and np.all(z.astype(np.float32) == np.float32(1.0))
            assert K.exact_ints(a, b) == K.exact_ints(c['a'], c['b'])
        else:
            assert f32_exact if c['kind'] == 'exact' else on_grid
            ties += len(np.unique(z)) < len(z)
    assert ties >= 10                                                        # positions with ties that are still not redone
    assert {c['family'] for c in redo} == {c['family'] for c in B.f64_loop_pool()} == {'random_wide', 'random_narrow', 'all_equal', 'disjoint', 'pairs_shared'}
    # the Python oracle holds float64 samples (the C restatement does not): it agrees with the exact integers
    small = [c for c in cases if sum(B.sizes_of(c)) <= 600]
    s0, o0, s1, o1 = HC.concat(small, list(range(len(small))), 'f64')
    ep = orc.detect_batch(s0, o0, s1, o1, np.zeros(len(small), np.int32), 2, 2.0, orc.METHOD_STOUFFER)
    for i, c in enumerate(small):
        ks_num, mwu_s, tie = K.exact_ints(*HC.values(c, 'f64'))
        n0, n1 = B.sizes_of(c)
        if tie != (n0 + n1) ** 3 - (n0 + n1):
            assert ep['mwu_u'][i] == K.mwu_u_of(mwu_s, n0, n1)
        assert abs(ep['ks_d'][i] - ks_num / (n0 * n1)) <= K.KS_D_FLOAT_FORM_ABS
    print('f64 redo: %d cases, %d of them class 3' % (len(cases), len(redo)))


@pytest.mark.parametrize('G', [1024, 512, 416, 6])
def test_persistent_batches(G):
    """positions i and i + G (the same block's next trip) differ in family and, where the launch has two sizes, in size; the
    successions the loops' resets are about occur: all-tied behind distinct, an (almost) empty hash table behind a full one,
    small S behind large S and large again"""
    n = 2 * G + 64
    for what, pools in (('big_rank', B.big_rank_loop_pools('f32')), ('big_rank_i16', B.big_rank_loop_pools('i16')), ('big_rank_ks', B.big_rank_ks_loop_pools('f32')),
                        ('big_hist', B.big_hist_loop_pools('f32')), ('big_hist_i16', B.big_hist_loop_pools('i16')), ('f64', [B.f64_loop_pool()]),
                        ('wide_redo', B.redo_loop_pools())):
        batch = B.persistent_batch(pools, G, n, B.LOOP_AFTER)
        assert len(batch) == n
        follow = set()
        for i in range(n - G):
            x, y = batch[i], batch[i + G]
            assert x['family'] != y['family'], (what, i)
            assert len(pools) == 1 or B.sizes_of(x) != B.sizes_of(y), (what, i)
            follow.add((x['family'], y['family']))
        if len(pools) == 2:
            trips = [min(B.sizes_of(batch[i])) for i in (0, G, 2 * G)]
            assert trips[0] == trips[2] != trips[1]
        if what.startswith('big_rank') or what.startswith('big_hist'):
            assert ('end_bin_hi', 'all_equal') in follow or ('one_bin', 'all_equal') in follow
        if what.startswith('big_hist') and G >= 416:
            assert ('hash_table', 'all_equal') in follow
        if what == 'wide_redo':
            assert all(B.redo_certain(c) for c in batch)
