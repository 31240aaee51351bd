"""GPU: the ranking of K1 — the binary search every sorting form shares (ks_rank.hpp: ks_search, ks_search_tops; all
ks_rank_kernel instances, rank_hist_kernel, rank_pair_kernel) and the rounds ks_rank_kernel ranks Q in: the fixed-stride
instances rank the full rounds two at a time and the first one-per-lane round together with the last full one (eight and five
searches side by side), the generic instances four and one.  The file was written to hold a rewrite of the search level as a
masked add (v_cmpx; DESIGN_NOTES.md A.14: measured, not adopted) to the results it had; it pins every branch of the search and
every combination of rounds on constructed rows.  Every case is held against the C oracle on the same rows: KS-only ks_d bit
for bit, the status equal, ks_p within the project's 1e-9; all tests mwu_u exact and the other tracks at the gates of the
constructed all-tests files (helpers.compare_outputs, helpers.t_abs_gate).  Every position of every batch is compared, and the
dispatch statistics must count every position.

Shapes.  Values are small whole numbers (exact in float32 and as int16), so a sample equals a key exactly or not at all.
The kernel sorts the group with FEWER samples (S) and streams the other (Q); a capacity class C = R x LG holds the S of
C / 2 + 1 .. C samples (class 64: 1 .. 64).  Per class the grid is S in {1, 2, C / 2, C - 1, C} x Q in {1, LG, 4 LG, 4 LG + 1,
9 LG + 1}: where the second number is the smaller one the roles (and the class) change over — those pairs are the tail-only and
one-full-round schedules of the smaller classes — and sizes 1, 2 and C / 2 as S land in the class whose capacity they fill
(C / 2) or in class 64.  So that S = C - 1 and S = C (the FULL path: no +inf pad, a sample may rank above every key) meet real
streaming in their own class, each class also runs (C - 1, C + 1), (C, C), (C, C + 1) and (C, C + 4 LG + 1).  In full rounds and
one-per-lane rounds of Q these are (0, 1), (1, 0), (1, 1), (2, 1) from the grid and (R / 4, 0), (R / 4, 1), (R / 4 + 1, 1) from
the additions: no pair of full rounds, one, two; an odd round left over behind the pairs with and without a merged round.
  S, sorted:  distinct even keys 0, 2, 4 ... except a run of two across the first column boundary (keys R - 1, R), across the middle
              column (keys C / 2 - 1, C / 2) and across the last one that exists, and one key three times;
  Q:          a sample below every key, one equal to the smallest, one equal to the largest, one above every key, one equal to
              the triple key (positions rotate through them where Q is shorter than five), then draws over the whole key range,
              odd (between two keys) and even (on a key).
Each pair runs as fixed stride (the UNIFORM instance) and as CSR with the same rows (the generic one): all tracks bit for bit.
One CSR batch per dtype puts streamed sizes 5, 40, 300 and 1 000 against sorted groups of at most 64 next to each other: the
waves of the (8, 8) class take the cooperative schedule there (ks_search_tops).
One case per class has more positions than twice the resident waves (sixteen per compute unit at most) and more items than
those waves, so that waves go round their loop a second time; every other case has at most 4 096 positions."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

CLASSES = [(8, 8), (16, 8), (16, 16), (16, 32), (16, 64), (32, 64)]
KS_TRACKS = ('ks_d', 'ks_p', 'comb_st', 'comb_p', 'status')
ALL_TRACKS = ('mwu_u', 'mwu_p', 't_t', 't_p', 'ks_d', 'ks_p', 'comb_st', 'comb_p', 'status')


def pairs_of(R, LG):
    C = R * LG
    grid = [(s, q) for s in (1, 2, C // 2, C - 1, C) for q in (1, LG, 4 * LG, 4 * LG + 1, 9 * LG + 1)]
    return grid + [(C - 1, C + 1), (C, C), (C, C + 1), (C, C + 4 * LG + 1)]


def sorted_keys(m, R, LG):
    """the keys of S in sorted order (see the module text)"""
    k = 2 * np.arange(m, dtype=np.int64)
    joins = [R, (R * LG) // 2, ((m - 1) // R) * R]                  # key j - 1 = key j across a column boundary
    for j in joins:
        if 1 <= j < m:
            k[j - 1] = k[j]
    t = min(m // 3, max(m - 3, 0))
    if m >= 3:
        k[t] = k[t + 1] = k[t + 2] = k[t + 1]
    return np.sort(k), (int(k[t + 1]) if m >= 3 else int(k[0]))


def make_rows(m, q, R, LG, npos, rng):
    """(npos, m) and (npos, q) whole numbers"""
    keys, triple = sorted_keys(m, R, LG)
    lo, hi = int(keys[0]), int(keys[-1])
    special = np.array([lo - 3, lo, hi, hi + 3, triple], dtype=np.int64)
    s = np.tile(keys, (npos, 1))
    s = rng.permuted(s, axis=1)
    qq = rng.integers(lo - 2, hi + 3, (npos, q))
    for i in range(npos):
        take = min(q, 5)
        qq[i, :take] = np.roll(special, -i)[:take]
    qq = rng.permuted(qq, axis=1)
    return s, qq


@pytest.fixture(scope='module')
def env():
    import torch
    import nanomod_amd as nm
    import oracle_c
    L = nm._lib
    assert L.load().nmod_device_count() > 0
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {'torch': torch, 'nm': nm, 'L': L, 'oracle': oracle_c, 'det': {}, 'waves': 16 * cus}


def _detector(env, tests):
    L = env['L']
    if tests not in env['det']:
        # the sorting forms are what is checked: the counting forms (which do not search) stay out
        env['det'][tests] = env['nm'].DeviceDetector(0, nb=2, weights_dif=2.0, method='stouffer', tests=tests,
                                                     flags=L.FLAG_NO_COUNTING | L.FLAG_NO_COUNT_WIDE)
    return env['det'][tests]


def _run(env, tests, a, b, off0, off1, stride):
    torch = env['torch']
    det = _detector(env, tests)
    npos = len(off0) - 1
    n0, n1 = np.diff(off0), np.diff(off1)
    rid = torch.zeros(npos, dtype=torch.int32, device='cuda:0')
    if stride:
        res = det.run(a, b, rid, stride0=int(n0[0]), stride1=int(n1[0]), npos=npos)
    else:
        res = det.run(a, b, rid, off0=torch.from_numpy(off0).cuda(), off1=torch.from_numpy(off1).cuda(), npos=npos,
                      max_n0=int(n0.max()), max_n1=int(n1.max()))
    torch.cuda.synchronize()
    stats = det.dispatch_stats()
    tracks = ALL_TRACKS if tests == env['L'].TEST_ALL else KS_TRACKS
    return {k: res[k].cpu().numpy() for k in tracks}, stats


def _against_oracle(env, tests, got, sig0, off0, sig1, off1, what):
    npos = len(off0) - 1
    all_tests = tests == env['L'].TEST_ALL
    exp = env['oracle'].detect_batch(sig0, off0, sig1, off1, np.zeros(npos, np.int32), 2, 2.0, 'stouffer', tests=7 if all_tests else 1)
    assert got['status'].shape == (npos,) and np.array_equal(got['status'], exp['status']), (what, 'status')
    assert np.array_equal(got['ks_d'], exp['ks_d']), (what, 'ks_d', np.flatnonzero(got['ks_d'] != exp['ks_d'])[:5])
    H.assert_close_p(got['ks_p'], exp['ks_p'], 1e-9, 'ks_p')
    if all_tests:
        live = (exp['status'] & 1) == 0                              # (MWU_ALL_IDENTICAL: U and its p are NaN on both sides)
        gate = H.t_abs_gate(sig0, off0, sig1, off1)
        H.compare_outputs({k: got[k][live] for k in got}, {k: exp[k][live] for k in ALL_TRACKS}, with_comb=False, t_abs=gate[live])
        dead = ~live
        assert np.all(np.isnan(got['mwu_u'][dead])) and np.all(np.isnan(exp['mwu_u'][dead])), what
        H.assert_close_p(got['mwu_p'][dead], exp['mwu_p'][dead], 1e-9, 'mwu_p')
        H.assert_close_stat(got['t_t'][dead], exp['t_t'][dead], 1e-11, gate[dead], 't_t')
        H.assert_close_p(got['t_p'][dead], exp['t_p'][dead], 1e-9, 't_p')
    H.assert_close_stat(got['comb_st'], exp['comb_st'], 1e-9, 1e-12, 'comb_st')
    H.assert_close_p(got['comb_p'], exp['comb_p'], 1e-9, 'comb_p')


def _check_pair(env, tests, dtype, s, q, s_first, what, ks_rank_only=False):
    """rows s (npos, m) and q (npos, n) as group 0 / group 1 (s_first) or the other way round: stride, CSR, oracle"""
    torch = env['torch']
    npdt = np.float32 if dtype == 'f32' else np.int16
    g0, g1 = (s, q) if s_first else (q, s)
    npos = g0.shape[0]
    sig0 = np.ascontiguousarray(g0.astype(npdt).reshape(-1)); sig1 = np.ascontiguousarray(g1.astype(npdt).reshape(-1))
    off0 = np.arange(npos + 1, dtype=np.int64) * g0.shape[1]; off1 = np.arange(npos + 1, dtype=np.int64) * g1.shape[1]
    a = torch.from_numpy(sig0).cuda(); b = torch.from_numpy(sig1).cuda()
    strided, st_s = _run(env, tests, a, b, off0, off1, True)
    listed, st_l = _run(env, tests, a, b, off0, off1, False)
    for st in (st_s, st_l):
        assert st['positions'] == npos and st['skipped'] == 0, (what, st)
        if ks_rank_only:
            assert st['ks_rank'] == npos, (what, st)
    for k in strided:
        assert np.array_equal(strided[k].view(np.uint8), listed[k].view(np.uint8)), (what, k)
    _against_oracle(env, tests, strided, sig0, off0, sig1, off1, what)


@pytest.mark.parametrize('mode', ['ks', 'all'])
@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: '%dx%d' % c)
def test_size_grid_of_a_class(env, cls, dtype, mode):
    R, LG = cls
    L = env['L']
    tests = L.TEST_KS if mode == 'ks' else L.TEST_ALL
    pw = 64 // LG
    npos = 2 * pw + 1                                               # two full work items and one with a single position
    rng = np.random.default_rng(1000 * R + LG + (dtype == 'i16'))
    for n, (m, q) in enumerate(pairs_of(R, LG)):
        s, qq = make_rows(m, q, R, LG, npos, rng)
        _check_pair(env, tests, dtype, s, qq, n % 2 == 0, (cls, dtype, mode, m, q), ks_rank_only=(mode == 'ks'))


@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('cls', CLASSES, ids=lambda c: '%dx%d' % c)
def test_waves_take_a_second_item(env, cls, dtype):
    """KS-only, S = C - 1 against Q = C + 1: more positions than twice the resident waves and more items than waves"""
    R, LG = cls
    C = R * LG
    pw = 64 // LG
    npos = max(2, pw) * env['waves'] + 5
    rng = np.random.default_rng(77 + C)
    base = min(npos, 64)
    s, qq = make_rows(C - 1, C + 1, R, LG, base, rng)              # 64 different positions, repeated in a rotating order
    pick = (np.arange(npos) * 7) % base
    _check_pair(env, env['L'].TEST_KS, dtype, s[pick], qq[pick], True, (cls, dtype, 'second item', npos), ks_rank_only=True)


@pytest.mark.parametrize('mode', ['ks', 'all'])
@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_ragged_neighbours_take_the_cooperative_schedule(env, dtype, mode):
    """CSR: streamed sizes 5, 40, 300, 1 000 next to each other, sorted groups of 3 .. 64 samples.  Eight neighbours share a wave
    of the (8, 8) class; ranking each position's Q with its own eight lanes takes as many rounds as the longest Q (125), all 64
    lanes ranking one position after the other take 2 x (1 + 1 + 5 + 16) = 46: the wave chooses the cooperative schedule."""
    torch, L = env['torch'], env['L']
    tests = L.TEST_KS if mode == 'ks' else L.TEST_ALL
    npdt = np.float32 if dtype == 'f32' else np.int16
    rng = np.random.default_rng(5 + (dtype == 'i16'))
    npos = 8 * 37 + 3
    qs = np.array([5, 40, 300, 1000])[np.arange(npos) % 4]
    ms = np.array([64, 3, 33, 63, 5, 64, 17, 48])[(np.arange(npos) // 4) % 8]
    rows_s, rows_q = [], []
    for i in range(npos):
        s, qq = make_rows(int(ms[i]), int(qs[i]), 8, 8, 1, rng)
        rows_s.append(np.roll(s[0], i)); rows_q.append(qq[0])
    sig0 = np.concatenate(rows_s).astype(npdt); sig1 = np.concatenate(rows_q).astype(npdt)
    off0 = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64); off1 = np.concatenate([[0], np.cumsum(qs)]).astype(np.int64)
    got, st = _run(env, tests, torch.from_numpy(sig0).cuda(), torch.from_numpy(sig1).cuda(), off0, off1, False)
    assert st['positions'] == npos and st['skipped'] == 0, st
    if mode == 'ks':
        assert st['ks_rank'] == npos, st                            # the sorting form of the KS-only classes took every position
    _against_oracle(env, tests, got, sig0, off0, sig1, off1, ('ragged', dtype, mode))
