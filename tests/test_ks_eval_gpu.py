"""The KS kernels' bin evaluation and float-form pass on the device: ks_d bit for bit against ks_2samp's D at the
smallest shapes that reach each kernel instance and edge (KS only and all tests, float32 and int16, CSR and fixed
stride), and positions constructed to exercise the float-form pass — each proven to do so by the numpy model of the
kernel (ks_model.py)."""
import numpy as np
import pytest

import helpers as H
import ks_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def nm():
    import nanomod_amd
    return nanomod_amd


def _csr(sizes):
    off = np.zeros(len(sizes) + 1, np.int64)
    off[1:] = np.cumsum(sizes)
    return off


def _fill(rng, sizes0, sizes1, grid3_every=0):
    """milli-unit int16 keys: every third position continuous (few ties), the others on a grid of 2 .. 40 values, and
    with grid3_every every position on a 3-value grid; some positions get a shifted second group"""
    a, b = [], []
    for i, (n0, n1) in enumerate(zip(sizes0, sizes1)):
        if grid3_every:
            g = 3
        else:
            g = 0 if i % 3 == 0 else int(rng.integers(2, 41))
        shift = int(rng.integers(0, 3)) if g else (400 if i % 7 == 0 else 0)
        if g:
            a.append(rng.integers(0, g, n0) * 10)
            b.append((rng.integers(0, g, n1) + (shift if i % 5 == 0 else 0)) * 10)
        else:
            a.append(rng.integers(-3000, 3001, n0))
            b.append(rng.integers(-3000, 3001, n1) + shift)
    return np.concatenate(a).astype(np.int16), np.concatenate(b).astype(np.int16)


def _case(name):
    """-> (int16 keys of group 0, of group 1, sizes0, sizes1, fixed stride possible)"""
    rng = np.random.default_rng(sum(name.encode()))
    if name == 'tiny':                       # (m, q) in {1..8} x {1..20}, each pair 6 times, the groups in either order
        pairs = [(m, q) for m in range(1, 9) for q in range(1, 21)] * 6
        s0 = np.array([p[i % 2] for i, p in enumerate(pairs)]); s1 = np.array([p[1 - i % 2] for i, p in enumerate(pairs)])
    elif name == 'cap128':                   # 65 .. 70 v 65 .. 140
        s0 = rng.integers(65, 71, 400); s1 = rng.integers(65, 141, 400)
    elif name == 'cap256':                   # 129 .. 140 v 129 .. 260
        s0 = rng.integers(129, 141, 300); s1 = rng.integers(129, 261, 300)
    elif name == 'grid3_200v200':            # four positions per wave, all on a 3-value grid
        s0 = np.full(256, 200); s1 = np.full(256, 200)
    elif name == 'full_256v256':             # a group that fills its capacity: no +inf pad
        s0 = np.full(128, 256); s1 = np.full(128, 256)
    elif name == 'cap512':                   # 257 .. 260 v 300
        s0 = rng.integers(257, 261, 200); s1 = np.full(200, 300)
    else:
        raise KeyError(name)
    k0, k1 = _fill(rng, s0, s1, grid3_every=(name == 'grid3_200v200'))
    return k0, k1, s0, s1, bool(np.all(s0 == s0[0]) and np.all(s1 == s1[0]))


CASES = ('tiny', 'cap128', 'cap256', 'grid3_200v200', 'full_256v256', 'cap512')
_REF = {}


def _reference(name, dtype, all_tests):
    """computed once per (case, dtype, tests) and shared; never modified"""
    import nanomod_oracle as orc
    key = (name, dtype, all_tests)
    if key not in _REF:
        k0, k1, s0, s1, _ = _case(name)
        off0, off1 = _csr(s0), _csr(s1)
        # what the library computes on: float32 samples, or milli-units / 1000
        v0 = (k0 / 1000.0).astype(np.float32).astype(np.float64) if dtype == 'f32' else k0 / 1000.0
        v1 = (k1 / 1000.0).astype(np.float32).astype(np.float64) if dtype == 'f32' else k1 / 1000.0
        npos = len(s0)
        rid = (np.arange(npos) // 11).astype(np.int32)
        ks = [orc.ks_2samp(v0[off0[i]:off0[i + 1]], v1[off1[i]:off1[i + 1]]) for i in range(npos)]
        d = np.array([k[0] for k in ks]); p = np.maximum(np.array([k[1] for k in ks]), orc.DBL_MIN)
        if all_tests:
            comb = orc.detect_batch(v0, off0, v1, off1, rid, 2, 2.0, orc.METHOD_STOUFFER)['comb_p']
        else:
            comb = orc.combine_track(d, p, rid, 2, 2.0, orc.METHOD_STOUFFER)[1]
        for arr in (d, p, comb):
            arr.setflags(write=False)
        _REF[key] = (d, p, comb, rid)
    return _REF[key]


def _run(nm, k0, k1, s0, s1, rid, dtype, tests, stride):
    sig0 = (k0 / 1000.0).astype(np.float32) if dtype == 'f32' else k0
    sig1 = (k1 / 1000.0).astype(np.float32) if dtype == 'f32' else k1
    if stride:
        return nm.detect_host(sig0, None, sig1, None, rid, nb=2, weights_dif=2.0, method='stouffer', tests=tests,
                              stride0=int(s0[0]), stride1=int(s1[0]))
    return nm.detect_host(sig0, _csr(s0), sig1, _csr(s1), rid, nb=2, weights_dif=2.0, method='stouffer', tests=tests)


@pytest.mark.parametrize('all_tests', [False, True], ids=['ks', 'all'])
@pytest.mark.parametrize('dtype', ['f32', 'i16'])
@pytest.mark.parametrize('name', CASES)
def test_ks_d_equals_ks_2samp(nm, name, dtype, all_tests):
    L = nm._lib
    k0, k1, s0, s1, uniform = _case(name)
    assert len(s0) <= 4096
    d, p, comb, rid = _reference(name, dtype, all_tests)
    for stride in ([False, True] if uniform else [False]):
        got = _run(nm, k0, k1, s0, s1, rid, dtype, L.TEST_ALL if all_tests else L.TEST_KS, stride)
        bad = np.nonzero(got['ks_d'] != d)[0]
        assert bad.size == 0, (name, dtype, all_tests, stride, bad[:5], got['ks_d'][bad[:5]], d[bad[:5]])
        H.assert_close_p(got['ks_p'], p, 1e-9, 'ks_p')
        H.assert_close_p(got['comb_p'], comb, 1e-9, 'comb_p')


# ---- positions built to exercise the float-form pass of the 256-capacity instance: 200 v 200, (R, LG) = (16, 16), four
# positions per wave.  A position is a pooled order: 'S' / 'Q' tokens with strictly increasing values.
def _from_pattern(pat):
    S = [i for i, t in enumerate(pat) if t == 'S']
    Q = [i for i, t in enumerate(pat) if t == 'Q']
    assert len(S) == 200 and len(Q) == 200, (len(S), len(Q))
    return np.array(S, np.int16), np.array(Q, np.int16)


def _constructed():
    pos = {}
    # the maximum at k = 40 (lane 2) and again at k = 140 (lane 8): two trips
    pos['two_lanes'] = _from_pattern('S' * 40 + 'Q' * 40 + 'SQ' * 60 + 'S' * 40 + 'Q' * 40 + 'SQ' * 60)
    # ... at k = 40 and k = 41: two bins of lane 2
    pos['twice_in_lane'] = _from_pattern('S' * 40 + 'Q' + 'S' + 'Q' * 39 + 'SQ' * 159 + 'Q')
    # (cumL(k-1), k) = -best and (cumU(k), k) = +best in bin 50
    pos['a_and_b_in_one_bin'] = _from_pattern('S' * 50 + 'Q' * 100 + 'SSSQQ' * 50)
    # the maximum below every key of S: the candidate (cumU(0), 0)
    pos['k0'] = _from_pattern('Q' * 80 + 'SSSSSQQQ' * 40)
    # identical groups: D = 0, nothing to evaluate
    same = np.arange(200, dtype=np.int16) * 3
    pos['identical'] = (same, same.copy())
    # a run of S with samples of Q on it next to the others (one tie sends the whole wave down the general form)
    rng = np.random.default_rng(5)
    pos['grid3'] = ((rng.integers(0, 3, 200) * 10).astype(np.int16), (rng.integers(0, 3, 200) * 10 + 10).astype(np.int16))
    return pos


def test_constructed_positions_do_what_they_claim():
    """by the model of the kernel (no device needed, but it belongs to the GPU test below)"""
    pos = _constructed()
    ev = {n: M.evaluate(s, q, 16, 16) for n, (s, q) in pos.items()}
    for n, (s, q) in pos.items():
        best, att, d = M.brute_force(s, q)
        assert ev[n]['best'] == best and {(c, k) for c, k, _, _ in ev[n]['cands']} == att and ev[n]['d'] == d, n
    assert len(ev['two_lanes']['hits']) == 2 and {l for _, _, l, _ in ev['two_lanes']['cands']} == {2, 8}
    c = ev['twice_in_lane']['cands']
    assert ev['twice_in_lane']['hits'] == [2] and sorted(k for _, k, _, _ in c) == [40, 41]
    c = ev['a_and_b_in_one_bin']['cands']
    assert sorted((k, kind) for _, k, _, kind in c) == [(50, 'a'), (50, 'b')] and ev['a_and_b_in_one_bin']['hits'] == [3]
    assert ev['k0']['cands'] == [(80, 0, 0, '0')]
    assert ev['identical']['best'] == 0 and ev['identical']['cands'] == [] and ev['identical']['d'] == 0.0
    assert M.has_tied_run(*pos['grid3'])
    # positions of one wave that need a different number of trips
    assert len(ev['two_lanes']['hits']) != len(ev['a_and_b_in_one_bin']['hits'])


@pytest.mark.parametrize('with_ties', [False, True], ids=['short_form', 'general_form'])
@pytest.mark.parametrize('dtype', ['f32', 'i16'])
def test_constructed_positions_on_the_device(nm, dtype, with_ties):
    """the waves of four: [two_lanes, a_and_b, twice_in_lane, k0 or grid3] and [identical, k0, two_lanes, twice_in_lane or
    grid3]: positions with different trip counts share a wave; with_ties puts a tied position into each wave, so the whole
    wave takes the general evaluation, otherwise the short one"""
    import nanomod_oracle as orc
    L = nm._lib
    pos = _constructed()
    last = 'grid3' if with_ties else None
    order = ['two_lanes', 'a_and_b_in_one_bin', 'twice_in_lane', last or 'k0', 'identical', 'k0', 'two_lanes', last or 'twice_in_lane']
    k0 = np.concatenate([pos[n][0] for n in order]); k1 = np.concatenate([pos[n][1] for n in order])
    npos = len(order)
    s0 = np.full(npos, 200); s1 = np.full(npos, 200)
    rid = np.zeros(npos, np.int32)
    exp = np.array([orc.ks_2samp(pos[n][0] / 1000.0, pos[n][1] / 1000.0)[0] for n in order])
    for n, e in zip(order, exp):
        assert e == M.evaluate(pos[n][0], pos[n][1], 16, 16)['d'], n
    for tests in (L.TEST_KS, L.TEST_ALL):
        for stride in (True, False):
            for swap in (False, True):       # either group may be the sorted one (equal sizes: the first is)
                a, b = (k1, k0) if swap else (k0, k1)
                got = _run(nm, a, b, s0, s1, rid, dtype, tests, stride)
                assert np.array_equal(got['ks_d'], exp), (dtype, tests, stride, swap, got['ks_d'], exp)
