"""CPU: the fixtures the device p-value tails (K2) and the window combine (K3) are pinned to (tests/golden/tails_k2.npz,
tails_k3.npz; definitions in tail_ref.py, written by oracle/gen_tail_golden.py).
  * a new mpmath run reproduces the committed files bit for bit;
  * the two CPU oracles agree with them: D, U, pads, clamps and the convention rows exactly, p within 1e-11 relative
    (measured: profiles/pvalue_tails.txt);
  * the inputs reach every branch of special_math.hpp and every band of the combined p in every configuration: conditions on
    the reference values alone, so the GPU test cannot go hollow."""
import numpy as np
import pytest

import helpers as H
import nanomod_oracle as orc
import tail_ref as T

P_REL = 1e-11


@pytest.fixture(scope='module')
def k2():
    return T.load_k2()


@pytest.fixture(scope='module')
def k3():
    return T.load_k3()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_k2_fixture_is_reproduced_bit_for_bit(k2):
    pytest.importorskip('mpmath')
    new = T.build_k2()
    assert sorted(new) == sorted(k2)
    for k in new:
        assert _same_bits(new[k], k2[k]), k


def test_k3_fixture_is_reproduced_bit_for_bit(k3):
    pytest.importorskip('mpmath')
    new = T.build_k3()
    assert sorted(new) == sorted(k3)
    for k in new:
        assert _same_bits(new[k], k3[k]), k


def test_reference_functions_against_mpmath_builtins(k2):
    """the hand-written series / continued fraction of tail_ref against mpmath's own betainc, jtheta and erfinv"""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = T.DPS
    rec = k2['recipes']
    for i in range(0, len(rec), 41):
        _, t2, df, _ = T.k2_welch_exact(rec[i])
        if t2 == 0:
            continue
        x = mp.mpf(df.numerator * (df + t2).denominator) / mp.mpf(df.denominator * (df + t2).numerator)
        with mp.workdps(420):                   # (betainc sums a hypergeometric series: room for its cancellation)
            ref = mp.betainc(mp.mpf(df.numerator) / (2 * df.denominator), mp.mpf(1) / 2, 0, x, regularized=True)
        got = T.student_t_two_sided_mp(t2, df)
        assert abs(got - ref) <= mp.mpf(10) ** -40 * ref, (i, got, ref)
    for x in (0.05, 0.3, 0.81, 0.83, 1.5, 7.0, 26.0):
        # Q(x) = 1 - theta_4(0, exp(-2 x^2)) ... as the dual: sqrt(2 pi)/x sum exp(-(2k-1)^2 pi^2 / (8 x^2))
        xx = mp.mpf(x)
        dual = 1 - mp.sqrt(2 * mp.pi) / xx * mp.nsum(lambda k: mp.exp(-(2 * k - 1) ** 2 * mp.pi ** 2 / (8 * xx * xx)), [1, mp.inf])
        got = T.kolmogorov_mp(x)
        assert abs(got - dual) <= mp.mpf(10) ** -45, (x, got, dual)
    for p in (0.5, 0.25, 1e-3, 1e-10):
        assert abs(T.norm_isf_mp(p) - mp.sqrt(2) * mp.erfinv(1 - 2 * mp.mpf(p))) <= mp.mpf(10) ** -40
    for p in (T.DBL_MIN, 1e-200, 1.0 - 2.0 ** -53):
        z = T.norm_isf_mp(p)
        assert abs(T.norm_sf_mp(z) - mp.mpf(p)) <= mp.mpf(10) ** -50 * mp.mpf(p)


# ---------------------------------------------------------------------------------------------------------------- K2
def _report(name, err, band):
    for b, n, w in T.worst_by_band(err, band):
        print('  cpu %-22s %-18s n=%-5d worst rel %.2e' % (name, b, n, w))


def _check_k2(out, fx, what, sig0, off0, sig1, off1):
    assert np.array_equal(out['ks_d'], fx['ks_d']), what + ': D'
    assert np.array_equal(out['mwu_u'], fx['mwu_u']), what + ': U'
    assert not out['status'].any()
    worst = 0.0
    for k in ('ks_p', 'mwu_p', 't_p'):
        clamp = fx[k] == T.DBL_MIN
        assert np.array_equal(out[k] == T.DBL_MIN, clamp), '%s %s: clamped positions differ' % (what, k)
        err = T.rel_err(out[k], fx[k])
        _report('%s %s' % (what, k), err, T.p_band(fx[k]))
        worst = max(worst, err.max())
        assert err.max() <= P_REL, (what, k, err.max(), int(err.argmax()))
    H.assert_close_stat(out['t_t'], fx['t_t'], 1e-11, H.t_abs_gate(sig0, off0, sig1, off1), what + ' t_t')
    return worst


def test_k2_python_oracle_agrees(k2):
    sig0, off0, sig1, off1 = T.k2_rows(k2['recipes'], np.float64)
    out = orc.per_position_tests(sig0, off0, sig1, off1)
    print()
    _check_k2(out, k2, 'orc', sig0, off0, sig1, off1)


def test_k2_c_oracle_agrees(k2):
    oracle_c = pytest.importorskip('oracle_c', reason='make -C oracle')
    sig0, off0, sig1, off1 = T.k2_rows(k2['recipes'], np.float32)
    out = oracle_c.detect_batch(sig0, off0, sig1, off1, np.zeros(len(off0) - 1, np.int32), 0, 2.0, 'ks', tests=7, threads=1)
    print()
    _check_k2(out, k2, 'oracle_c', sig0, off0, sig1, off1)


def test_k2_exact_statistics(k2):
    """D's two forms and U against the recipes' integers (no oracle involved)"""
    rec = k2['recipes']
    prod = (rec[:, 0] * rec[:, 1]).astype(np.float64)
    assert np.array_equal(k2['ks_d_rational'], k2['ks_num'] / prod)
    assert (np.abs(k2['ks_d'] - k2['ks_d_rational']) <= 2.3e-16).all()          # the float form: one rounding of a difference <= 1
    assert (k2['ks_num'] >= 0).all() and (k2['ks_num'] <= rec[:, 0] * rec[:, 1]).all()
    assert np.array_equal(k2['mwu_u'] * 2, np.rint(k2['mwu_u'] * 2)) and (k2['mwu_u'] <= prod / 2).all()
    # cross-group ties are present (h = 0, s = 1): U on a half-integer somewhere, D taken at tied points
    assert (k2['mwu_u'] != np.rint(k2['mwu_u'])).sum() >= 20


def test_k2_inputs_reach_every_branch(k2):
    br = T.k2_branches(k2)
    rec = k2['recipes']
    assert set(zip(rec[:, 0].tolist(), rec[:, 1].tolist())) >= set(T.SIZE_PAIRS)
    ladder = rec[:, 4] < 2
    for fam in (0, 1):                                          # per h: every pair with its 64 + ~40 shifts
        assert (rec[:, 4] == fam).sum() == sum(len(T.k2_shifts(n0)) for n0, _ in T.SIZE_PAIRS)
    assert ladder.sum() >= 1200
    # kolmogorov_sf: the theta dual below x = 0.82, the alternating series above
    assert br['ks_dual'].sum() >= 50 and (~br['ks_dual']).sum() >= 50, br['ks_dual'].sum()
    # student_t_two_sided: the hypergeometric fast path t^2 < 9 && y < 0.3, and both regimes of betacf among the rest
    fast, direct = br['fast'], br['direct']
    assert fast.sum() >= 50 and (~fast).sum() >= 50, fast.sum()
    assert (~fast & direct).sum() >= 20 and (~fast & ~direct).sum() >= 20, ((~fast & direct).sum(), (~fast & ~direct).sum())
    # betacf's rescaling: a fraction long enough for its terms to leave the double range (tail_ref.LARGE_DF_PAIRS)
    assert ((k2['t_df'] >= 6e4) & (k2['t_t2'] >= 9.0) & (k2['t_t2'] < 100.0)).sum() >= 6
    # lbeta_half: the z < 16 shift
    assert br['shift'].sum() >= 20 and (~br['shift']).sum() >= 20
    for k in ('ks_p', 'mwu_p', 't_p'):
        assert (k2[k] == T.DBL_MIN).sum() >= 20, (k, (k2[k] == T.DBL_MIN).sum())
        assert ((k2[k] > T.DBL_MIN) & (k2[k] < 1e-100)).sum() >= 20, k
    # every 64-lane wave of finalize_kernel (ladder order) that holds a fast lane also holds a lane of the continued fraction
    # somewhere in the ladder: the ballots are exercised with lanes on both sides
    n = len(rec) // 64 * 64
    f = fast[:n].reshape(-1, 64)
    assert ((f.any(1)) & (~f.all(1))).sum() >= 10


# ---------------------------------------------------------------------------------------------------------------- K3
def test_k3_python_oracle_agrees(k3):
    print()
    for key, p, nb, wd, m in T.k3_tracks(k3):
        meth = orc.METHOD_STOUFFER if m == 'S' else orc.METHOD_FISHER
        with np.errstate(all='ignore'):
            st, pv = orc.combine_track(np.zeros(T.K3_N), p, k3['run_id'], nb, float(wd), meth)
        T.check_k3_track(key, st, pv, k3, P_REL, st_rel=1e-12, st_abs=1e-13, who='orc')


def test_k3_convention_rows(k3):
    """what the planted NaN, 0.0 and 1.0 do, stated from the track's layout alone"""
    run_id = k3['run_id']
    pos = np.arange(T.K3_N)
    for nb, wd, m in T.K3_CONV:
        key = T.k3_key(nb, wd, m, 'conv')
        st, pv = k3[key + '_st'], k3[key + '_p']
        in_win = lambda i: (np.abs(pos - i) <= nb) & (run_id == run_id[i])        # the windows of i's run that contain i
        nan = np.zeros(T.K3_N, bool); zero = np.zeros(T.K3_N, bool); one = np.zeros(T.K3_N, bool)
        for i, v in T.K3_CONV_PLANTS:
            (nan if v != v else zero if v == 0.0 else one)[in_win(i)] = True
        edge = np.array([i - nb < 0 or i + nb >= T.K3_N or run_id[i - nb] != run_id[i] or run_id[i + nb] != run_id[i] for i in pos])
        minus = (one | edge) if m == 'S' else np.zeros(T.K3_N, bool)              # isf(1) = -inf, pads included; ln 1 = 0
        exp_nan = nan | (zero & minus)
        assert np.array_equal(np.isnan(pv), exp_nan) and np.array_equal(np.isnan(st), exp_nan), key
        hit = zero & ~exp_nan
        assert hit.any() and (st[hit] == T.DBL_MAX).all() and (pv[hit] == T.DBL_MIN).all(), key
        rest = minus & ~exp_nan & ~zero
        assert (st[rest] == -np.inf).all() and (pv[rest] == 1.0).all(), key
        # the NaN at 254 stays in its run: across the seam 255|256, position 256 is NaN only through the NaN at 300 of its own run
        assert np.isnan(pv[255]) and np.isnan(pv[256]) == (300 - 256 <= nb)


def test_k3_inputs_reach_every_band(k3):
    run_id = k3['run_id']
    assert run_id[255] != run_id[256] and run_id[511] == run_id[512] and run_id[699] != run_id[700]
    assert (run_id == run_id[-1]).sum() < 2 * 64 + 1 and T.K3_N == 4 * T.K3_TILE + 37
    print()
    for nb, wd, m in T.K3_CONFIGS:
        key = T.k3_key(nb, wd, m)
        p, band, ep = k3[key + '_in'], k3[key + '_band'], k3[key + '_p']
        assert (p < 1.0).all() and (p >= T.DBL_MIN).all()
        counts = np.bincount(band, minlength=6)
        print('  %-22s %s' % (key, ' '.join('%s: %d' % (n, c) for n, c in zip(T.BAND_NAMES, counts))))
        assert (counts[:4] >= 30).all(), (key, counts)              # (no configuration needs the relaxed p > 0.5 count: nb = 64 has >= 102)
        assert counts[T.BAND_CLAMP] >= 1, key
        edge = np.array([i - nb < 0 or i + nb >= T.K3_N or run_id[i - nb] != run_id[i] or run_id[i + nb] != run_id[i]
                         for i in range(T.K3_N)])
        assert edge.sum() >= 1
        if m == 'S':                                                # a window that touches a pad: Z = -inf, p = 1, and only there
            assert np.array_equal(band == T.BAND_PAD, edge) and (ep[edge] == 1.0).all()
        # the four numeric bands occur inside every run that has interior positions
        for lo, hi in T._runs(run_id):
            if hi - lo >= 2 * nb + 9:
                inner = band[lo + nb:hi - nb]
                assert all((inner == b).any() for b in range(4)), (key, lo, hi)
    raw = k3['raw_in']
    assert (raw == T.DBL_MIN).sum() >= 3 and (raw == 0.5).sum() >= 3 and (raw == 1.0 - 2.0 ** -53).sum() >= 3 and (raw < 1.0).all()
