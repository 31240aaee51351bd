"""The definitions the device p-value tails (K2, finalize_kernel) and the window combine (K3, combine_kernel) are held to:
mpmath at 60 digits over exact integers / rationals, no scipy anywhere in an expected value.

K2.  A position is two arithmetic sequences, so every statistic has a closed form:
    group 0 = {0, 1, ..., n0-1},   group 1 = {s i + j + h : i < n1},   s in {1, 1/16, 8}, j an integer shift, h in {1/2, 0}
(a recipe row is (n0, n1, 16 s, j, 2 h): integers).  All values are float32-exact (k2_rows asserts it).  h = 0 with s = 1 ties
the groups against each other.  Expected values:
    ks_num  exact integer max |c0 n1 - c1 n0| over the pooled points; ks_d its scipy-1.2.1 float form max |c0/n0 - c1/n1|
            (ks_d_rational: the correctly rounded quotient, what NMOD_FLAG_KS_RATIONAL_D reports);
    ks_p    the Kolmogorov series 2 sum (-1)^(k-1) exp(-2 k^2 x^2) at the 60-digit argument (en + 0.12 + 0.11/en) ks_num/(n0 n1);
    mwu_u   min(U1, U2) from exact rank sums on the x16 integer grid; mwu_p = erfc(|z| / sqrt 2) / 2, z^2 an exact rational;
    t_t     Welch's t from the closed-form means and sums of squares (rationals); t_p = I_{df/(df+t^2)}(df/2, 1/2);
each p clamped to DBL_MIN (m_min_float) and rounded to double once.

K3.  Tracks of K3_N = 4 * 256 + 37 positions (four tiles of combine_kernel and a ragged fifth) with run breaks on a tile
seam (255|256), none on the next seam, one inside a tile (700) and a last run shorter than one window of nb = 64.  The
p-values of a track are budgeted per configuration so that the COMBINED value sweeps 1 ... below DBL_MIN inside every run
(k3_track); expected values are
    Stouffer  z_j = isf(p_j) (Newton in mpmath on log Q), Z = sum w_j z_j / ||w||_2 with the doubles of stouffer_weights,
              p = Q(Z); a window that touches a pad (track end / another run: the reference substitutes p = 1) is Z = -inf, p = 1;
    Fisher    X = -2 sum ln p_j, p = exp(-X/2) sum_{m < 2nb+1} (X/2)^m / m!; a pad contributes 0;
clamped as m_min_float / m_max_float do.  The convention track (NaN, 0.0 and 1.0 planted) follows the same arithmetic with
IEEE rules for the infinities: (+inf) + (-inf) = NaN, NaN poisons its window.

Everything that needs mpmath imports it inside the function: the GPU tests use only the numpy parts (k2_rows, the fixtures)."""
import fractions
import os
import sys

import numpy as np

import helpers

F = fractions.Fraction
DBL_MIN = sys.float_info.min
DBL_MAX = sys.float_info.max
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
K2_FIXTURE = os.path.join(GOLDEN, 'tails_k2.npz')
K3_FIXTURE = os.path.join(GOLDEN, 'tails_k3.npz')
DPS = 60


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


# ---------------------------------------------------------------------------------------------------------------- K2
SIZE_PAIRS = ((2, 2), (3, 5), (8, 8), (17, 16), (64, 64), (200, 200), (256, 255), (700, 300), (2048, 2048), (2500, 1100))
SCALES16 = (16, 1, 128)                    # 16 s for s = 1, 1/16, 8
# The ladder above reaches the complement side of student_t_two_sided's continued fraction (x >= (a+1)/(a+b+2) on a lane the
# series has not finished: t^2 < 9 and y >= 0.3, which needs df < ~4.5) at a handful of positions only.  These extra pairs
# of tiny groups, same construction, every shift in sixteenths (j16) over a short range, fill that side.
SMALL_DF_PAIRS = ((2, 2), (2, 3), (3, 2), (3, 3), (2, 5), (4, 2))
# betacf's rescaling is first needed where the fraction runs long enough for its terms to leave the double range: they shrink by
# ~(1 - x) per step and the fraction takes ~sqrt(a) steps, which passes 1e-308 from df ~ 3e4 on (t^2 just above 9).  None of
# the pairs above gets there; this one does (df = 65 534), at eight shifts that put t between 3 and 9.2 (s = 1, h = 1/2).
LARGE_DF_PAIRS = ((32768, 32768),)
LARGE_DF_SHIFTS = tuple(222 + 64 * k for k in range(8))
K2_COLUMNS = ('n0', 'n1', 's16', 'j16', 'family')       # family: 0 = ladder h = 1/2, 1 = ladder h = 0, 2 = small-df, 3 = large-df extras


def k2_shifts(n0):
    """every shift of the first 64, then 40 evenly spaced up to 1.25 n0"""
    js = list(range(64))
    top = (5 * n0) // 4
    if top > 64:
        js += sorted(set(64 + ((top - 64) * (i + 1)) // 40 for i in range(40)))
    return js


def k2_recipes():
    rec = []
    for fam, h2 in ((0, 1), (1, 0)):
        for pi, (n0, n1) in enumerate(SIZE_PAIRS):
            for k, j in enumerate(k2_shifts(n0)):
                rec.append((n0, n1, SCALES16[(k + pi) % 3], 16 * j + 8 * h2, fam))
    for pi, (n0, n1) in enumerate(SMALL_DF_PAIRS):
        for k in range(48):                                # shifts 0, 1/16, ... 47/16
            rec.append((n0, n1, SCALES16[(k + pi) % 3], k, 2))
    for n0, n1 in LARGE_DF_PAIRS:
        for j in LARGE_DF_SHIFTS:
            rec.append((n0, n1, 16, 16 * j + 8, 3))
    return np.array(rec, dtype=np.int64)


def k2_keys16(r):
    """the two groups of recipe row r on the x16 integer grid"""
    n0, n1, s16, j16 = (int(v) for v in r[:4])
    return 16 * np.arange(n0, dtype=np.int64), s16 * np.arange(n1, dtype=np.int64) + j16


def k2_rows(recipes, dtype=np.float32):
    """(sig0, off0, sig1, off1) of the recipes as CSR rows of `dtype`; every value is float32-exact"""
    g0, g1 = [], []
    for r in recipes:
        a, b = k2_keys16(r)
        g0.append(a / 16.0); g1.append(b / 16.0)
    off0 = np.zeros(len(recipes) + 1, np.int64); off0[1:] = np.cumsum([len(a) for a in g0])
    off1 = np.zeros(len(recipes) + 1, np.int64); off1[1:] = np.cumsum([len(b) for b in g1])
    sig0 = np.concatenate(g0); sig1 = np.concatenate(g1)
    for s in (sig0, sig1):
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s), 'a ladder value is not float32-exact'
    return sig0.astype(dtype), off0, sig1.astype(dtype), off1


def kolmogorov_mp(x):
    mp = _mp()
    x = mp.mpf(x)
    if x <= 0:
        return mp.mpf(1)
    s = mp.mpf(0)
    eps = mp.mpf(10) ** -(DPS + 10)
    k = 1
    while True:
        t = mp.exp(-2 * k * k * x * x)
        s += t if k % 2 else -t
        if t < eps:
            break
        k += 1
    return min(mp.mpf(1), max(mp.mpf(0), 2 * s))


def norm_sf_mp(z):
    mp = _mp()
    return mp.erfc(mp.mpf(z) / mp.sqrt(2)) / 2


def _betacf_mp(a, b, x):
    """continued fraction of I_x(a, b) (DLMF 8.17.22) by the modified Lentz recurrence; x < (a+1)/(a+b+2)"""
    mp = _mp()
    tiny = mp.mpf(10) ** -300
    eps = mp.mpf(10) ** -(DPS - 2)
    qab, qap, qam = a + b, a + 1, a - 1
    c = mp.mpf(1)
    d = 1 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1 / d
    h = d
    for m in range(1, 200000):
        m2 = 2 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1 + aa * d
        d = tiny if abs(d) < tiny else d
        c = 1 + aa / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1 + aa * d
        d = tiny if abs(d) < tiny else d
        c = 1 + aa / c
        c = tiny if abs(c) < tiny else c
        d = 1 / d
        de = d * c
        h *= de
        if abs(de - 1) < eps:
            return h
    raise AssertionError('betacf_mp did not converge')


def student_t_two_sided_mp(t2, df):
    """I_{df/(df+t^2)}(df/2, 1/2) = 2 t.sf(|t|, df) from exact rationals t^2, df"""
    mp = _mp()
    if t2 == 0:
        return mp.mpf(1)
    tot = df + t2
    x = mp.mpf(df.numerator * tot.denominator) / mp.mpf(df.denominator * tot.numerator)        # df / (df + t^2)
    y = mp.mpf(t2.numerator * tot.denominator) / mp.mpf(t2.denominator * tot.numerator)        # 1 - x, without cancellation
    a = mp.mpf(df.numerator) / mp.mpf(2 * df.denominator)
    b = mp.mpf(1) / 2
    lfront = a * mp.log(x) + b * mp.log(y) - (mp.loggamma(a) + mp.loggamma(b) - mp.loggamma(a + b))
    if x < (a + 1) / (a + b + 2):
        return mp.exp(lfront) * _betacf_mp(a, b, x) / a
    # here y < 1.5 / (a + 2.5): p > 0.08, the complement loses no more than two of the 60 digits
    return 1 - mp.exp(lfront) * _betacf_mp(b, a, y) / b


def k2_welch_exact(r):
    """(sign of t, t^2, df, y = t^2/(df + t^2)) as exact rationals from the closed-form means and sums of squares"""
    n0, n1, s16, j16 = (int(v) for v in r[:4])
    s = F(s16, 16)
    m0 = F(n0 - 1, 2); ss0 = F(n0 * (n0 * n0 - 1), 12)
    m1 = s * F(n1 - 1, 2) + F(j16, 16); ss1 = s * s * F(n1 * (n1 * n1 - 1), 12)
    vn0 = ss0 / ((n0 - 1) * n0); vn1 = ss1 / ((n1 - 1) * n1)
    df = (vn0 + vn1) ** 2 / (vn0 ** 2 / (n0 - 1) + vn1 ** 2 / (n1 - 1))
    d = m0 - m1
    t2 = d * d / (vn0 + vn1)
    return (d > 0) - (d < 0), t2, df, t2 / (df + t2)


def k2_mwu_exact(r):
    """(min U, |bigU - meanrank|, variance) of scipy 1.2.1's mannwhitneyu as exact rationals"""
    a, b = k2_keys16(r)
    n0, n1 = len(a), len(b)
    vals, cnt = np.unique(np.concatenate([a, b]), return_counts=True)
    below = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    rank2 = 2 * below + cnt + 1                                      # twice the average rank of a tie group
    r0 = F(int(rank2[np.searchsorted(vals, a)].sum()), 2)
    u0 = n0 * n1 + F(n0 * (n0 + 1), 2) - r0
    u1 = n0 * n1 - u0
    n = n0 + n1
    c = cnt.astype(object)
    T = 1 - F(int(np.sum(c ** 3 - c)), n ** 3 - n)
    var = T * n0 * n1 * (n + 1) / 12
    return min(u0, u1), abs(max(u0, u1) - F(n0 * n1, 2) - F(1, 2)), var


def k2_ks_exact(r):
    """(ks_num, the float form of D)"""
    a, b = k2_keys16(r)
    n0, n1 = len(a), len(b)
    pooled = np.concatenate([a, b])
    c0 = np.searchsorted(a, pooled, side='right'); c1 = np.searchsorted(b, pooled, side='right')
    return int(np.max(np.abs(c0 * n1 - c1 * n0))), float(np.max(np.abs(c0 / float(n0) - c1 / float(n1))))


K2_EXPECTED = ('ks_num', 'ks_d', 'ks_d_rational', 'ks_p', 'mwu_u', 'mwu_p', 't_t', 't_p',
               'ks_x', 'mwu_z', 't_df', 't_t2', 't_y')       # the last five: where the position sits in the device's branches


def _clamp_p(p):
    return max(float(p), DBL_MIN)


def k2_expected(recipes):
    mp = _mp()
    out = {k: np.empty(len(recipes), np.int64 if k == 'ks_num' else np.float64) for k in K2_EXPECTED}
    for i, r in enumerate(recipes):
        n0, n1 = int(r[0]), int(r[1])
        num, dfl = k2_ks_exact(r)
        en = mp.sqrt(mp.mpf(n0 * n1) / (n0 + n1))
        x = (en + mp.mpf(0.12) + mp.mpf(0.11) / en) * mp.mpf(num) / (n0 * n1)       # (0.12, 0.11: the doubles of the 1.2.1 expression)
        out['ks_num'][i] = num; out['ks_d'][i] = dfl; out['ks_d_rational'][i] = num / float(n0 * n1)
        out['ks_x'][i] = float(x); out['ks_p'][i] = _clamp_p(kolmogorov_mp(x))
        umin, dev, var = k2_mwu_exact(r)
        z = mp.mpf(dev.numerator) / dev.denominator / mp.sqrt(mp.mpf(var.numerator) / var.denominator)
        out['mwu_u'][i] = float(umin); out['mwu_z'][i] = float(z); out['mwu_p'][i] = _clamp_p(norm_sf_mp(z))
        sign, t2, df, y = k2_welch_exact(r)
        out['t_t'][i] = float(sign * mp.sqrt(mp.mpf(t2.numerator) / t2.denominator))
        out['t_df'][i] = float(df); out['t_t2'][i] = float(t2); out['t_y'][i] = float(y)
        out['t_p'][i] = _clamp_p(student_t_two_sided_mp(t2, df))
    return out


def build_k2():
    rec = k2_recipes()
    out = {'recipes': rec}
    out.update(k2_expected(rec))
    return out


def k2_branches(fx):
    """where each position sits in the device's branches (special_math.hpp), from the reference values alone"""
    a = 0.5 * fx['t_df']
    fast = (fx['t_t2'] < 9.0) & (fx['t_y'] < 0.3)
    direct = (1.0 - fx['t_y']) < (a + 1.0) / (a + 2.5)
    return dict(ks_dual=fx['ks_x'] < 0.82, fast=fast, direct=direct, shift=a < 16.0)


# ---------------------------------------------------------------------------------------------------------------- K3
K3_TILE = 256
K3_N = 4 * K3_TILE + 37
K3_BREAKS = (256, 700, 1040)                # a run starts at each: tile seam 255|256, mid-tile 700, last run of 21 positions
K3_CONFIGS = ((1, 2, 'S'), (1, 2, 'F'), (2, 2, 'S'), (2, 2, 'F'), (5, 1, 'S'), (16, 3, 'S'), (16, 2, 'F'),
              (64, 2, 'S'), (64, 1, 'S'), (64, 2, 'F'))
K3_RAW = ((1, 2, 'S'), (1, 2, 'F'), (2, 2, 'S'), (2, 2, 'F'))
K3_CONV = ((1, 2, 'S'), (2, 2, 'F'), (16, 3, 'S'), (64, 2, 'S'), (64, 2, 'F'))
METHOD_NAME = {'S': 'stouffer', 'F': 'fisher'}
# band labels of a position, from the reference p
BAND_HIGH, BAND_MID, BAND_LOW, BAND_FAR, BAND_CLAMP, BAND_PAD = 0, 1, 2, 3, 4, 5
BAND_NAMES = ('p > 0.5', '1e-3 .. 0.5', '1e-100 .. 1e-3', 'DBL_MIN .. 1e-100', 'clamped', 'pad (-inf)')
SWEEP_U = (0.0, 0.22, 0.44, 0.66, 0.90, 1.0)        # a fifth of a run per band, the last tenth for the clamp


def k3_key(nb, wd, m, kind='sweep'):
    return '%s_nb%d_wd%d_%s' % (kind, nb, wd, m)


def k3_run_id(n=K3_N, breaks=K3_BREAKS):
    r = np.zeros(n, np.int32)
    for b in breaks:
        r[b:] += 1
    return r


def stouffer_weights(nb, wd):
    """the doubles of myDetect.py:396-400"""
    w = [100.0]
    for _ in range(nb):
        w.insert(0, w[0] / float(wd)); w.append(w[-1] / float(wd))
    return w


def _runs(run_id):
    edges = [0] + [i for i in range(1, len(run_id)) if run_id[i] != run_id[i - 1]] + [len(run_id)]
    return list(zip(edges[:-1], edges[1:]))


def k3_sweep_u(run_id, nb):
    """0 ... 1 along every run, starting at the run's first interior position (window inside the run) when it has some"""
    u = np.empty(len(run_id))
    for lo, hi in _runs(run_id):
        i = np.arange(lo, hi, dtype=np.float64)
        if hi - lo >= 2 * nb + 9:
            u[lo:hi] = np.clip((i - (lo + nb)) / float(hi - lo - 2 * nb - 1), 0.0, 1.0)
        else:
            u[lo:hi] = (i - lo) / float(max(hi - lo - 1, 1))
    return u


def chi2_sf_even_mp(x, W):
    """Q(W, x) = exp(-x) sum_{m < W} x^m / m!"""
    mp = _mp()
    x = mp.mpf(x)
    t = mp.mpf(1); s = mp.mpf(1)
    for m in range(1, W):
        t = t * x / m
        s += t
    return mp.exp(-x) * s


def _fisher_knot(W, log10p):
    """x with Q(W, x) = 10^log10p (bisection; Q is decreasing), to 1e-9"""
    mp = _mp()
    target = mp.mpf(10) ** log10p
    lo, hi = mp.mpf(0), mp.mpf(4000)
    for _ in range(60):
        mid = (lo + hi) / 2
        if chi2_sf_even_mp(mid, W) > target:
            lo = mid
        else:
            hi = mid
    return float(round((lo + hi) / 2 * 1000) / 1000)          # (a grid value: the knot does not depend on the last bits)


def _uniform(seed, n, k):
    """k columns of n uniforms of [0, 1) (numpy's PCG64 stream: the same doubles everywhere)"""
    return np.random.default_rng(seed).random((n, k))


def k3_track(nb, wd, m, seed):
    """the input p-values of a sweep configuration, and for Stouffer the z they were drawn from (Newton's starting point)"""
    mp = _mp()
    run_id = k3_run_id()
    u = k3_sweep_u(run_id, nb)
    W = 2 * nb + 1
    p = np.empty(K3_N)
    if m == 'F':
        # X/2 = sum g_j ~ G(u): G runs through the x at which Q(W, x) = 1 (nearly), 0.5, 1e-3, 1e-100, 1e-305 and 1e-335
        knots = [0.02 * W] + [_fisher_knot(W, e) for e in (np.log10(0.5), -3, -100, -305, -335)]
        G = np.interp(u, SWEEP_U, knots)
        g = np.minimum(G / W * (0.5 + _uniform(seed, K3_N, 1)[:, 0]), 708.0)
        for i in range(K3_N):
            p[i] = float(mp.exp(-mp.mpf(float(g[i]))))
        assert (p < 1.0).all() and (p >= DBL_MIN).all()
        return p, None
    # Z = sum w z / ||w||_2 ~ Zc(u) + N(0, 1): Zc runs through Q^-1 of the same band edges, -3 ... 40
    w = np.array(stouffer_weights(nb, wd))
    ratio = float(np.sqrt(np.sum(w * w))) / float(np.sum(w))
    Zc = np.interp(u, SWEEP_U, (-3.0, 0.0, 3.09, 21.27, 37.3, 40.0))
    un = _uniform(seed, K3_N, 12)
    noise = un[:, 0]
    for k in range(1, 12):
        noise = noise + un[:, k]
    z = np.clip(Zc * ratio + (noise - 6.0), -8.0, 37.5)          # (sum of 12 uniforms - 6: unit variance, plain additions)
    for i in range(K3_N):
        p[i] = float(norm_sf_mp(float(z[i])))
    assert (p < 1.0).all() and (p >= DBL_MIN).all()
    return p, z


def k3_raw_track(seed=7):
    """log-uniform over [DBL_MIN, 1) with exact DBL_MIN, 0.5 and 1 - 2^-53 planted"""
    mp = _mp()
    e = _uniform(seed, K3_N, 1)[:, 0] * 708.0
    p = np.array([float(mp.exp(-mp.mpf(float(v)))) for v in e])
    p = np.clip(p, DBL_MIN, 1.0 - 2.0 ** -53)
    for k, i in enumerate(range(40, K3_N, 97)):
        p[i] = (DBL_MIN, 0.5, 1.0 - 2.0 ** -53)[k % 3]
    return p


K3_CONV_PLANTS = ((254, np.nan), (300, np.nan), (500, 0.0), (701, 0.0), (850, 1.0), (1050, 1.0))


def k3_conv_track(seed=11):
    """moderate p-values (1e-6 ... 1) with a NaN, a 0.0 and a 1.0 planted inside runs and next to run breaks"""
    mp = _mp()
    e = _uniform(seed, K3_N, 1)[:, 0] * 14.0 + 0.01
    p = np.array([float(mp.exp(-mp.mpf(float(v)))) for v in e])
    for i, v in K3_CONV_PLANTS:
        p[i] = v
    return p


def norm_isf_mp(p, z0=None):
    """z with Q(z) = p for a double 0 < p < 1: Newton on log Q(z) - log p (concave: monotone from the right of the root)"""
    mp = _mp()
    p = mp.mpf(p)
    if p > 0.5:
        return -norm_isf_mp(1 - p)                # (1 - p is exact at 60 digits)
    lp = mp.log(p)
    z = mp.sqrt(-2 * lp) if z0 is None else mp.mpf(z0)
    tol = mp.mpf(10) ** -(DPS - 5)
    for _ in range(100):
        q = norm_sf_mp(z)
        step = (mp.log(q) - lp) * q * mp.sqrt(2 * mp.pi) * mp.exp(z * z / 2)
        z += step
        if abs(step) < tol * max(1, abs(z)):
            return z
    raise AssertionError('norm_isf_mp did not converge')


def k3_expected(p, run_id, nb, wd, m, z0=None):
    """(st, p, band) of a track: mpmath for the finite windows, IEEE rules for NaN and the infinities"""
    mp = _mp()
    n = len(p)
    W = 2 * nb + 1
    st = np.empty(n); pv = np.empty(n); band = np.empty(n, np.uint8)
    inf = float('inf')
    if m == 'S':
        w = stouffer_weights(nb, wd)
        wn = mp.sqrt(sum(mp.mpf(v) ** 2 for v in w))
        tr = []
        for i in range(n):
            v = float(p[i])
            if v != v:
                tr.append(v)
            elif v <= 0.0:
                tr.append(inf)
            elif v >= 1.0:
                tr.append(-inf)
            else:
                tr.append(norm_isf_mp(v, None if z0 is None or v > 0.5 else z0[i]))
    else:
        tr = [float(p[i]) if (p[i] != p[i]) else (-inf if p[i] <= 0.0 else mp.log(mp.mpf(float(p[i])))) for i in range(n)]
    for i in range(n):
        acc = mp.mpf(0); pos = neg = nan = pad = False
        for k in range(-nb, nb + 1):
            j = i + k
            if j < 0 or j >= n or run_id[j] != run_id[i]:
                pad = True
                neg = neg or m == 'S'               # the reference's substitute p = 1: isf = -inf, ln = 0
                continue
            v = tr[j]
            if isinstance(v, float):
                nan = nan or v != v; pos = pos or v == inf; neg = neg or v == -inf
            else:
                acc += mp.mpf(w[nb + k]) * v if m == 'S' else v
        if m == 'F':                                # X = -2 sum ln p: ln 0 = -inf is the only infinity
            pos, neg = neg, False
        if nan or (pos and neg):
            st[i] = pv[i] = float('nan')
        elif pos:
            st[i] = DBL_MAX; pv[i] = DBL_MIN
        elif neg:
            st[i] = -inf; pv[i] = 1.0
        elif m == 'S':
            Z = acc / wn
            st[i] = float(Z); pv[i] = _clamp_p(norm_sf_mp(Z))
        else:
            st[i] = float(-2 * acc); pv[i] = _clamp_p(chi2_sf_even_mp(-acc, W))
        q = pv[i]
        if st[i] == -inf:
            band[i] = BAND_PAD
        elif q != q or q <= DBL_MIN:
            band[i] = BAND_CLAMP
        else:
            band[i] = BAND_HIGH if q > 0.5 else BAND_MID if q > 1e-3 else BAND_LOW if q > 1e-100 else BAND_FAR
    return st, pv, band


def build_k3():
    out = {'run_id': k3_run_id()}
    for c, (nb, wd, m) in enumerate(K3_CONFIGS):
        key = k3_key(nb, wd, m)
        p, z = k3_track(nb, wd, m, seed=1000 + c)
        out[key + '_in'] = p
        out[key + '_st'], out[key + '_p'], out[key + '_band'] = k3_expected(p, out['run_id'], nb, wd, m, z)
    out['raw_in'] = k3_raw_track()
    for nb, wd, m in K3_RAW:
        key = k3_key(nb, wd, m, 'raw')
        out[key + '_st'], out[key + '_p'], out[key + '_band'] = k3_expected(out['raw_in'], out['run_id'], nb, wd, m)
    out['conv_in'] = k3_conv_track()
    for nb, wd, m in K3_CONV:
        key = k3_key(nb, wd, m, 'conv')
        out[key + '_st'], out[key + '_p'], out[key + '_band'] = k3_expected(out['conv_in'], out['run_id'], nb, wd, m)
    return out


def load_k2():
    return dict(np.load(K2_FIXTURE))


def load_k3():
    return dict(np.load(K3_FIXTURE))


# ---------------------------------------------------------------------------------------------------------------- errors
def rel_err(got, exp):
    """|got - exp| / |exp| where exp is finite and non-zero; positions where exp is NaN, infinite or 0 are the caller's to
    compare exactly (0 here)"""
    got = np.asarray(got, np.float64); exp = np.asarray(exp, np.float64)
    m = np.isfinite(exp) & (exp != 0.0)
    e = np.zeros(exp.shape)
    with np.errstate(invalid='ignore', over='ignore'):
        e[m] = np.abs(got[m] - exp[m]) / np.abs(exp[m])
    e[m & ~np.isfinite(got)] = np.inf
    return e


def p_band(p):
    """the band of a reference p (the four numeric bands, BAND_CLAMP at DBL_MIN)"""
    p = np.asarray(p)
    b = np.full(p.shape, BAND_FAR, np.uint8)
    b[p > 1e-100] = BAND_LOW; b[p > 1e-3] = BAND_MID; b[p > 0.5] = BAND_HIGH; b[p <= DBL_MIN] = BAND_CLAMP
    return b


def worst_by_band(err, band):
    """[(band name, count, worst error)] over the bands that occur"""
    return [(BAND_NAMES[b], int((band == b).sum()), float(err[band == b].max())) for b in range(len(BAND_NAMES)) if (band == b).any()]


def k3_tracks(k3):
    """(key, input, nb, wd, method letter) of every expected track"""
    for nb, wd, m in K3_CONFIGS:
        key = k3_key(nb, wd, m)
        yield key, k3[key + '_in'], nb, wd, m
    for nb, wd, m in K3_RAW:
        yield k3_key(nb, wd, m, 'raw'), k3['raw_in'], nb, wd, m
    for nb, wd, m in K3_CONV:
        yield k3_key(nb, wd, m, 'conv'), k3['conv_in'], nb, wd, m


def check_k3_track(key, st, pv, k3, p_rel, st_rel=1e-9, st_abs=1e-12, who='cpu'):
    """pads, clamps, NaN and infinities exact; the rest: p within p_rel, st within st_rel |st| + st_abs.  Returns (err, band)."""
    est, ep, band = k3[key + '_st'], k3[key + '_p'], k3[key + '_band']
    assert np.array_equal(np.isnan(pv), np.isnan(ep)) and np.array_equal(np.isnan(st), np.isnan(est)), key + ': NaN positions'
    special = np.isnan(ep) | np.isinf(est) | (ep == DBL_MIN) | (est == DBL_MAX)
    assert np.array_equal(pv[special], ep[special], equal_nan=True), key + ': pad / clamp / convention p'
    sx = np.isnan(est) | np.isinf(est) | (est == DBL_MAX)
    assert np.array_equal(st[sx], est[sx], equal_nan=True), key + ': pad / clamp / convention st'
    assert not (pv[~special] == DBL_MIN).any() and not np.isinf(st[~sx]).any(), key + ': a clamp or a pad where the reference has none'
    err = rel_err(pv, ep)
    err[special] = 0.0
    for b, n, w in worst_by_band(err, band):
        print('  %s %-22s %-18s n=%-5d worst rel %.2e' % (who, key, b, n, w))
    assert err.max() <= p_rel, (key, err.max(), int(err.argmax()), pv[err.argmax()], ep[err.argmax()])
    helpers.assert_close_stat(st, est, st_rel, st_abs, key + ' st')
    return err, band
