"""The definition of nmod_site_diff (include/nanomod_hip.h, K15) restated in numpy — stoich_ref's evaluation per row, the reductions by
math.fsum — the same problem in 50-digit mpmath, the gates derived from stoich_ref's constants, and the seeded pairs of rows that the
CPU pin (tests/test_site_diff.py) and the GPU parity tests (tests/test_site_diff_gpu.py) share.  Written from the header's text; the
reference project has no such step.

The outer iteration, as the header states it: K14's bracketed iteration for an interval end with H(d) = 2 (g^ - h(d)) and the
envelope slope S_1(x* + d) where the inner maximiser x* is interior, a bisection step where it is an end of I(d); every outer
evaluation runs its own inner iteration from the midpoint of I(d)."""
import functools
import math

import numpy as np

import stoich_ref as sr
from stoich_ref import EPS, C_SUM, C_T, C_LOG, C_ERFC, DBL_MIN

TOO_FEW, FLAT, NOT_CONVERGED, POOL_AT_END, TOO_LARGE = 1, 2, 4, 8, 32
FIELDS = ('pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat', 'p_diff')
SMALL, WAVE = 128, 512             # the class steps of the kernels (NMOD_DIFF_SMALL, NMOD_DIFF_WAVE): 16 lanes, one wave, a workgroup beyond
STAGE = sr.STAGE                   # words of both rows together that the workgroup form stages in LDS


def _shift(x, d):
    return min(max(x + d, 0.0), 1.0)


def _pair(w0, w1, p0, p1):
    return sr.evaluate(w0, p0), sr.evaluate(w1, p1)


def _solve(ev, mode, a, b, ghat, drop, max_iter, tol):
    """stoich_ref.solve over a callable: ev(x) -> (S, D, g)"""
    x = a + 0.5 * (b - a)
    for k in range(1, max_iter + 1):
        S, D, g = ev(x)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            if mode == 0:
                right = S > 0.0
                xn = x + np.float64(S) / np.float64(D)
            else:
                h = 2.0 * (ghat - g)
                right = h > drop if mode == 1 else h <= drop
                xn = x + np.float64(h - drop) / np.float64(2.0 * S)
        a, b = (x, b) if right else (a, x)
        if xn != x and not (xn > a and xn < b):
            xn = a + 0.5 * (b - a)
        step = abs(xn - x)
        x = float(xn)
        if tol > 0.0 and (b - a <= tol or step <= tol):
            return x, k, False
    return x, max_iter, True


def _joint(w0, w1, d):
    def ev(x):
        e0, e1 = _pair(w0, w1, x, _shift(x, d))
        return e0['S'] + e1['S'], e0['D'] + e1['D'], e0['g'] + e1['g']
    return ev


def inner(w0, w1, d, max_iter, tol):
    """the inner maximiser at d: (x*, at an end of I(d), not converged)"""
    lo, hi = max(0.0, -d), min(1.0, 1.0 - d)
    ev = _joint(w0, w1, d)
    if ev(lo)[0] <= 0.0:
        return lo, True, False
    if ev(hi)[0] >= 0.0:
        return hi, True, False
    x, _, nc = _solve(ev, 0, lo, hi, 0.0, 0.0, max_iter, tol)
    return x, False, nc


def _nan_site(n0, n1, status):
    r = {f: np.nan for f in FIELDS}
    r.update(n_valid0=n0, n_valid1=n1, iters=0, status=status, gates=None)
    return r


def _sum_err(n, e):                # the error of S at a point (stoich_ref.row: the sum and the operations per term, and t carried through u)
    return EPS * (C_SUM * n * e['abs_u'] + C_T * e['u2t'])


def _g_err(n, e):                  # the error of g at a point
    return EPS * ((C_SUM * n + C_LOG) * e['abs_g'] + C_T * e['abs_u'])


def site(s0, s1, min_valid=3, max_iter=60, tol=1e-12, ci_drop=sr.CI_DROP_95, interval=True):
    """one site by the header's definition: its outputs and `gates` (None without an estimate)"""
    s0, s1 = np.asarray(s0, dtype=np.float64), np.asarray(s1, dtype=np.float64)
    n0, n1 = int(sr._valid(s0).sum()), int(sr._valid(s1).sum())
    if n0 < min_valid or n1 < min_valid:
        return _nan_site(n0, n1, TOO_FEW)
    w0, w1 = sr.signed_t(s0), sr.signed_t(s1)
    if not math.fsum(np.abs(w0)) > 0.0 or not math.fsum(np.abs(w1)) > 0.0:
        return _nan_site(n0, n1, FLAT)
    z0, z1 = _pair(w0, w1, 0.0, 0.0)
    o0, o1 = _pair(w0, w1, 1.0, 1.0)
    nc = False

    def alone(w, z, o):
        if z['S'] <= 0.0:
            return 0.0, 0, False
        if o['S'] >= 0.0:
            return 1.0, 0, False
        return sr.solve(w, 0, 0.0, 1.0, 0.0, 0.0, max_iter, tol)
    pi0, _, c0 = alone(w0, z0, o0)
    pi1, _, c1 = alone(w1, z1, o1)
    if z0['S'] + z1['S'] <= 0.0:
        pip, iters, cp = 0.0, 0, False
    elif o0['S'] + o1['S'] >= 0.0:
        pip, iters, cp = 1.0, 0, False
    else:
        pip, iters, cp = _solve(_joint(w0, w1, 0.0), 0, 0.0, 1.0, 0.0, 0.0, max_iter, tol)
    nc = c0 or c1 or cp
    h0, h1 = _pair(w0, w1, pi0, pi1)
    q0, q1 = _pair(w0, w1, pip, pip)
    ghat, gpool = h0['g'] + h1['g'], q0['g'] + q1['g']
    stat = max(2.0 * (ghat - gpool), 0.0)
    p_diff = max(math.erfc(math.sqrt(0.5 * stat)), DBL_MIN)
    delta = pi1 - pi0

    # ---- gates (stoich_ref.row's reasoning, per row and summed)
    def root_gate(e, n, interior):                     # a root of S (or of S0 + S1: e, n lists): tolerance, spacing, error of S over D
        if not interior:
            return 0.0
        return tol + 2.0 * EPS + sum(_sum_err(m + 1, v) for v, m in zip(e, n)) / sum(v['D'] for v in e)
    g_pi0 = root_gate([h0], [n0], 0.0 < pi0 < 1.0)
    g_pi1 = root_gate([h1], [n1], 0.0 < pi1 < 1.0)
    g_pip = root_gate([q0, q1], [n0, n1], 0.0 < pip < 1.0)
    # g at a maximiser: its own error, and D x^2 / 2 for a deviation x of the point (the slope is 0 there); one rounding of the sum
    gh_err = _g_err(n0, h0) + _g_err(n1, h1) + 0.5 * (h0['D'] * g_pi0 ** 2 + h1['D'] * g_pi1 ** 2) + EPS * abs(ghat)
    gp_err = _g_err(n0, q0) + _g_err(n1, q1) + 0.5 * (q0['D'] + q1['D']) * g_pip ** 2 + EPS * abs(gpool)
    # at an end the estimate is exact but the slope is not 0: nothing moves, the point is the same in both
    g_stat = 2.0 * (gh_err + gp_err) + 4.0 * EPS * stat
    pd = lambda st: max(math.erfc(math.sqrt(0.5 * max(st, 0.0))), DBL_MIN)
    p_rng = (pd(stat + g_stat) * (1.0 - C_ERFC * EPS), pd(stat - g_stat) * (1.0 + C_ERFC * EPS))
    gates = dict(pi0=g_pi0, pi1=g_pi1, pi_pool=g_pip, delta=g_pi0 + g_pi1 + 2.0 * EPS, stat=g_stat, p_diff=p_rng, delta_lo=0.0, delta_hi=0.0)
    res = dict(pi0=pi0, pi1=pi1, pi_pool=pip, delta=delta, delta_lo=np.nan, delta_hi=np.nan, stat=stat, p_diff=p_diff, n_valid0=n0,
               n_valid1=n1, iters=iters, gates=gates)
    if interval:
        state = dict(nc=False)

        def profile(d):
            x, at_end, c = inner(w0, w1, d, max_iter, tol)
            state['nc'] = state['nc'] or c
            e0, e1 = _pair(w0, w1, x, _shift(x, d))
            return (np.nan if at_end else e1['S']), 0.0, e0['g'] + e1['g']

        def end_gate(d):
            # the root of H(d) = 2 (g^ - h(d)) - drop, |H'| = 2 |h'|: tolerance, spacing of doubles below 2, the errors of h and g^ over
            # |h'|.  h' = S1 at the pair where pi1 moves with d (x* interior, or pi0 held at an end), else -S0
            x, at_end, _ = inner(w0, w1, d, max_iter, tol)
            p1 = _shift(x, d)
            e0, e1 = _pair(w0, w1, x, p1)
            g_in = 0.0 if at_end else tol + 2.0 * EPS + (_sum_err(n0 + 1, e0) + _sum_err(n1 + 1, e1)) / (e0['D'] + e1['D'])
            h_err = _g_err(n0, e0) + _g_err(n1, e1) + 0.5 * (e0['D'] + e1['D']) * g_in ** 2 + EPS * abs(e0['g'] + e1['g'])
            slope = abs(e0['S']) if at_end and p1 in (0.0, 1.0) else abs(e1['S'])
            return tol + 4.0 * EPS + (h_err + gh_err) / slope
        lo_end = 2.0 * (ghat - (o0['g'] + z1['g'])) <= ci_drop
        hi_end = 2.0 * (ghat - (z0['g'] + o1['g'])) <= ci_drop
        lo, hi, cl, ch = -1.0, 1.0, False, False
        if not lo_end:
            lo, _, cl = _solve(profile, 1, -1.0, delta, ghat, ci_drop, max_iter, tol)
            gates['delta_lo'] = end_gate(lo)
        if not hi_end:
            hi, _, ch = _solve(profile, 2, delta, 1.0, ghat, ci_drop, max_iter, tol)
            gates['delta_hi'] = end_gate(hi)
        nc = nc or cl or ch or state['nc']
        res.update(delta_lo=lo, delta_hi=hi)
    res['status'] = (NOT_CONVERGED if nc else 0) | (POOL_AT_END if pip in (0.0, 1.0) else 0)
    return res


DEFAULTS = dict(sr.DEFAULTS)


def site_diff(score0, off0, score1, off1, **opts):
    """every site of two CSR batches: a list of site() results"""
    o = dict(DEFAULTS, **opts)
    return [site(score0[off0[i]:off0[i + 1]], score1[off1[i]:off1[i + 1]], **o) for i in range(len(off0) - 1)]


# ---- the same problem in 50 digits
def exact_site(s0, s1, ci_drop=sr.CI_DROP_95):
    import mpmath as mp
    with mp.workdps(50):
        rows = []
        for s in (s0, s1):
            v = [mp.mpf(float(x)) for x in s if abs(x) <= sr.DBL_MAX]
            rows.append(([mp.exp(-abs(x)) for x in v], [x >= 0 for x in v]))

        def den(x, ei, p):
            return (x + (1 - x) * ei) if p else ((1 - x) + x * ei)

        def S(r, x):
            return mp.fsum((1 - ei) / den(x, ei, p) * (1 if p else -1) for ei, p in zip(*rows[r]))

        def g(r, x):
            return mp.fsum(mp.log(den(x, ei, p)) for ei, p in zip(*rows[r]))

        def bisect(f, a, b, n=170):   # f(a) > 0 >= f(b)
            for _ in range(n):
                m = (a + b) / 2
                a, b = (m, b) if f(m) > 0 else (a, m)
            return (a + b) / 2
        zero, one = mp.mpf(0), mp.mpf(1)

        def mle(f):
            return zero if f(zero) <= 0 else (one if f(one) >= 0 else bisect(f, zero, one))
        pi0, pi1 = mle(lambda x: S(0, x)), mle(lambda x: S(1, x))
        pip = mle(lambda x: S(0, x) + S(1, x))
        ghat = g(0, pi0) + g(1, pi1)
        stat = max(2 * (ghat - g(0, pip) - g(1, pip)), zero)

        def h(d):
            lo, hi = max(zero, -d), min(one, 1 - d)
            f = lambda x: S(0, x) + S(1, x + d)
            x = lo if (lo == hi or f(lo) <= 0) else (hi if f(hi) >= 0 else bisect(f, lo, hi, 90))
            return g(0, x) + g(1, x + d)
        H = lambda d: 2 * (ghat - h(d)) - ci_drop
        delta = pi1 - pi0
        lo = -one if H(-one) <= 0 else bisect(H, -one, delta, 60)
        hi = one if H(one) <= 0 else bisect(lambda d: -H(d), delta, one, 60)
        return dict(pi0=pi0, pi1=pi1, pi_pool=pip, delta=delta, delta_lo=lo, delta_hi=hi, stat=stat,
                    p_diff=max(mp.erfc(mp.sqrt(stat / 2)), mp.mpf(DBL_MIN)))


# ---- seeded pairs
LENGTHS = (0, 1, 2, 7, 8, 9, SMALL - 1, SMALL, SMALL + 1, WAVE - 1, WAVE, WAVE + 1)
LOPSIDED = ((3, SMALL + 1), (SMALL + 1, 3), (5, WAVE + 1), (WAVE + 1, 5), (STAGE - 700, 700), (STAGE - 700, 701))


@functools.lru_cache(maxsize=None)
def length_batch():
    """(score0, off0, score1, off1): every length of LENGTHS against itself, the lopsided pairs, a pair whose lengths sum to the LDS
    stage limit and one score past it"""
    rng = np.random.default_rng(1501)
    r0, r1 = [], []
    for i, (a, b) in enumerate([(n, n) for n in LENGTHS] + list(LOPSIDED)):
        sep = sr.SEPARATIONS[i % 4]
        r0.append(sr.simulate_row(rng, a, sep, (0.3, 0.5, 0.1)[i % 3]))
        r1.append(sr.simulate_row(rng, b, sep, (0.3, 0.7, 0.6)[i % 3]))
    return sr._csr(r0) + sr._csr(r1)


@functools.lru_cache(maxsize=None)
def content_batch():
    """(score0, off0, score1, off1): separations 0.3 .. 8 at equal and unequal shares 0 .. 1, and rows holding +-800, +-1e300, +-0.0, NaN,
    +-inf, one row all-invalid, one row flat"""
    rng = np.random.default_rng(1502)
    r0, r1 = [], []
    for sep in sr.SEPARATIONS:
        for p0, p1 in ((0.0, 0.0), (0.3, 0.3), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (0.02, 0.5), (0.5, 0.98), (0.7, 0.2)):
            r0.append(sr.simulate_row(rng, 40, sep, p0))
            r1.append(sr.simulate_row(rng, 25, sep, p1))
    nan, inf = np.nan, np.inf
    odd = [np.array([800.0, 800.0, 800.0, -800.0]), np.array([-800.0] * 5), np.array([800.0] * 5), np.array([1e300, -1e300, 1e300, 2.0, -1.0]),
           np.array([0.0, -0.0, 1.0, -2.0, 0.5]), np.array([nan, 2.0, -1.0, inf, 0.7, -inf, -0.2]), np.array([nan, inf, -inf, nan]),
           np.array([0.0, -0.0, 0.0, 0.0])]
    for i, o in enumerate(odd):
        plain = sr.simulate_row(rng, 30, 3.0, 0.5)
        r0 += [o, plain, o]
        r1 += [plain, o, odd[(i + 1) % len(odd)]]
    return sr._csr(r0) + sr._csr(r1)


@functools.lru_cache(maxsize=None)
def expected(which, **opts):
    """the restatement over length_batch / content_batch, computed once"""
    s0, o0, s1, o1 = length_batch() if which == 'length' else content_batch()
    return site_diff(s0, o0, s1, o1, **opts)
