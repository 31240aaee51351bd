"""The definition of nmod_site_stoich (include/nanomod_hip.h, K14) restated in numpy — the same operations per score in the same order,
the reductions by math.fsum — the same problem solved in 50-digit mpmath, the gates derived from the two, and the seeded rows that the
CPU pin (tests/test_site_stoich.py) and the GPU parity tests (tests/test_site_stoich_gpu.py) share.  Written from the header's text;
the reference project has no such step.

Per row: the valid scores s_i (|s| <= DBL_MAX), t_i = -expm1(-|s_i|), the side of s_i; with q = 1 - pi on the plus side (s >= 0) and
q = pi on the minus side, an evaluation at pi is   S = sum +-u,  D = sum u^2,  g = sum log1p(-q t),   u = t / (1 - q t)."""
import functools
import math

import numpy as np

TOO_FEW, FLAT, NOT_CONVERGED, AT_ZERO, AT_ONE, TOO_LARGE = 1, 2, 4, 8, 16, 32
FIELDS = ('pi', 'pi_lo', 'pi_hi', 'stat', 'p_null')
DBL_MAX, DBL_MIN = 1.7976931348623157e308, 2.2250738585072014e-308
CI_DROP_95 = 3.841458820694124
SMALL, WAVE = 256, 1024            # the class steps of the kernels: 16 lanes, one wave, a workgroup beyond
STAGE = 6144                       # scores of a row the workgroup form stages in LDS (site_stoich.hip: kStStage)

# ---- the constants of the gates.  EPS is the unit roundoff of a double.
EPS = 2.0 ** -53
# C_SUM: a sum of n terms in any fixed order is within (n - 1) EPS sum|term| of the exact sum; the factor 8 over that covers the
# handful of correctly rounded operations per term (q t, 1 - q t, the division, the square) — the constant of the prototype behind
# the issue (c = 8), which stayed within 0.15 of the gate against mpmath.
C_SUM = 8.0
# C_T: t = -expm1(-|s|) comes from two libraries: glibc's expm1 is within 1 ulp, the device library's within the 3 ulp OpenCL allows.
# A relative error C_T EPS of t moves u = t / (1 - q t) by (du/dt) t C_T EPS = C_T EPS u^2 / t, and log1p(-q t) by C_T EPS q u.
C_T = 4.0
# C_LOG: log1p itself, 1 ulp (glibc) + 2 ulp (OpenCL): relative, per term.
C_LOG = 4.0
# C_EXP: exp in resp, 1 ulp + 3 ulp (OpenCL); C_ROUND: the four correctly rounded operations that follow it.
C_EXP, C_ROUND = 4.0, 4.0
# C_ERFC: 0.5 erfc(sqrt(l)): erfc within 16 ulp (OpenCL) + 2 ulp (glibc), sqrt and the halving exact or correctly rounded: relative.
C_ERFC = 20.0


def _valid(s):
    return np.abs(s) <= DBL_MAX


def signed_t(s):
    """t with the side of s as its sign; 0 for an invalid score"""
    s = np.asarray(s, dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        t = -np.expm1(-np.abs(s))
        return np.where(_valid(s), np.where(s >= 0.0, t, -t), 0.0)


def evaluate(w, pi):
    """(S, D, g) at pi over the signed t values w; also sum|u| and sum u^2 / t and sum|log1p| for the gates"""
    t, plus = np.abs(w), w >= 0.0
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        qt = np.where(plus, 1.0 - pi, pi) * t
        u = t / (1.0 - qt)
        lg = np.log1p(-qt)
        u2t = np.where(t > 0.0, u * u / np.where(t > 0.0, t, 1.0), 0.0)
    return dict(S=math.fsum(np.where(plus, u, -u)), D=math.fsum(u * u), g=math.fsum(lg), abs_u=math.fsum(np.abs(u)), u2t=math.fsum(u2t),
                abs_g=math.fsum(np.abs(lg)))


def solve(w, mode, a, b, ghat, drop, max_iter, tol):
    """the bracketed iteration of the header; mode 0: the root of S, 1: the lower end of the interval, 2: the upper end.
    Returns (x, evaluations, not_converged)"""
    x = a + 0.5 * (b - a)
    for k in range(1, max_iter + 1):
        e = evaluate(w, x)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            if mode == 0:
                right = e['S'] > 0.0
                xn = x + np.float64(e['S']) / np.float64(e['D'])
            else:
                h = 2.0 * (ghat - e['g'])
                right = h > drop if mode == 1 else h <= drop
                xn = x + np.float64(h - drop) / np.float64(2.0 * e['S'])
        a, b = (x, b) if right else (a, x)
        if xn != x and not (xn > a and xn < b):                     # (xn == x: the step is below the spacing of doubles at x; x stays)
            xn = a + 0.5 * (b - a)
        step = abs(xn - x)
        x = float(xn)
        if tol > 0.0 and (b - a <= tol or step <= tol):
            return x, k, False
    return x, max_iter, True


def _nan_row(n_valid, status, nrow):
    r = {f: np.nan for f in FIELDS}
    r.update(n_valid=n_valid, iters=0, status=status, resp=np.full(nrow, np.nan), gates=None)
    return r


def row(s, min_valid=3, max_iter=60, tol=1e-12, ci_drop=CI_DROP_95, estimate_only=False):
    """one row by the header's definition: its outputs, resp, and `gates` (None without an estimate); estimate_only: pi, stat, p_null,
    n_valid, iters alone (the simulations)"""
    s = np.asarray(s, dtype=np.float64)
    valid = _valid(s)
    n = int(valid.sum())
    if n < min_valid:
        return _nan_row(n, TOO_FEW, len(s))
    w = signed_t(s)
    if not math.fsum(np.abs(w)) > 0.0:
        return _nan_row(n, FLAT, len(s))
    try:
        P = math.fsum(s[valid & (s >= 0.0)])
    except OverflowError:
        P = math.inf
    e0, e1 = evaluate(w, 0.0), evaluate(w, 1.0)
    at0 = e0['S'] <= 0.0
    at1 = not at0 and e1['S'] >= 0.0
    iters, nc = 0, False
    if at0 or at1:
        pi = 0.0 if at0 else 1.0
    else:
        pi, iters, nc = solve(w, 0, 0.0, 1.0, 0.0, 0.0, max_iter, tol)
    eh = evaluate(w, pi)
    gh = eh['g']
    lhat = 0.0 if at0 else max(gh + P, 0.0)
    if estimate_only:
        return dict(pi=pi, stat=2.0 * lhat, p_null=1.0 if at0 else max(0.5 * math.erfc(math.sqrt(lhat)), DBL_MIN), n_valid=n, iters=iters)
    lo0, hi1 = 2.0 * (gh - e0['g']) <= ci_drop, 2.0 * (gh - e1['g']) <= ci_drop
    lo, hi = 0.0, 1.0
    if not lo0:
        lo, _, c = solve(w, 1, 0.0, pi, gh, ci_drop, max_iter, tol)
        nc = nc or c
    if not hi1:
        hi, _, c = solve(w, 2, pi, 1.0, gh, ci_drop, max_iter, tol)
        nc = nc or c
    p_null = 1.0 if at0 else max(0.5 * math.erfc(math.sqrt(lhat)), DBL_MIN)
    # resp
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        e = np.exp(-np.abs(s))
        den = np.where(s >= 0.0, pi + (1.0 - pi) * e, (1.0 - pi) + pi * e)
        r = np.where(s >= 0.0, pi / den, (pi * e) / den)
    r = np.where(valid, 0.0 if pi == 0.0 else (1.0 if pi == 1.0 else r), np.nan)

    # ---- the gates (module docstring of the constants above), n = the valid scores
    interior = not (at0 or at1)
    # pi^: a deviation of the root of S is its tolerance plus the error of S over |S'| = D.  S's error: the sum and the few operations
    # per term, C_SUM n EPS sum|u|, and the error of t carried through u, C_T EPS sum u^2 / t; and the spacing of doubles below 1, 2 EPS
    # (tol == 0 stops where a step falls below it).  At either end the estimate is exact.
    g_pi = tol + 2.0 * EPS + EPS * (C_SUM * n * eh['abs_u'] + C_T * eh['u2t']) / eh['D'] if interior else 0.0

    def g_err(ev):                 # the error of g at a point: the sum, log1p itself, and t carried through: d log1p(-q t) = q u dt / t
        return EPS * ((C_SUM * n + C_LOG) * ev['abs_g'] + C_T * ev['abs_u'])
    # g(pi^) as a function of pi^: g' = S is 0 at the root, so a deviation g_pi moves it by D g_pi^2 / 2 only
    gh_err = g_err(eh) + 0.5 * eh['D'] * g_pi * g_pi

    def g_end(x, fixed):           # an end of the interval: the root of h = 2 (g^ - g(x)) - drop, |h'| = 2 |S(x)|
        if fixed:
            return 0.0
        ev = evaluate(w, x)
        return tol + 2.0 * EPS + (g_err(ev) + gh_err) / abs(ev['S'])
    # l^ = g^ + P: P's sum over the plus side, C_SUM n EPS sum s
    l_err = 0.0 if at0 or math.isinf(lhat) else gh_err + C_SUM * n * EPS * P            # (an infinite l^ is matched as it is)
    # p_null is decreasing in l^: between its values at l^ +- l_err, widened by erfc's own relative error
    pn = lambda l: max(0.5 * math.erfc(math.sqrt(max(l, 0.0))), DBL_MIN)
    p_rng = (1.0, 1.0) if at0 else (pn(lhat + l_err) * (1.0 - C_ERFC * EPS), pn(lhat - l_err) * (1.0 + C_ERFC * EPS))
    # resp: dr/dpi = e / den^2 times the gate of pi^, exp's error through dr/de e = r (1 - r), and the roundings
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        g_r = np.where(valid, g_pi * e / (den * den) + (C_EXP + C_ROUND) * EPS * r, 0.0) if interior else np.zeros(len(s))
    # mean(resp) - pi^ = pi^ (1 - pi^) S(pi^) / n exactly (the score equation), and |S(pi^)| <= D g_pi
    g_mean = (pi * (1.0 - pi) * eh['D'] * g_pi / n + float(np.mean(g_r[valid]))) if interior else None
    gates = dict(pi=g_pi, pi_lo=g_end(lo, lo0), pi_hi=g_end(hi, hi1), stat=2.0 * l_err, p_null=p_rng, resp=g_r, mean_resp=g_mean)
    return dict(pi=pi, pi_lo=lo, pi_hi=hi, stat=2.0 * lhat, p_null=p_null, n_valid=n, iters=iters,
                status=(NOT_CONVERGED if nc else 0) | (AT_ZERO if at0 else 0) | (AT_ONE if at1 else 0), resp=r, gates=gates)


def site_stoich(score, off=None, stride=0, **opts):
    """every row of a CSR (off) or fixed-stride batch: a list of row() results"""
    score = np.asarray(score, dtype=np.float64)
    if off is None:
        off = np.arange(0, len(score) + 1, stride, dtype=np.int64)
    o = dict(DEFAULTS, **opts)
    return [row(score[off[i]:off[i + 1]], **o) for i in range(len(off) - 1)]


def ci_drop_of(level):
    from statistics import NormalDist
    return NormalDist().inv_cdf((1.0 + level) / 2.0) ** 2


# the defaults of the Python layers: ci_level = 0.95 as they convert it (within an ulp of CI_DROP_95)
DEFAULTS = dict(min_valid=3, max_iter=60, tol=1e-12, ci_drop=ci_drop_of(0.95))


# ---- the same problem in 50 digits
def exact_row(s, ci_drop=CI_DROP_95):
    """pi^, the interval, stat and p_null of the valid scores of `s` in 50-digit arithmetic (t is not rounded: no t reaches 1)"""
    import mpmath as mp
    with mp.workdps(50):
        s = [mp.mpf(float(v)) for v in s if abs(v) <= DBL_MAX]
        e = [mp.exp(-abs(v)) for v in s]                        # 1 - q t is written out in e = 1 - t: no cancellation at any |s|
        plus = [v >= 0 for v in s]

        def den(x, ei, p):
            return (x + (1 - x) * ei) if p else ((1 - x) + x * ei)

        def S(x):
            return mp.fsum((1 - ei) / den(x, ei, p) * (1 if p else -1) for ei, p in zip(e, plus))

        def g(x):
            return mp.fsum(mp.log(den(x, ei, p)) for ei, p in zip(e, plus))

        def bisect(f, a, b):      # f(a) > 0 >= f(b); 170 halvings: below 1e-50
            for _ in range(170):
                m = (a + b) / 2
                a, b = (m, b) if f(m) > 0 else (a, m)
            return (a + b) / 2
        zero, one = mp.mpf(0), mp.mpf(1)
        if S(zero) <= 0:
            pi = zero
        elif S(one) >= 0:
            pi = one
        else:
            pi = bisect(S, zero, one)
        gh = g(pi)
        h = lambda x: 2 * (gh - g(x)) - ci_drop
        lo = zero if h(zero) <= 0 else bisect(h, zero, pi)
        hi = one if h(one) <= 0 else bisect(lambda x: -h(x), pi, one)
        lhat = gh + mp.fsum(v for v in s if v >= 0) if pi > 0 else zero
        p = one if pi == 0 else mp.erfc(mp.sqrt(lhat)) / 2
        return dict(pi=pi, pi_lo=lo, pi_hi=hi, stat=2 * lhat, p_null=max(p, mp.mpf(DBL_MIN)))


# ---- seeded rows
def simulate_row(rng, n, sep, pi, scale=1.0):
    """window sums of n reads at a position where a share pi is modified: unit-spread levels `sep` apart, s = sep x - sep^2 / 2"""
    z = rng.random(n) < pi
    x = rng.normal(size=n) + sep * z
    return scale * (sep * x - 0.5 * sep * sep)


SEPARATIONS = (0.3, 1.0, 3.0, 8.0)
SHARES = (0.0, 0.02, 0.5, 0.98, 1.0)
# a lane's register chain; the sub-wave / wave step; the wave / workgroup step; the LDS-staged limit of the workgroup form
PARITY_LENGTHS = (0, 1, 2, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, STAGE, STAGE + 1)


def _csr(rows):
    off = np.zeros(len(rows) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rows])
    return (np.concatenate(rows) if rows else np.zeros(0)), off


@functools.lru_cache(maxsize=None)
def parity_batch():
    """(score, off): two rows of every length of PARITY_LENGTHS, shares and separations rotating"""
    rng = np.random.default_rng(1401)
    rows = []
    for i, n in enumerate(PARITY_LENGTHS):
        for j in range(2):
            sep, pi = SEPARATIONS[(i + 2 * j) % 4], (0.5, 0.02, 0.98, 0.3)[(i + j) % 4]
            rows.append(simulate_row(rng, n, sep, pi))
    return _csr(rows)


@functools.lru_cache(maxsize=None)
def content_batch():
    """(score, off): every separation at every share, in rows of 60 (16 lanes), 300 (a wave) and — at 3 sd — 1 500 (a workgroup); rows
    of scaled sums; rows holding +-800, +-1e300, +-0.0, NaN and +-inf; rows with only invalid scores; flat rows"""
    rng = np.random.default_rng(1402)
    rows = []
    for sep in SEPARATIONS:
        for pi in SHARES:
            rows.append(simulate_row(rng, 60, sep, pi))
            rows.append(simulate_row(rng, 300, sep, pi))
    rows += [simulate_row(rng, 1500, 3.0, pi) for pi in SHARES]
    rows += [simulate_row(rng, 40, 1.0, 0.4, scale) for scale in (5.0, 40.0)]
    nan, inf = np.nan, np.inf
    rows += [np.array([800.0, 800.0, 800.0, -800.0]), np.array([-800.0] * 5), np.array([800.0] * 5),
             np.array([1e300, -1e300, 1e300, 2.0, -1.0]), np.array([1.5e308, 1.5e308, 1e300, -3.0]),
             np.array([0.0, -0.0, 0.0, 0.0]), np.array([0.0, -0.0, 1.0, -2.0, 0.5]),
             np.array([nan, 2.0, -1.0, inf, 0.7, -inf, -0.2]), np.array([nan, inf, -inf]), np.array([nan] * 20),
             np.array([nan, 1.0, nan, -1.0]), np.array([5.0]), np.array([-5.0]), np.array([3.0, -0.5]),
             np.concatenate([simulate_row(rng, 280, 3.0, 0.5), [nan, inf, 800.0, -800.0, 1e300, -1e300, 0.0, -0.0]]),
             np.concatenate([simulate_row(rng, 1100, 1.0, 0.5), [nan, inf, 800.0, -800.0, 1e300, -1e300, 0.0, -0.0]])]
    return _csr(rows)


@functools.lru_cache(maxsize=None)
def expected(which, **opts):
    """the restatement over parity_batch / content_batch, computed once"""
    score, off = parity_batch() if which == 'parity' else content_batch()
    return site_stoich(score, off, **opts)
