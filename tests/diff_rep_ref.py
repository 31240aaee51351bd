"""The definition of nmod_site_diff_rep (include/nanomod_hip.h, K24) restated in numpy — stoich_ref's evaluation per sample, diff_ref's
condition level over the two super-rows, the reductions by math.fsum — the same problem in 50-digit mpmath, the gates derived as
diff_ref.site derives them (root_gate, _sum_err, _g_err and stoich_ref's constants; no constant of its own), the seeded sites that the
CPU pin (tests/test_site_diff_rep.py) and the GPU parity tests (tests/test_site_diff_rep_gpu.py) share, and the seeded null simulation.
Written from the header's text; the reference project has no such step.

Gates.  Per sample, pi_s has diff_ref's root gate and g_g(pi_s) the error of g at a maximiser; g_sat sums them and adds the roundings
of its G - 1 additions.  stat_het, phi and F carry the propagated errors of g_sat and g_cond; p_het and p_rep are [lo, hi] ranges
between the tails at both ends of their statistic's gate, widened by P_TAIL, the relative bound tests/test_tails_gpu.py (P_REL)
already holds the device's Student t and chi2 tails to."""
import functools
import math

import numpy as np

import diff_ref as D
import stoich_ref as sr
from stoich_ref import EPS, DBL_MIN

TOO_FEW, FLAT, NOT_CONVERGED, POOL_AT_END, PHI_ZERO, TOO_LARGE = 1, 2, 4, 8, 16, 32
NO_ESTIMATE = TOO_FEW | FLAT | TOO_LARGE
MAX_SAMPLES = 16
COND_FIELDS = ('pi0', 'pi1', 'pi_pool', 'delta', 'delta_lo', 'delta_hi', 'stat_cond', 'p_cond')
FIELDS = COND_FIELDS + ('stat_het', 'p_het', 'phi', 'p_rep')
SMALL, WAVE, STAGE = D.SMALL, D.WAVE, D.STAGE
P_TAIL = 1e-9                      # tests/test_tails_gpu.py: P_REL


def chi2_sf(stat, df):
    """the chi2_df tail by the header's closed forms, x = stat / 2"""
    x = 0.5 * stat
    if not x > 0.0:
        return 1.0
    if math.isinf(x):
        return 0.0
    if df % 2 == 0:
        return min(math.fsum(math.exp(-x + m * math.log(x) - math.lgamma(m + 1.0)) for m in range(df // 2)), 1.0)
    return min(math.erfc(math.sqrt(x)) + math.fsum(math.exp(-x + (j - 0.5) * math.log(x) - math.lgamma(j + 0.5)) for j in range(1, (df - 1) // 2 + 1)), 1.0)


def t_two_sided(F, df):
    """the F(1, df) tail of F, the two-sided Student t tail of sqrt(F): I_{df / (df + F)}(df / 2, 1 / 2)"""
    from scipy.special import betainc
    if F == 0.0:
        return 1.0
    if math.isinf(F):
        return 0.0
    return float(betainc(0.5 * df, 0.5, df / (df + F)))


def f1_quantile(level, df):
    """the `level` quantile of F(1, df) (scipy: the reference of the package's own helper, engine._f1_quantile)"""
    from scipy import stats
    return float(stats.t.ppf(0.5 * (1.0 + level), df)) ** 2


def p_het_of(stat_het, df):
    return max(chi2_sf(stat_het, df), DBL_MIN)


def p_rep_of(stat_cond, phi, phi_floor, df):
    """(p_rep, whether NMOD_REP_PHI_ZERO)"""
    phi_used = max(phi, phi_floor)
    if stat_cond == 0.0:
        return 1.0, False
    if phi_used == 0.0:
        return DBL_MIN, True
    return max(t_two_sided(stat_cond / phi_used, df), DBL_MIN), False


def _nan_site(G, n_valid, status):
    r = {f: np.nan for f in FIELDS}
    r.update(pi_s=np.full(G, np.nan), n_valid=np.asarray(n_valid, np.int32), iters=0, status=status, gates=None)
    return r


def _alone(w, n, max_iter, tol):
    """K14's estimate of one sample: (pi, not converged, the evaluation at pi, its root gate, the error of g there)"""
    z, o = sr.evaluate(w, 0.0), sr.evaluate(w, 1.0)
    if z['S'] <= 0.0:
        pi, nc = 0.0, False
    elif o['S'] >= 0.0:
        pi, nc = 1.0, False
    else:
        pi, _, nc = sr.solve(w, 0, 0.0, 1.0, 0.0, 0.0, max_iter, tol)
    e = sr.evaluate(w, pi)
    gate = tol + 2.0 * EPS + D._sum_err(n + 1, e) / e['D'] if 0.0 < pi < 1.0 else 0.0
    g_err = D._g_err(n, e) + 0.5 * e['D'] * gate ** 2 if math.isfinite(e['g']) else 0.0
    return pi, nc, e, gate, g_err


def site(rows, n_control, min_valid=3, max_iter=60, tol=1e-12, ci_drop=None, phi_floor=0.0, interval=True):
    """one site by the header's definition: rows, the G sample rows, the first n_control of them condition 0.  Its outputs and `gates`
    (None without an estimate).  ci_drop: the quantile of F(1, G - 2) the caller passes (default: the 0.95 one)"""
    rows = [np.asarray(r, dtype=np.float64) for r in rows]
    G = len(rows)
    df = G - 2
    assert 3 <= G <= MAX_SAMPLES and 1 <= n_control <= G - 1
    if ci_drop is None:
        ci_drop = f1_quantile(0.95, df)
    n = [int(sr._valid(r).sum()) for r in rows]
    s0, s1 = np.concatenate(rows[:n_control]), np.concatenate(rows[n_control:])
    if max(len(s0), len(s1)) > 16777215:
        return _nan_site(G, [0] * G, TOO_LARGE)
    if min(n) < min_valid:
        return _nan_site(G, n, TOO_FEW)
    ws = [sr.signed_t(r) for r in rows]
    if any(not math.fsum(np.abs(w)) > 0.0 for w in ws):
        return _nan_site(G, n, FLAT)
    # the saturated fit
    sat = [_alone(w, m, max_iter, tol) for w, m in zip(ws, n)]
    pi_s = np.array([s[0] for s in sat])
    gsat = 0.0
    with np.errstate(invalid='ignore'):
        for s in sat:
            gsat = gsat + s[2]['g']                                 # ascending g, one rounding each
    gsat_err = sum(s[4] for s in sat) + (G - 1) * EPS * sum(abs(s[2]['g']) for s in sat if math.isfinite(s[2]['g']))
    # the condition level: nmod_site_diff of the two super-rows, without its interval (the drop is not known yet)
    c = D.site(s0, s1, min_valid=min_valid, max_iter=max_iter, tol=tol, ci_drop=1.0, interval=False)
    assert c['gates'] is not None
    w0, w1 = sr.signed_t(s0), sr.signed_t(s1)
    n0, n1 = c['n_valid0'], c['n_valid1']
    h0, h1 = D._pair(w0, w1, c['pi0'], c['pi1'])
    with np.errstate(invalid='ignore'):
        ghat = h0['g'] + h1['g']
        stat_het = max(2.0 * (gsat - ghat), 0.0) if not math.isnan(gsat - ghat) else 0.0
    gh_err = D._g_err(n0, h0) + D._g_err(n1, h1) + 0.5 * (h0['D'] * c['gates']['pi0'] ** 2 + h1['D'] * c['gates']['pi1'] ** 2) + EPS * abs(ghat) \
        if math.isfinite(ghat) else 0.0
    g_het = 2.0 * (gsat_err + gh_err) + 4.0 * EPS * stat_het
    phi = stat_het / df
    g_phi = g_het / df + EPS * phi
    phi_used = max(phi, phi_floor)
    stat = c['stat']
    g_stat = c['gates']['stat']
    p_rep, phi_zero = p_rep_of(stat, phi, phi_floor, df)
    # the ranges of the tails: each is decreasing in its statistic
    ph = lambda st: p_het_of(max(st, 0.0), df)
    het_rng = (ph(stat_het + g_het) * (1.0 - P_TAIL), ph(stat_het - g_het) * (1.0 + P_TAIL))
    g_used = g_phi if phi > phi_floor - g_phi else 0.0              # (the floor itself is exact)
    if stat == 0.0 or phi_zero:
        rep_rng = (p_rep, p_rep)
    else:
        f_lo = max(stat - g_stat, 0.0) / (phi_used + g_used) * (1.0 - 4.0 * EPS)
        f_hi = (stat + g_stat) / (phi_used - g_used) * (1.0 + 4.0 * EPS) if phi_used > g_used else math.inf
        pr = lambda F: max(t_two_sided(F, df), DBL_MIN)
        rep_rng = (pr(f_hi) * (1.0 - P_TAIL), min(pr(f_lo) * (1.0 + P_TAIL), 1.0))
    gates = dict(c['gates'])
    gates.update(stat_cond=gates.pop('stat'), p_cond=gates.pop('p_diff'), stat_het=g_het, phi=g_phi, p_het=het_rng, p_rep=rep_rng,
                 pi_s=np.array([s[3] for s in sat]))
    res = dict(pi_s=pi_s, n_valid=np.asarray(n, np.int32), pi0=c['pi0'], pi1=c['pi1'], pi_pool=c['pi_pool'], delta=c['delta'], delta_lo=np.nan,
               delta_hi=np.nan, stat_cond=stat, p_cond=c['p_diff'], stat_het=stat_het, p_het=p_het_of(stat_het, df), phi=phi, p_rep=p_rep,
               iters=c['iters'], gates=gates, phi_used=phi_used, drop=phi_used * ci_drop)
    nc = bool(c['status'] & NOT_CONVERGED) or any(s[1] for s in sat)
    if interval and phi_used * ci_drop > 0.0:
        ci = D.site(s0, s1, min_valid=min_valid, max_iter=max_iter, tol=tol, ci_drop=phi_used * ci_drop, interval=True)
        res.update(delta_lo=ci['delta_lo'], delta_hi=ci['delta_hi'])
        gates.update(delta_lo=ci['gates']['delta_lo'], delta_hi=ci['gates']['delta_hi'])
        nc = nc or bool(ci['status'] & NOT_CONVERGED)
    elif interval:                                                  # a drop of 0: the interval is the point delta, no root is run
        res.update(delta_lo=c['delta'], delta_hi=c['delta'])
        gates.update(delta_lo=gates['delta'], delta_hi=gates['delta'])
    res['status'] = (NOT_CONVERGED if nc else 0) | (POOL_AT_END if c['pi_pool'] in (0.0, 1.0) else 0) | (PHI_ZERO if phi_zero else 0)
    return res


DEFAULTS = dict(min_valid=3, max_iter=60, tol=1e-12)


def split(score, off, G):
    """the sites of a CSR batch: a list of lists of G rows"""
    return [[score[off[i * G + g]:off[i * G + g + 1]] for g in range(G)] for i in range((len(off) - 1) // G)]


def site_diff_rep(score, off, G, n_control, **opts):
    o = dict(DEFAULTS, **opts)
    return [site(rows, n_control, **o) for rows in split(score, off, G)]


def csr(sites):
    """(score, off) of a list of sites, each a list of G rows, site-major"""
    return sr._csr([np.asarray(r, np.float64) for rows in sites for r in rows])


# ---- the same problem in 50 digits
def exact_site(rows, n_control, phi_floor=0.0):
    """pi_s, the condition level (diff_ref.exact_site without its interval), stat_het, p_het, phi and p_rep in 50 digits"""
    import mpmath as mp
    G = len(rows)
    df = G - 2
    with mp.workdps(50):
        def fit(s):
            v = [mp.mpf(float(x)) for x in s if abs(x) <= sr.DBL_MAX]
            e, plus = [mp.exp(-abs(x)) for x in v], [x >= 0 for x in v]
            den = lambda x, ei, p: (x + (1 - x) * ei) if p else ((1 - x) + x * ei)
            S = lambda x: mp.fsum((1 - ei) / den(x, ei, p) * (1 if p else -1) for ei, p in zip(e, plus))
            g = lambda x: mp.fsum(mp.log(den(x, ei, p)) for ei, p in zip(e, plus))
            zero, one = mp.mpf(0), mp.mpf(1)
            if S(zero) <= 0:
                return zero, g(zero)
            if S(one) >= 0:
                return one, g(one)
            a, b = zero, one
            for _ in range(170):
                m = (a + b) / 2
                a, b = (m, b) if S(m) > 0 else (a, m)
            return (a + b) / 2, g((a + b) / 2)
        sat = [fit(r) for r in rows]
        gsat = mp.fsum(s[1] for s in sat)
        (pi0, g0), (pi1, g1) = fit(np.concatenate(rows[:n_control])), fit(np.concatenate(rows[n_control:]))
        pip, gp = fit(np.concatenate(rows))
        stat = max(2 * (g0 + g1 - gp), mp.mpf(0))
        stat_het = max(2 * (gsat - g0 - g1), mp.mpf(0))
        phi = stat_het / df
        used = max(phi, mp.mpf(phi_floor))
        p_het = mp.gammainc(mp.mpf(df) / 2, stat_het / 2, mp.inf, regularized=True)
        if stat == 0:
            p_rep = mp.mpf(1)
        elif used == 0:
            p_rep = mp.mpf(DBL_MIN)
        else:
            F = stat / used
            p_rep = mp.betainc(mp.mpf(df) / 2, mp.mpf(1) / 2, 0, df / (df + F), regularized=True)
        return dict(pi_s=[s[0] for s in sat], pi0=pi0, pi1=pi1, pi_pool=pip, delta=pi1 - pi0, stat_cond=stat, stat_het=stat_het, phi=phi,
                    p_cond=max(mp.erfc(mp.sqrt(stat / 2)), mp.mpf(DBL_MIN)), p_het=max(p_het, mp.mpf(DBL_MIN)), p_rep=max(p_rep, mp.mpf(DBL_MIN)))


# ---- seeded sites
ODD_LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65)               # sample lengths that break the lane alignment of a super-row (and 0)
CONFIGS = tuple((G, nc) for G in (3, 4, 7, 16) for nc in sorted({1, G - 1, G // 2}))
LENGTH_MIN_VALID = 1                                                # so that the samples of 1 and 2 scores carry an estimate


def _split_total(total, k, start):
    """k sample lengths that sum to total: ODD_LENGTHS from `start` on while they fit, the last sample takes the rest"""
    out = []
    for j in range(k - 1):
        n = ODD_LENGTHS[(start + j) % len(ODD_LENGTHS)]
        out.append(n if sum(out) + n < total - (k - 1 - j) else 1)
    return out + [total - sum(out)]


def _sim_site(rng, lens, n_control, sep, p0, p1):
    return [sr.simulate_row(rng, n, sep, p0 if g < n_control else p1) for g, n in enumerate(lens)]


# the super-row lengths at K15's steps, by class; every configuration takes one of each in turn
_SMALL_L, _WAVE_L, _BLOCK_L = (SMALL - 1, SMALL, SMALL + 1 - 2), (WAVE - 1, WAVE, SMALL + 1), (WAVE + 1, 700, 1300)


@functools.lru_cache(maxsize=None)
def length_batches():
    """{(G, n_control): list of sites}: per configuration a site of each class of K15 with the longer super-row at or next to a class
    step (127, 128, 129, 511, 512, 513 all occur), samples of ODD_LENGTHS inside it, the longer condition alternating; lopsided sites
    (a sample of 3 beside one past the wave step); both super-rows staged at 6144 words in all and at 6145; a sample of 0 scores"""
    rng = np.random.default_rng(2401)
    out = {}
    for ci, (G, nc) in enumerate(CONFIGS):
        sites = []
        for cls, longs in enumerate((_SMALL_L, _WAVE_L, _BLOCK_L)):
            long_len = longs[ci % 3]
            short_len = (max(G, 40), long_len, long_len - 5)[(ci + cls) % 3]
            k0, k1 = nc, G - nc
            first_long = (ci + cls) % 2 == 0
            l0 = _split_total(long_len if first_long else short_len, k0, ci + cls)
            l1 = _split_total(short_len if first_long else long_len, k1, ci + 2 * cls + 3)
            sites.append(_sim_site(rng, l0 + l1, nc, sr.SEPARATIONS[1 + (ci + cls) % 3], (0.3, 0.5, 0.1)[ci % 3], (0.3, 0.7, 0.6)[cls]))
        out[(G, nc)] = sites
    # the exact steps every class test names, in the configurations where the rotation above left them out
    out[(3, 1)].append(_sim_site(rng, [SMALL + 1, 60, 69], 1, 3.0, 0.4, 0.5))          # 129 against 129
    out[(4, 2)].append(_sim_site(rng, [500, 13, 17, 33], 2, 3.0, 0.4, 0.6))            # 513 against 50
    out[(7, 3)].append(_sim_site(rng, [100, 400, 11, 9, 200, 300, 3], 3, 1.0, 0.2, 0.3))   # 511 against 512
    # lopsided
    out[(3, 1)].append(_sim_site(rng, [3, WAVE + 8, 30], 1, 3.0, 0.5, 0.5))
    out[(3, 2)].append(_sim_site(rng, [3, WAVE + 3, 40], 2, 3.0, 0.5, 0.3))
    # the stage limit
    out[(4, 2)].append(_sim_site(rng, [3000, 2444, 600, 100], 2, 3.0, 0.3, 0.4))       # 6144 words in all
    out[(4, 2)].append(_sim_site(rng, [3000, 2444, 600, 101], 2, 3.0, 0.3, 0.4))       # 6145: read again per evaluation
    out[(3, 1)].append(_sim_site(rng, [STAGE - 1000, 563, 437], 1, 1.0, 0.5, 0.5))     # 6144, 1 v 2
    # an empty sample
    out[(7, 3)].append(_sim_site(rng, [0, 5, 9, 16, 17, 63, 64], 3, 3.0, 0.5, 0.5))
    out[(16, 8)].append(_sim_site(rng, list(ODD_LENGTHS) + [1, 2, 7, 8, 9], 8, 3.0, 0.4, 0.6))
    return out


def _const(n, v):
    return np.full(n, float(v))


@functools.lru_cache(maxsize=None)
def content_sites():
    """G = 4, n_control = 2: shares at 0 and 1 in a sample, a condition and the pool; NaN, +-inf, -0.0, |s| > 37; a flat sample; a sample
    below min_valid = 3; the constructed PHI_ZERO site; overdispersed and homogeneous replicates"""
    rng = np.random.default_rng(2402)
    sim = lambda n, sep, p: sr.simulate_row(rng, n, sep, p)
    nan, inf = np.nan, np.inf
    sites = []
    for sep in (1.0, 3.0, 8.0):
        sites += [[sim(20, sep, 0.3), sim(25, sep, 0.3), sim(18, sep, 0.3), sim(30, sep, 0.3)],          # homogeneous null
                  [sim(20, sep, 0.1), sim(25, sep, 0.5), sim(18, sep, 0.2), sim(30, sep, 0.6)],          # overdispersed null
                  [sim(20, sep, 0.1), sim(25, sep, 0.15), sim(18, sep, 0.8), sim(30, sep, 0.85)],        # a difference
                  [sim(20, sep, 0.0), sim(25, sep, 0.4), sim(18, sep, 0.5), sim(30, sep, 1.0)],          # a share at an end in a sample
                  [sim(20, sep, 0.0), sim(25, sep, 0.0), sim(18, sep, 0.5), sim(30, sep, 0.6)],          # ... in a condition
                  [sim(20, sep, 1.0), sim(25, sep, 1.0), sim(18, sep, 1.0), sim(30, sep, 1.0)],          # ... in the pool
                  [sim(20, sep, 0.0), sim(25, sep, 0.0), sim(18, sep, 0.0), sim(30, sep, 0.0)]]
    plain = lambda: sim(15, 3.0, 0.5)
    sites += [[_const(6, -40), _const(5, -40), _const(7, 40), _const(4, 40)],                            # every g is 0: PHI_ZERO
              [np.array([800.0, 800.0, 800.0, -800.0]), plain(), plain(), np.array([-800.0] * 5)],
              [np.array([1e300, -1e300, 1e300, 2.0, -1.0]), plain(), np.array([800.0] * 5), plain()],
              [np.array([0.0, -0.0, 1.0, -2.0, 0.5]), plain(), plain(), np.array([-0.0, 3.0, -3.0, 0.25])],
              [np.array([nan, 2.0, -1.0, inf, 0.7, -inf, -0.2]), plain(), np.array([nan, nan, 1.0, -1.0, 2.0, -inf]), plain()],
              [plain(), np.array([0.0, -0.0, 0.0, 0.0]), plain(), plain()],                              # FLAT
              [plain(), plain(), np.array([nan, inf, 1.0, -2.0]), plain()],                              # two valid scores: TOO_FEW
              [plain(), plain(), plain(), np.array([3.0, -0.5])],
              [np.array([nan, inf, -inf, nan]), plain(), plain(), plain()]]
    return sites


@functools.lru_cache(maxsize=None)
def expected(which, key=None, **opts):
    """the restatement over one of length_batches() (which = 'length', key = (G, n_control), min_valid = LENGTH_MIN_VALID unless given)
    or over content_sites() (G = 4, n_control = 2), computed once"""
    if which == 'length':
        G, nc = key
        o = dict(DEFAULTS, min_valid=LENGTH_MIN_VALID)
        o.update(opts)
        return [site(rows, nc, **o) for rows in length_batches()[key]]
    return [site(rows, 2, **dict(DEFAULTS, **opts)) for rows in content_sites()]


# ---- the seeded null simulation
SIM_CELLS = (('3v3 rho 0', 3, 3, 0.0), ('3v3 rho 0.05', 3, 3, 0.05), ('3v3 rho 0.15', 3, 3, 0.15), ('2v2 rho 0.1', 2, 2, 0.1))
SIM_SITES, SIM_READS, SIM_SEP, SIM_SHARE = 400, 50, 2.0, 0.3


@functools.lru_cache(maxsize=None)
def simulate_null(cell):
    """SIM_SITES seeded null sites of a cell of SIM_CELLS: both conditions at SIM_SHARE, every replicate's share drawn
    Beta(share (1 - rho) / rho, (1 - share) (1 - rho) / rho) (rho 0: the share itself), SIM_READS reads each, levels SIM_SEP sd apart.
    Returns the 5 % rejection rates dict(p_cond, p_rep, p_rep_floor1, p_het) and the number of sites with an estimate"""
    name, k0, k1, rho = SIM_CELLS[cell]
    rng = np.random.default_rng(2410 + cell)
    G, df = k0 + k1, k0 + k1 - 2
    rej = dict(p_cond=0, p_rep=0, p_rep_floor1=0, p_het=0)
    n = 0
    for _ in range(SIM_SITES):
        shares = [SIM_SHARE] * G if rho == 0.0 else rng.beta(SIM_SHARE * (1.0 - rho) / rho, (1.0 - SIM_SHARE) * (1.0 - rho) / rho, G)
        r = site([sr.simulate_row(rng, SIM_READS, SIM_SEP, p) for p in shares], k0, interval=False)
        if r['gates'] is None:
            continue
        n += 1
        rej['p_cond'] += r['p_cond'] <= 0.05
        rej['p_rep'] += r['p_rep'] <= 0.05
        rej['p_rep_floor1'] += p_rep_of(r['stat_cond'], r['phi'], 1.0, df)[0] <= 0.05
        rej['p_het'] += r['p_het'] <= 0.05
    return {k: v / n for k, v in rej.items()}, n
