"""The definitions of nmod_rep_prior and nmod_site_diff_rep_mod (include/nanomod_hip.h, K25) restated in numpy on top of diff_rep_ref:
the prior fit with scipy.special.polygamma and math.fsum, the moderated site on diff_rep_ref.site (its three fits, its phi and its
gates unchanged), the same quantities in 50-digit mpmath, the per-site gates built the way diff_rep_ref builds them, and the seeded
null and planted simulations.  Written from the header's text; the reference project has no such step.

Gates.  phi_post carries phi's gate scaled by df / (d0 + df) and the roundings of its five operations; the p_rep gate is the image
of the gates of stat_cond and phi_post under the monotone tail, widened by diff_rep_ref.P_TAIL; the interval ends have diff_ref's
gates at the moderated drop.  The scalar functions carry the deviations from mpmath that tests/test_site_diff_mod.py measures over
its grids (MEASURED below), each gated at twice its measured value."""
import functools
import math

import numpy as np

import diff_ref as D
import diff_rep_ref as R
import stoich_ref as sr
from stoich_ref import EPS, DBL_MIN

BAD_PRIOR = 64
PRIOR_WORDS, PRIOR_CHUNK = 8, 1024
PRIOR_FIELDS = ('d0', 's0sq', 'df_tot', 'ci_drop', 'n_used', 'n_zero', 'emean', 'evar')
NUS = tuple(range(1, 15)) + (2.37, 14.6, 1e6, math.inf)
LEVELS = (0.9, 0.95, 0.999)

# the worst relative deviation of this file's functions from 50-digit mpmath over the grids of tests/test_site_diff_mod.py, which
# measures them again and holds them to MARGIN times these values (profiles/site_diff_mod.txt records them)
MEASURED = dict(trigamma_inverse=3.9e-16, d0=1.5e-14, s0sq=5.4e-16, f1_quantile=5.7e-16, tail=1.5e-14)
MARGIN = 2.0
# the device's own functions against mpmath (special_math.hpp, compiled for the host in tests/test_site_diff_mod.py): the quantile is a
# bisection of student_t_two_sided, whose log1p(-y) loses digits near y = 1 (df 1, level 0.999: t = 637)
DEVICE_MEASURED = dict(digamma=1.4e-15, trigamma=6.7e-16, tetragamma=7.2e-16, trigamma_inverse=4.3e-16, f1_quantile=2.0e-11)


def digamma(x):
    from scipy.special import polygamma
    return float(polygamma(0, x))


def trigamma(x):
    from scipy.special import polygamma
    return float(polygamma(1, x))


def trigamma_inverse(x):
    """the header's Newton iteration on 1 / psi' with its start, stop rule and the two asymptotic ends"""
    from scipy.special import polygamma
    if x != x:
        return x
    if x > 1e7:
        return 1.0 / math.sqrt(x)
    if x < 1e-6:
        return 1.0 / x
    y = 0.5 + 1.0 / x
    for _ in range(50):
        tri = float(polygamma(1, y))
        dif = tri * (1.0 - tri / x) / float(polygamma(2, y))
        y += dif
        if -dif / y < 1e-8:
            break
    return y


def f1_quantile(level, nu):
    """the `level` quantile of F(1, nu), real nu; nu = inf: the chi2_1 quantile"""
    from scipy import stats
    alpha = 1.0 - level
    if math.isinf(nu):
        return float(stats.norm.isf(0.5 * alpha)) ** 2
    t = float(stats.t.isf(0.5 * alpha, nu))                         # (good to 5e-11 only: three Newton steps on the tail below)
    for _ in range(3):
        t += (tail(t * t, nu) - alpha) / (2.0 * float(stats.t.pdf(t, nu)))
    return t * t


def tail(F, nu):
    """the two-sided Student t tail of sqrt(F) on nu degrees of freedom, 1 - I_{F / (nu + F)}(1 / 2, nu / 2) (the complement as scipy
    has it: diff_rep_ref.t_two_sided's argument nu / (nu + F) rounds to 1 for a large nu; that form where F > nu); nu = inf: erfc(sqrt(F / 2))"""
    from scipy.special import betainc, betaincc
    if F == 0.0:
        return 1.0
    if math.isinf(F):
        return 0.0
    if math.isinf(nu):
        return math.erfc(math.sqrt(0.5 * F))
    if F > nu:                                                      # (the argument that is not close to 1)
        return float(betainc(0.5 * nu, 0.5, nu / (nu + F)))
    return float(betaincc(0.5, 0.5 * nu, F / (nu + F)))


def solve(emean, evar, n, df, level):
    """(d0, s0sq, df_tot, ci_drop) from the moments: the header's three cases"""
    if n < 2:
        d0, s0 = 0.0, math.nan
    elif evar > 0.0:
        d0 = 2.0 * trigamma_inverse(evar)
        s0 = math.exp(emean + digamma(0.5 * d0) - math.log(0.5 * d0))
    else:
        d0, s0 = math.inf, math.exp(emean)
    return d0, s0, df + d0, f1_quantile(level, df + d0)


def rep_prior(phi, status, df, ci_level=0.95):
    """the record as a dict of PRIOR_FIELDS, and what its gates are made of: e (the sites of the fit, in order), abs_e = sum |e_i|,
    sq = sum (e_i - emean)^2 (both by math.fsum)"""
    phi, status = np.asarray(phi, np.float64), np.asarray(status, np.uint8)
    est = (status & R.NO_ESTIMATE) == 0
    with np.errstate(invalid='ignore'):
        used = est & np.isfinite(phi) & (phi > 0.0)
        zero = est & (phi <= 0.0)
    n = int(used.sum())
    e = np.log(phi[used]) - digamma(0.5 * df) + math.log(0.5 * df)
    emean = math.fsum(e) / n if n else math.nan
    sq = math.fsum((e - emean) ** 2) if n else 0.0
    evar = sq / (n - 1) - trigamma(0.5 * df) if n >= 2 else math.nan
    d0, s0, dft, drop = solve(emean, evar, n, df, ci_level)
    return dict(d0=d0, s0sq=s0, df_tot=dft, ci_drop=drop, n_used=float(n), n_zero=float(zero.sum()), emean=emean, evar=evar,
                e=e, abs_e=math.fsum(np.abs(e)), sq=sq)


def record(p):
    return np.array([p[f] for f in PRIOR_FIELDS], np.float64)


def prior_gates(p, df, level=0.95):
    """How far the device's record may lie from rep_prior's.  emean and evar: the summation bound (n + 4) 2^-52 sum |e_i| (sum
    (e_i - emean)^2 for evar) of the issue, over n (n - 1), and for evar the representation of psi'(df / 2) and of the difference
    (DEVICE_MEASURED's trigamma, one rounding).  d0, s0sq, ci_drop: the measured deviations of both sides' functions, and the gates of
    emean and evar carried through the solve by evaluating it at both ends (each is monotone in each moment)"""
    n = int(p['n_used'])
    u = 2.0 ** -52
    g = dict(emean=0.0, evar=0.0, d0=0.0, s0sq=0.0, ci_drop=0.0, df_tot=0.0)
    level_gate = MARGIN * (MEASURED['f1_quantile'] + DEVICE_MEASURED['f1_quantile'])
    if n >= 1:
        g['emean'] = (n + 4) * u * p['abs_e'] / n
    if n < 2:
        g['ci_drop'] = level_gate * p['ci_drop']
        return g
    tri = trigamma(0.5 * df)
    g['evar'] = (n + 4) * u * p['sq'] / (n - 1) + (MARGIN * DEVICE_MEASURED['trigamma'] + EPS) * tri + EPS * abs(p['evar'])
    if math.isinf(p['d0']):
        g['s0sq'] = p['s0sq'] * (g['emean'] + 4.0 * EPS)
        g['ci_drop'] = level_gate * p['ci_drop']
        return g
    inv_gate = MARGIN * (MEASURED['trigamma_inverse'] + DEVICE_MEASURED['trigamma_inverse'])
    ends = [solve(p['emean'] + a * g['emean'], p['evar'] + b * g['evar'], n, df, 0.95)[:3] for a in (-1, 1) for b in (-1, 1)
            if p['evar'] + b * g['evar'] > 0.0]
    g['d0'] = max(abs(x[0] - p['d0']) for x in ends) + inv_gate * p['d0']
    g['df_tot'] = g['d0'] + EPS * p['df_tot']
    psi_gate = MARGIN * DEVICE_MEASURED['digamma'] * max(1.0, abs(digamma(0.5 * p['d0']))) + 4.0 * EPS * (abs(p['emean']) + abs(math.log(0.5 * p['d0'])))
    g['s0sq'] = max(abs(x[1] - p['s0sq']) for x in ends) + p['s0sq'] * (psi_gate + inv_gate * max(1.0, 0.5 * p['d0'] * abs(trigamma(0.5 * p['d0']) - 2.0 / p['d0'])) + 4.0 * EPS)
    lo, hi = f1_quantile(level, df + p['d0'] - g['d0']), f1_quantile(level, df + p['d0'] + g['d0'])
    g['ci_drop'] = abs(hi - lo) + level_gate * p['ci_drop']
    return g


# ---- the moderated site
def prior_bad(prior):
    d0, s0, dft, ci = (float(v) for v in prior[:4])
    return d0 != d0 or dft != dft or (d0 > 0.0 and s0 != s0) or d0 < 0.0 or s0 < 0.0 or dft < 0.0 or ci < 0.0


def phi_post_of(phi, prior, df):
    d0, s0 = float(prior[0]), float(prior[1])
    if d0 == 0.0:
        return phi
    if math.isinf(d0):
        return s0
    return (d0 * s0 + df * phi) / (d0 + df)


def p_rep_of(stat_cond, phi_post, phi_floor, dft):
    """(p_rep, whether NMOD_REP_PHI_ZERO)"""
    phi_used = max(phi_post, phi_floor)
    if stat_cond == 0.0:
        return 1.0, False
    if phi_used == 0.0:
        return DBL_MIN, True
    return max(tail(stat_cond / phi_used, dft), DBL_MIN), False


def site(rows, n_control, prior, phi_floor=0.0, interval=True, min_valid=3, max_iter=60, tol=1e-12, base=None):
    """one site by the header's definition under the record `prior`: diff_rep_ref.site's outputs and gates for everything that does not
    change, then phi_post, p_rep, the interval at phi_used * prior[3] and the status.  base: diff_rep_ref.site's result for these rows
    and options where the caller has it already (with any drop and floor: neither reaches what is taken from it; its roots converged)"""
    G = len(rows)
    df = G - 2
    if base is None:
        base = R.site(rows, n_control, min_valid=min_valid, max_iter=max_iter, tol=tol, ci_drop=1.0, phi_floor=0.0, interval=False)
    else:
        assert not base['status'] & R.NOT_CONVERGED
    r = dict(base)
    bad = prior_bad(prior)
    if r['gates'] is None:
        r.update(phi_post=np.nan, status=r['status'] | (BAD_PRIOR if bad else 0))
        return r
    status = r['status'] & ~R.PHI_ZERO
    gates = dict(r['gates'])
    r['gates'] = gates
    if bad:
        r.update(phi_post=np.nan, p_rep=np.nan, delta_lo=np.nan, delta_hi=np.nan, status=status | BAD_PRIOR, phi_used=np.nan)
        gates.update(phi_post=None, p_rep=None, delta_lo=None, delta_hi=None)
        return r
    d0, dft, ci_drop = float(prior[0]), float(prior[2]), float(prior[3])
    phi, g_phi = r['phi'], gates['phi']
    post = phi_post_of(phi, prior, df)
    g_post = g_phi if d0 == 0.0 else (0.0 if math.isinf(d0) else df * g_phi / (d0 + df) + 4.0 * EPS * post)
    phi_used = max(post, phi_floor)
    stat, g_stat = r['stat_cond'], gates['stat_cond']
    p_rep, phi_zero = p_rep_of(stat, post, phi_floor, dft)
    g_used = g_post if post > phi_floor - g_post else 0.0
    if stat == 0.0 or phi_zero:
        rng = (p_rep, p_rep)
    else:
        f_lo = max(stat - g_stat, 0.0) / (phi_used + g_used) * (1.0 - 4.0 * EPS)
        f_hi = (stat + g_stat) / (phi_used - g_used) * (1.0 + 4.0 * EPS) if phi_used > g_used else math.inf
        pr = lambda F: max(tail(F, dft), DBL_MIN)
        rng = (pr(f_hi) * (1.0 - R.P_TAIL), min(pr(f_lo) * (1.0 + R.P_TAIL), 1.0))
    gates.update(phi_post=g_post, p_rep=rng, delta_lo=None, delta_hi=None)
    r.update(phi_post=post, p_rep=p_rep, phi_used=phi_used, drop=phi_used * ci_drop, delta_lo=np.nan, delta_hi=np.nan)
    nc = bool(status & R.NOT_CONVERGED)
    if interval and phi_used * ci_drop > 0.0:
        s0, s1 = np.concatenate(rows[:n_control]), np.concatenate(rows[n_control:])
        ci = D.site(s0, s1, min_valid=min_valid, max_iter=max_iter, tol=tol, ci_drop=phi_used * ci_drop, interval=True)
        r.update(delta_lo=ci['delta_lo'], delta_hi=ci['delta_hi'])
        gates.update(delta_lo=ci['gates']['delta_lo'], delta_hi=ci['gates']['delta_hi'])
        nc = nc or bool(ci['status'] & R.NOT_CONVERGED)
    elif interval:
        r.update(delta_lo=r['delta'], delta_hi=r['delta'])
        gates.update(delta_lo=gates['delta'], delta_hi=gates['delta'])
    r['status'] = (status & ~R.NOT_CONVERGED) | (R.NOT_CONVERGED if nc else 0) | (R.PHI_ZERO if phi_zero else 0)
    return r


@functools.lru_cache(maxsize=None)
def expected(which, key, prior, phi_floor=0.0, base_drop=None):
    """site() over diff_rep_ref.length_batches()[key] (which = 'length', min_valid = LENGTH_MIN_VALID) or content_sites() (G = 4,
    n_control = 2) under the record `prior` (a tuple), computed once.  base_drop: the ci_drop at which diff_rep_ref.expected holds (or
    will hold) the same sites for nmod_site_diff_rep's own tests: its three fits are then not run again"""
    if which == 'length':
        base = R.expected('length', key, ci_drop=base_drop) if base_drop is not None else [None] * len(R.length_batches()[key])
        return [site(rows, key[1], prior, phi_floor, min_valid=R.LENGTH_MIN_VALID, base=b) for rows, b in zip(R.length_batches()[key], base)]
    base = R.expected('content', ci_drop=base_drop, phi_floor=0.0) if base_drop is not None else [None] * len(R.content_sites())
    return [site(rows, 2, prior, phi_floor, base=b) for rows, b in zip(R.content_sites(), base)]


# ---- the same in 50 digits
def exact_trigamma_inverse(x):
    import mpmath as mp
    with mp.workdps(50):
        x = mp.mpf(x)
        return mp.findroot(lambda y: mp.polygamma(1, y) - x, mp.mpf(trigamma_inverse(float(x))))


def exact_solve(e, df):
    """(d0, s0sq) of the values e (doubles, taken as exact) in 50 digits; d0 = inf where evar <= 0"""
    import mpmath as mp
    with mp.workdps(50):
        v = [mp.mpf(float(x)) for x in e]
        n = len(v)
        m = mp.fsum(v) / n
        evar = mp.fsum((x - m) ** 2 for x in v) / (n - 1) - mp.polygamma(1, mp.mpf(df) / 2)
        if evar <= 0:
            return mp.inf, mp.exp(m)
        d0 = 2 * mp.findroot(lambda y: mp.polygamma(1, y) - evar, mp.mpf(trigamma_inverse(float(evar))))
        return d0, mp.exp(m + mp.digamma(d0 / 2) - mp.log(d0 / 2))


def exact_f1_quantile(level, nu):
    """of the double `level` (alpha = 1 - level taken exactly)"""
    import mpmath as mp
    with mp.workdps(50):
        alpha = 1 - mp.mpf(level)
        if math.isinf(nu):
            return 2 * mp.erfinv(1 - alpha) ** 2
        n = mp.mpf(nu)
        t = mp.findroot(lambda t: mp.betainc(n / 2, mp.mpf(1) / 2, 0, n / (n + t * t), regularized=True) - alpha, mp.sqrt(mp.mpf(f1_quantile(level, nu))))
        return t * t


def exact_tail(F, nu):
    import mpmath as mp
    with mp.workdps(50):
        F = mp.mpf(F)
        if math.isinf(nu):
            return mp.erfc(mp.sqrt(F / 2))
        n = mp.mpf(nu)
        return mp.betainc(n / 2, mp.mpf(1) / 2, 0, n / (n + F), regularized=True)


# ---- the seeded simulations: diff_rep_ref's cells (its seeds and its order of draws, so the null sites are its own), per site what the
# prior fit and both tests need; `planted`: the other condition's replicates drawn around SIM_SHARE + PLANTED[cell]
PLANTED = (0.12, 0.22, 0.36, 0.50)       # chosen so that K24's p_rep rejects a quarter to two fifths of the planted sites


@functools.lru_cache(maxsize=None)
def simulate(cell, planted=False):
    """dict(phi, status, stat_cond, p_cond, p_rep: arrays over the sites with an estimate; df)"""
    name, k0, k1, rho = R.SIM_CELLS[cell]
    rng = np.random.default_rng((2410 if not planted else 2510) + cell)
    G = k0 + k1
    out = dict(phi=[], stat_cond=[], p_cond=[], p_rep=[])
    for _ in range(R.SIM_SITES):
        if not planted:
            shares = [R.SIM_SHARE] * G if rho == 0.0 else rng.beta(R.SIM_SHARE * (1.0 - rho) / rho, (1.0 - R.SIM_SHARE) * (1.0 - rho) / rho, G)
            rows = [sr.simulate_row(rng, R.SIM_READS, R.SIM_SEP, p) for p in shares]
        else:
            means = [R.SIM_SHARE] * k0 + [R.SIM_SHARE + PLANTED[cell]] * k1
            shares = means if rho == 0.0 else [rng.beta(m * (1.0 - rho) / rho, (1.0 - m) * (1.0 - rho) / rho) for m in means]
            rows = [R._sim_site(rng, [R.SIM_READS], 1, R.SIM_SEP, p, p)[0] for p in shares]
        r = R.site(rows, k0, interval=False)
        if r['gates'] is None:
            continue
        for f in out:
            out[f].append(r[f])
    res = {f: np.array(v) for f, v in out.items()}
    res.update(df=G - 2, status=np.zeros(len(res['phi']), np.uint8))
    return res


def rates(cell, planted=False):
    """the 5 % rejection rates of p_cond, K24's p_rep and the moderated p_rep with the prior fitted on the cell, and the prior"""
    s = simulate(cell, planted)
    p = rep_prior(s['phi'], s['status'], s['df'])
    prior = record(p)
    mod = np.array([p_rep_of(st, phi_post_of(ph, prior, s['df']), 0.0, p['df_tot'])[0] for st, ph in zip(s['stat_cond'], s['phi'])])
    n = len(mod)
    return dict(p_cond=float((s['p_cond'] <= 0.05).sum()) / n, p_rep=float((s['p_rep'] <= 0.05).sum()) / n, p_mod=float((mod <= 0.05).sum()) / n,
                n=n, d0=p['d0'], s0sq=p['s0sq'], n_zero=int(p['n_zero']))
